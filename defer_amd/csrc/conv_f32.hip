// fp32 implicit-GEMM convolution for gfx950 on the exact f32-input MFMA
// (v_mfma_f32_32x32x2_f32): fp32 NHWC activations, fp32 OHWI weights,
// fp32 output, y = act(acc*scale[c] + bias[c] + res).
//
// The accuracy path (PipelineConfig(dtype="fp32")): each output element
// is a k-ordered f32 fmaf chain, one rounding per product, no split-K
// and no atomics, so results are run-to-run deterministic. This is a
// simple double-buffered kernel, separate from the tuned bf16 pipeline
// in conv.hip.
//
// Tiling. 256 threads = 2x2 waves; block tile BM (pixels) x BN (couts)
// x BK = 32. Both tiles are staged global -> registers -> LDS as float4
// chunks, [rows][BK + 4] floats. The 144-B row stride makes every float4
// access conflict-free: 8 consecutive rows (fragment reads) or the 8
// chunks of one row (staging writes) each cover all 32 banks once.
//
// Operand roles are swapped relative to the usual GEMM: weights are the
// MFMA "A" operand (row i = cout) and activations the "B" operand
// (col j = pixel). A lane then holds one pixel and, in accumulator
// registers 4g..4g+3, four CONSECUTIVE couts (8g + 4*(lane>>5) + 0..3),
// which is what a float4 along Cout needs.
//
// k order inside one 8-wide step: lane (idx = lane&31, h = lane>>5)
// reads float4 tile[idx][8q + 4h .. +3] and feeds element j to MFMA j,
// so MFMA j sums k = {8q + j, 8q + 4 + j}. Both operands use the same
// map, so the products pair up correctly; the summation order is a fixed
// permutation of k.
//
// Epilogue: accumulators go through LDS ([BM][BN + 4], reusing the tile
// buffers) and come back row-major, so scale/bias/residual/act run on
// float4s and each row is written with contiguous 16-byte stores.
//
// Addressing: every global access is float* + 64-bit element index.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int F32_TPB = 256;
constexpr int F32_BK = 32;
constexpr int F32_LDK = F32_BK + 4;   // padded LDS row, floats

template <int BM, int BN>
constexpr int conv_f32_lds_bytes() {
    constexpr int tiles = 2 * (BM + BN) * F32_LDK * 4;
    constexpr int stage = BM * (BN + 4) * 4;
    return tiles > stage ? tiles : stage;
}

template <int BM, int BN, bool GEMM>
__global__ __launch_bounds__(F32_TPB) void conv_f32_kernel(
    defer_hip::ConvF32Params p) {
    constexpr int BK = F32_BK, LDK = F32_LDK;
    constexpr int WM = BM / 2, WN = BN / 2;     // wave tile
    constexpr int TM = WM / 32, TN = WN / 32;   // 32x32 MFMA tiles per wave
    constexpr int AI = BM * (BK / 4) / F32_TPB; // float4 chunks per thread
    constexpr int BI = BN * (BK / 4) / F32_TPB;
    constexpr int LDC = BN + 4;
    static_assert(TM >= 1 && TN >= 1 && AI >= 1 && BI >= 1, "tile too small");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [2][BM][LDK] activations
    float* Bs = smem + 2 * BM * LDK;        // [2][BN][LDK] weights

    const float* __restrict__ X = p.x;
    const float* __restrict__ Wt = p.w;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int M = p.M, K = p.K, Cout = p.Cout;

    // staging map: chunk = tid + 256*i -> row = (tid>>3) + 32*i, k4 = tid&7
    const int srow = tid >> 3, sk = (tid & 7) * 4;

    // per-row gather state (fixed over the K loop)
    long abase[AI];   // GEMM: row offset; conv: image offset (elements)
    int aih0[AI], aiw0[AI];
    bool aval[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        int m = m0 + srow + 32 * i;
        aval[i] = m < M;
        if (GEMM) {
            abase[i] = (long)m * K;
            aih0[i] = aiw0[i] = 0;
        } else {
            int mm = aval[i] ? m : 0;
            int ow = mm % p.OW;
            int t = mm / p.OW;
            int oh = t % p.OH;
            int n = t / p.OH;
            abase[i] = (long)n * p.H * p.W * p.Cin;
            aih0[i] = oh * p.stride - p.pad;
            aiw0[i] = ow * p.stride - p.pad;
        }
    }
    long bbase[BI];
    bool bval[BI];
#pragma unroll
    for (int i = 0; i < BI; ++i) {
        int n = n0 + srow + 32 * i;
        bval[i] = n < Cout;
        bbase[i] = (long)n * K;
    }

    f32x4 ra[AI], rb[BI];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    auto load_tile = [&](int kt) {
        const int k = kt * BK + sk;          // K % 4 == 0: whole chunk valid
        const bool kval = k < K;
        int r = 0, s = 0, c = k;
        if (!GEMM) {
            int rs = k / p.Cin;
            c = k - rs * p.Cin;
            r = rs / p.S;
            s = rs - r * p.S;
        }
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            f32x4 v = zero4;
            if (GEMM) {
                if (aval[i] && kval)
                    v = *reinterpret_cast<const f32x4*>(X + abase[i] + k);
            } else {
                int ih = aih0[i] + r, iw = aiw0[i] + s;
                if (aval[i] && kval && ih >= 0 && ih < p.H && iw >= 0 &&
                    iw < p.W)
                    v = *reinterpret_cast<const f32x4*>(
                        X + abase[i] + ((long)ih * p.W + iw) * p.Cin + c);
            }
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < BI; ++i) {
            f32x4 v = zero4;
            if (bval[i] && kval)
                v = *reinterpret_cast<const f32x4*>(Wt + bbase[i] + k);
            rb[i] = v;
        }
    };
    auto store_tile = [&](int buf) {
        float* a = As + buf * BM * LDK;
        float* b = Bs + buf * BN * LDK;
#pragma unroll
        for (int i = 0; i < AI; ++i)
            *reinterpret_cast<f32x4*>(a + (srow + 32 * i) * LDK + sk) = ra[i];
#pragma unroll
        for (int i = 0; i < BI; ++i)
            *reinterpret_cast<f32x4*>(b + (srow + 32 * i) * LDK + sk) = rb[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int fidx = lane & 31, fh = lane >> 5;
    const int nk = (K + BK - 1) / BK;

    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tile(kt + 1);
        const float* a = As + buf * BM * LDK + (wm * WM + fidx) * LDK + 4 * fh;
        const float* b = Bs + buf * BN * LDK + (wn * WN + fidx) * LDK + 4 * fh;
#pragma unroll
        for (int q = 0; q < BK / 8; ++q) {
            f32x4 xa[TM], wb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                xa[i] = *reinterpret_cast<const f32x4*>(a + i * 32 * LDK + 8 * q);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                wb[j] = *reinterpret_cast<const f32x4*>(b + j * 32 * LDK + 8 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                            wb[j][e], xa[i][e], acc[i][j], 0, 0, 0);
        }
        // the other buffer was last read in iteration kt-1, and every
        // wave has passed that iteration's barrier
        if (kt + 1 < nk) store_tile(buf ^ 1);
        __syncthreads();
    }

    // accumulators -> LDS [BM][LDC]; lane = pixel, regs 4g..4g+3 = couts
    float* Cs = smem;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1],
                           acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                int ml = wm * WM + i * 32 + fidx;
                int nl = wn * WN + j * 32 + 8 * g + 4 * fh;
                *reinterpret_cast<f32x4*>(Cs + ml * LDC + nl) = v;
            }
    __syncthreads();

    const float* __restrict__ scale = p.scale;
    const float* __restrict__ bias = p.bias;
    const float* __restrict__ res = p.res;
    float* __restrict__ out = p.out;
    constexpr int NC = BN / 4;               // float4 chunks per tile row
#pragma unroll 4
    for (int ch = tid; ch < BM * NC; ch += F32_TPB) {
        int ml = ch / NC, nl = (ch % NC) * 4;
        int m = m0 + ml, n = n0 + nl;
        if (m >= M || n >= Cout) continue;   // Cout % 4 == 0: whole chunk
        f32x4 v = *reinterpret_cast<const f32x4*>(Cs + ml * LDC + nl);
        if (scale) v = v * *reinterpret_cast<const f32x4*>(scale + n);
        if (bias) v = v + *reinterpret_cast<const f32x4*>(bias + n);
        long o = (long)m * Cout + n;
        if (res) v = v + *reinterpret_cast<const f32x4*>(res + o);
        if (p.relu == ACT_HARDSWISH) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = hardswish_f(v[e]);
        } else if (p.relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        if (p.relu == ACT_RELU6) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fminf(v[e], 6.f);
        }
        *reinterpret_cast<f32x4*>(out + o) = v;
    }
}

// zero-pad the channel (last) dim C -> C4 of [rows][C] fp32
__global__ void pad_channels_f32_kernel(const float* __restrict__ x,
                                        float* __restrict__ y, long rows,
                                        int C, int C4) {
    long total = rows * C4;
    long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long gstride = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total; i += gstride) {
        long r = i / C4;
        int c = (int)(i - r * C4);
        y[i] = c < C ? x[r * C + c] : 0.f;
    }
}

template <int BM, int BN, bool GEMM>
void launch_tile(const defer_hip::ConvF32Params& p, hipStream_t s) {
    constexpr int lds = conv_f32_lds_bytes<BM, BN>();
    static bool attr_set = [] {
        // > 64 KiB of dynamic LDS needs the opt-in, once per kernel
        return hipFuncSetAttribute(
                   reinterpret_cast<const void*>(&conv_f32_kernel<BM, BN, GEMM>),
                   hipFuncAttributeMaxDynamicSharedMemorySize,
                   lds) == hipSuccess;
    }();
    (void)attr_set;
    dim3 grid((p.M + BM - 1) / BM, (p.Cout + BN - 1) / BN);
    hipLaunchKernelGGL((conv_f32_kernel<BM, BN, GEMM>), grid, dim3(F32_TPB),
                       lds, s, p);
}

}  // namespace

namespace defer_hip {

void launch_conv_f32(const ConvF32Params& p, bool gemm_mode, int tile,
                     hipStream_t s) {
    // 128x128 amortizes each LDS fragment over the most MFMAs; the narrow
    // 128x64 tile serves Cout <= 64 (no half-empty n-tile) and grids that
    // would otherwise leave most of the 256 CUs without a block.
    bool narrow;
    if (tile == 1) narrow = false;
    else if (tile == 2) narrow = true;
    else {
        long blocks_wide = (long)((p.M + 127) / 128) * ((p.Cout + 127) / 128);
        narrow = p.Cout <= 64 || blocks_wide < 256;
    }
    if (narrow) {
        if (gemm_mode) launch_tile<128, 64, true>(p, s);
        else launch_tile<128, 64, false>(p, s);
    } else {
        if (gemm_mode) launch_tile<128, 128, true>(p, s);
        else launch_tile<128, 128, false>(p, s);
    }
}

void launch_pad_channels_f32(const float* x, float* y, long rows, int C,
                             int C4, hipStream_t s) {
    long total = rows * C4;
    long g = (total + 255) / 256;
    hipLaunchKernelGGL(pad_channels_f32_kernel,
                       dim3((int)(g < 2048 ? g : 2048)), dim3(256), 0, s, x,
                       y, rows, C, C4);
}

}  // namespace defer_hip
