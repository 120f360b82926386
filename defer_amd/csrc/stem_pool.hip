// Stem fusion for gfx950: 7x7/s2 Cin=3 conv + folded BN + ReLU + 3x3/s2/p1
// max-pool in one launch (ResNet50/101/152 and DenseNet121 conv1 -> pool1).
// It reads the raw input and writes only the pooled tensor: the spatial
// pre-pad pass of the stem gather and the 4x larger conv1 activation never
// touch memory.
//
// Output is bit-identical to launch_pad2d + conv_igemm_kernel<AMODE_STEM>
// followed by maxpool_kernel:
//   - same K order: (r, TR=24-element run of one zero-padded input row),
//     the stem_repack_w weights (zero for k >= 168), six 16x16x32 bf16
//     MFMAs per accumulator in ascending k from a zero accumulator; the
//     k >= 168 tail reads padded row r = 7 as the igemm gather does;
//   - same epilogue expression, rounded to bf16 BEFORE the max (the pool
//     kernel maxes bf16 values in fp32, which is exact);
//   - the same taps as maxpool_kernel (outside the conv output: none);
//     the max itself runs on the bf16 bit patterns (see the pool phase).
//
// Tiling: a block owns (image, band of pooled rows) over the full width, so
// there is no column halo and one recomputed conv row per band. It walks
// down two conv rows per step.
//   - Input: the zero-padded input rows a step needs (10 for two conv
//     rows) live in a 16-slot LDS ring (slot = padded row % 16), filled
//     with the padding folded in: a border or out-of-image element is
//     stored as zero while staging, so the k-walk has no validity math.
//     Each step adds 4 rows, loaded to registers before the step's MFMAs
//     and stored to LDS after them. Every input element is read from
//     global once per band instead of ~16 times by the fragment gather.
//   - A: fragments are read from that ring (4-byte aligned runs).
//   - B: each lane keeps ALL 24 weight fragments (4 n-frags x 6 k-steps,
//     96 VGPRs) for the whole kernel — no weight LDS, no B traffic.
//   - Conv rows: the three bf16 conv rows a pooled row needs sit in a
//     3-slot LDS ring (slot = conv row % 3), so the last row of a step is
//     the first tap of the next one.
//   - LDS: 48 KB conv ring + 25 KB input ring -> 2 blocks/CU.
#include "common.h"
#include "kernels.h"

using defer_hip::StemPoolParams;

#define SP_TPB 256
#define SP_NW (SP_TPB / WAVE)
#define SP_MAXOW 128            // conv-row width the LDS rings cover
#define SP_C 64                 // Cout
#define SP_KS 6                 // k-steps of 32 (K = 168 padded to 192)
#define SP_TR 24                // run length: ceil(7*3/8)*8
#define SP_K (7 * SP_TR)        // 168
#define SP_IR 16                // input-row ring slots
#define SP_PITCH 792            // >= 6 * (SP_MAXOW - 1) + SP_TR elements
#define SP_SROWS 4              // input rows staged per step
#define SP_SPT ((SP_PITCH + SP_TPB - 1) / SP_TPB)   // elements/thread/row

__global__ __launch_bounds__(SP_TPB, 2) void stem_pool_kernel(
    StemPoolParams p) {
    const bf16* __restrict__ X = (const bf16*)p.x;
    const bf16* __restrict__ Wp = (const bf16*)p.wp;
    bf16* __restrict__ OUT = (bf16*)p.out;

    // conv-row ring [slot][col][64 ch]; the 32-byte channel groups of a
    // column are XOR-swizzled by (col >> 2) & 3 so the four 4-column
    // groups of an accumulator write hit different banks
    __shared__ __attribute__((aligned(16)))
    bf16 ring[3 * SP_MAXOW * SP_C];
    // zero-padded input rows [slot][element], element = pixel * 3 + c
    __shared__ __attribute__((aligned(16)))
    bf16 inr[SP_IR * SP_PITCH];

    const int tid = threadIdx.x;
    // wave-uniform by construction; say so, or the per-wave task loop
    // compiles to exec-masked branches
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int lane = tid % WAVE;
    const int lo16 = lane & 15;
    const int hi4 = lane >> 4;

    // ---- weights: all fragments resident in registers
    bf16x8 bfr[4][SP_KS];
    float sc[4], bi[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int n = ni * 16 + lo16;
        sc[ni] = p.scale[n];
        bi[ni] = p.bias[n];
#pragma unroll
        for (int ks = 0; ks < SP_KS; ++ks) {
            const int k = ks * 32 + hi4 * 8;
            bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            bfr[ni][ks] = (k < SP_K) ? load_bf16x8(Wp + n * SP_K + k) : z;
        }
    }

    // ---- A lane geometry: k = ks*32 + hi4*8 -> (padded row r, run
    // offset t), both constant per lane and k-step
    int kr[SP_KS], kt[SP_KS];
#pragma unroll
    for (int ks = 0; ks < SP_KS; ++ks) {
        const int k = ks * 32 + hi4 * 8;
        kr[ks] = k / SP_TR;
        kt[ks] = k % SP_TR;
    }

    const int MF = (p.OW + 15) / 16;            // m-fragments per conv row
    const int LEN = 6 * (p.OW - 1) + SP_TR;     // staged elements per row
    const int W3 = p.W * 3;
    const int items = p.NB * p.bands;

    // ---- input staging: padded rows [pa, pa + n), n <= SP_SROWS, of the
    // image at xn. Padded row pr is input row pr - 3, padded element e is
    // input element e - 9; everything outside the image is zero.
    bf16 sv[SP_SROWS][SP_SPT];
    auto stage_load = [&](const bf16* xn, int pa, int n) {
#pragma unroll
        for (int i = 0; i < SP_SROWS; ++i) {
            const int ih = pa + i - 3;
            const bool rowok = i < n && ih >= 0 && ih < p.H;
            const bf16* src = xn + (long)(rowok ? ih : 0) * W3;
#pragma unroll
            for (int j = 0; j < SP_SPT; ++j) {
                const int e = tid + j * SP_TPB - 9;
                sv[i][j] = (rowok && e >= 0 && e < W3) ? src[e] : (bf16)0.f;
            }
        }
    };
    auto stage_store = [&](int pa, int n) {
#pragma unroll
        for (int i = 0; i < SP_SROWS; ++i) {
            if (i >= n) continue;
            bf16* dst = inr + ((pa + i) & (SP_IR - 1)) * SP_PITCH;
#pragma unroll
            for (int j = 0; j < SP_SPT; ++j) {
                const int e = tid + j * SP_TPB;
                if (e < LEN) dst[e] = sv[i][j];
            }
        }
    };

    // task t of a step that starts at conv row r0: (row r0 + t / MF,
    // m-fragment t % MF)
    auto compute = [&](int r0, int t) {
        const int dr = t >= MF ? 1 : 0;
        const int mf = t - dr * MF;
        int colA = mf * 16 + lo16;
        if (colA >= p.OW) colA = p.OW - 1;      // clamped, never pooled
        const int prow = 2 * (r0 + dr);
        bf16x8 a[SP_KS];
#pragma unroll
        for (int ks = 0; ks < SP_KS; ++ks) {
            // 16 bytes at a 4-byte-aligned LDS address
            const void* q = __builtin_assume_aligned(
                inr + ((prow + kr[ks]) & (SP_IR - 1)) * SP_PITCH +
                    colA * 6 + kt[ks], 4);
            __builtin_memcpy(&a[ks], q, 16);
        }
        f32x4 acc[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[ni] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < SP_KS; ++ks)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                acc[ni] = MFMA_BF16_16x16x32(a[ks], bfr[ni][ks], acc[ni]);
        bf16* row = ring + ((r0 + dr) % 3) * (SP_MAXOW * SP_C);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int col = mf * 16 + hi4 * 4 + e;  // (col >> 2) & 3 == hi4
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int c = (ni * 16 + lo16) ^ (hi4 << 4);
                float v = acc[ni][e] * sc[ni] + bi[ni];
                row[col * SP_C + c] = f2bf(apply_act(v, ACT_RELU));
            }
        }
    };

    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int nb = item / p.bands;
        const int band = item - nb * p.bands;
        const int p0 = band * p.rpb;
        const int p1 = min(p0 + p.rpb, p.POH);   // exclusive
        const bf16* xn = X + (long)nb * p.H * W3;

        // steps: s = -1 is the halo row 2*p0-1 (bands below the first);
        // s >= 0 computes conv rows 2p, 2p+1 of pooled row p = p0 + s
        const int s_first = p0 > 0 ? -1 : 0;
        const int s_end = p1 - p0;
        auto step_r0 = [&](int s) { return s < 0 ? 2 * p0 - 1 : 2 * (p0 + s); };
        auto step_nr = [&](int s) {
            return s < 0 ? 1 : min(2, p.OH - step_r0(s));
        };
        // one past the last padded row a step reads: conv row r reads
        // padded rows 2r .. 2r+7 (row 7 against the zero-weight tail)
        auto step_hi = [&](int s) {
            return 2 * (step_r0(s) + step_nr(s) - 1) + 8;
        };

        // fill the window of the first step; the previous item's last
        // barrier has retired every read of both rings
        int staged = 2 * step_r0(s_first);
        for (const int hi = step_hi(s_first); staged < hi;
             staged += SP_SROWS) {
            const int n = min(SP_SROWS, hi - staged);
            stage_load(xn, staged, n);
            stage_store(staged, n);
        }
        staged = step_hi(s_first);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();

        for (int s = s_first; s < s_end; ++s) {
            const int r0 = step_r0(s);
            const int nt = step_nr(s) * MF;
            // next step's new input rows: loads fly under this step's
            // MFMAs. Their slots hold rows at least 6 below this step's
            // window (16 slots, <= 14 rows from this window's first row
            // to the next window's last), so storing needs no barrier
            const int nhi = s + 1 < s_end ? step_hi(s + 1) : staged;
            const int nnew = nhi - staged;       // 0..SP_SROWS
            stage_load(xn, staged, nnew);
#pragma unroll 1
            for (int t = wave; t < nt; t += SP_NW) compute(r0, t);
            stage_store(staged, nnew);
            staged = nhi;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();   // conv rows + input rows visible
            if (s >= 0) {
                const int pr = p0 + s;
                bf16* orow = OUT + ((long)nb * p.POH + pr) * p.POW * SP_C;
#pragma unroll 1
                for (int i = tid; i < p.POW * 8; i += SP_TPB) {
                    const int q = i >> 3, c8 = i & 7;
                    // Every conv value is a ReLU output: +0, a positive
                    // bf16, or -0 at worst. On those bit patterns the
                    // signed 16-bit integer order IS the float order
                    // (-0 = 0x8000 sorts lowest, as fmaxf ranks it), so
                    // the max runs packed, two channels per instruction,
                    // with no bf16 -> f32 unpacking; the bits that come
                    // out are the ones maxpool_kernel's fp32 max selects.
                    // A tap outside the conv output (maxpool_kernel skips
                    // it) re-reads the window centre instead: always
                    // inside, and max is idempotent, so the nine LDS reads
                    // issue back to back without branches.
                    s16x8 best;
#pragma unroll
                    for (int dr = -1; dr <= 1; ++dr) {
                        int r = 2 * pr + dr;
                        if (r < 0 || r >= p.OH) r = 2 * pr;
                        const bf16* row =
                            ring + (r % 3) * (SP_MAXOW * SP_C);
#pragma unroll
                        for (int dc = -1; dc <= 1; ++dc) {
                            int c = 2 * q + dc;
                            if (c < 0 || c >= p.OW) c = 2 * q;
                            const s16x8 v = __builtin_bit_cast(
                                s16x8,
                                load_bf16x8(
                                    row + c * SP_C +
                                    ((c8 * 8) ^ (((c >> 2) & 3) << 4))));
                            best = (dr == -1 && dc == -1)
                                       ? v
                                       : __builtin_elementwise_max(best, v);
                        }
                    }
                    const bf16x8 o = __builtin_bit_cast(bf16x8, best);
                    store_bf16x8(orow + q * SP_C + c8 * 8, o);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();      // ring slots reusable
            }
        }
    }
}

namespace defer_hip {

bool stem_pool_supported(int Cin, int Cout, int R, int S, int stride,
                         int pad, bool relu, int pk, int ps, int pp,
                         int OH, int OW) {
    return Cin == 3 && Cout == SP_C && R == 7 && S == 7 && stride == 2 &&
           pad == 3 && relu && pk == 3 && ps == 2 && pp == 1 && OH >= 1 &&
           OW >= 1 && OW <= SP_MAXOW;
}

StemPoolParams launch_stem_pool(const StemPoolParams& p0, int max_blocks,
                                hipStream_t s) {
    StemPoolParams p = p0;
    // 2 blocks fit a CU, 512 on the chip. Split each image into bands so
    // that there are about 512 (image, band) items and every block walks
    // one: 768 items ran as two rounds, the second half empty. One conv
    // row is recomputed per band.
    int bands = (512 + p.NB - 1) / p.NB;
    if (bands > p.POH) bands = p.POH;
    if (bands < 1) bands = 1;
    p.rpb = (p.POH + bands - 1) / bands;
    p.bands = (p.POH + p.rpb - 1) / p.rpb;
    long items = (long)p.NB * p.bands;
    int grid = (int)(items < 512 ? items : 512);
    if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
    hipLaunchKernelGGL(stem_pool_kernel, dim3(grid), dim3(SP_TPB), 0, s, p);
    return p;
}

}  // namespace defer_hip
