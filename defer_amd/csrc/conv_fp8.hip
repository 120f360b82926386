// fp8 (OCP e4m3, torch.float8_e4m3fn) convolution for gfx950 (CDNA4) on
// v_mfma_f32_16x16x128_f8f6f4, and the quantiser that feeds it.
//
// conv_fp8_kernel: implicit GEMM, C[M, N] = A[M, K] x B[K, N] with
//   M = NB*OH*OW output pixels, N = Cout, K = R*S*Cin bytes,
//   A row m = the NHWC e4m3 input patch of pixel m, gathered on the fly,
//   B = OHWI e4m3 weights, so B^T rows are K contiguous bytes.
// fp32 accumulation; for output channel c the epilogue computes, in fp32,
//   v = clamp(acc * scale[c] + bias[c] + res_scale * float(res_q), lo, hi)
// ((lo, hi) = (-inf, +inf) none, (0, +inf) relu, (0, 6) relu6) and writes
// either e4m3(clamp(v * out_inv_scale, -448, 448)), round-to-nearest-even,
// or one bf16 rounding of v. res_scale and out_inv_scale are kernel
// arguments: no host sync, capturable.
//
// Work split. A workgroup of four waves owns a BM x BN output tile (128x128
// or 64x64, plan_conv_fp8) and walks tiles grid-stride, n fastest so the
// workgroups of one wavefront of tiles share A rows in L2. The waves sit
// 2 x 2; a wave owns (BM/2) x (BN/2) as MI x NI 16x16 accumulators (4 x 4 or
// 2 x 2), so one K-tile costs MI + NI fragment reads for MI * NI MFMAs.
//
// K-tile = 128 bytes per row = one MFMA K step. An LDS tile row is 128 B = 8
// pieces of 16 B; logical piece q of row r lives at physical piece
// q ^ (r & 7). Staging is global_load_lds, 16 B a lane: a wave instruction
// fills 8 consecutive rows (1 KiB, lane-linear), so lane l writes physical
// piece l & 7 of row l >> 3 and therefore FETCHES logical piece
// (l & 7) ^ (l >> 3) -- the swizzle is applied to the source. Cin % 16 == 0,
// so a piece never straddles a filter tap: its (r, s, c) comes from one
// k / Cin and one tap / S per lane per K-tile, shared by all the rows the
// lane stages. A piece outside the image, past row M, past Cout or past K
// (K is rounded up to 128 only in the loop count) is fetched from a 16-byte
// zero buffer instead: e4m3 zero is the zero byte, so padding needs no scale
// and no packed copy of the weights.
//
// Pipeline: two LDS stages, one barrier per K-tile. Iteration kt waits for
// tile kt (vmcnt(0) + barrier), reads its MI + NI fragments into registers,
// THEN issues the loads of tile kt + 1 into the other stage (every wave has
// passed this barrier only after its reads of tile kt - 1, which lived
// there) and runs the MFMAs under those loads. Two workgroups share a CU
// (64 KiB LDS each at 128x128), so one's barrier wait is the other's MFMA
// time.
//
// MFMA operands, v_mfma_f32_16x16x128_f8f6f4 with cbsz = blgp = 0 (e4m3 both
// sides) and zero scale operands, which hipcc lowers to the unscaled
// instruction. Each lane supplies 32 bytes of A and 32 of B. Lane l reads
// row (l & 15) of the fragment and the 32 contiguous K bytes 32*(l >> 4) ..
// 32*(l >> 4) + 31 of the K-tile, as two 16-byte LDS reads, the same mapping
// for A and for B. The sum over K does not depend on how the instruction
// orders those 128 products as long as A and B agree, which the shared read
// code guarantees; what the exact-integer GPU test (tests/
// test_conv_fp8_gpu.py) pins down is the part that does matter: operand row
// = l & 15 on both sides, and the accumulator layout acc[j] = C[4*(l >> 4) +
// j][l & 15], the one of the bf16 16x16x32 MFMA.
//
// K < 128 (NARROW, plan_conv_fp8): the reduction is a zero-padded part of one
// MFMA K step. The fp8 instruction sums the products inside a step with fewer
// bits than an fp32 chain (docs/STATE.md, "fp8 MFMA accumulation"), an error
// that does not shrink with K, while a (K + 7) * 2^-24 bound does; there is
// no rate to gain on a mostly padded step either. Such a conv keeps the
// staging, the LDS tile and the fragment reads, widens each lane's 32 bytes
// to bf16 in registers (exact) and runs four v_mfma_f32_16x16x32_bf16: step
// j takes bytes 8j .. 8j + 7 of every lane, for A and B alike, so lane group
// g's slot i of step j is k = 32 g + 8 j + i on both sides. Same operand
// rows, same accumulator layout.
//
// Epilogue: per 16-row strip a wave bounces its fp32 accumulators through
// LDS (row pitch BN/2 + 4 floats) and re-reads them so a lane owns 16
// consecutive channels of one pixel: one 16-byte residual load, four float4
// scale / bias loads, one 16-byte store of 16 e4m3 or two of 8 bf16.
// Accumulation order is fixed (K-tiles in order, no split-K, no atomics):
// run-to-run identical.
//
// quantize_fp8_kernel: bf16 or fp32 -> e4m3 of clamp(x * inv_scale, +-448),
// 16 values a lane per step (16-byte loads, one 16-byte store), grid-stride.
#include "common.h"
#include "kernels.h"

// no packed fp32 instructions in this file's kernels
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

using defer_hip::ConvFp8Params;

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int F8_TPB = 256;
constexpr int F8_BK = 128;          // bytes of K per tile row
constexpr int F8_GRID_CAP = 512;    // workgroups: 2 per CU

__device__ __forceinline__ void glds16_u8(const u8* src, u8* lds_base) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)lds_base, 16, 0, 0);
}

// 16 fp32 -> 16 e4m3 bytes of clamp(v * inv, -448, 448), RNE
__device__ __forceinline__ u32x4 pack16_e4m3(const float* v, float inv) {
    u32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            a[e] = fminf(fmaxf(v[4 * q + e] * inv, -448.0f), 448.0f);
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(a[0], a[1], 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(a[2], a[3], w, true);
        o[q] = (u32)w;
    }
    return o;
}

// 8 e4m3 bytes -> 8 bf16, exact: an e4m3 value has at most 4 significant bits
// and an exponent inside bf16's, so the high half of its fp32 is the value
__device__ __forceinline__ bf16x8 e4m3x8_to_bf16(int w0, int w1) {
    u32x4 o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int w = h ? w1 : w0;
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
        const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
        o[2 * h] = (__float_as_uint(lo[0]) >> 16) |
                   (__float_as_uint(lo[1]) & 0xffff0000u);
        o[2 * h + 1] = (__float_as_uint(hi[0]) >> 16) |
                       (__float_as_uint(hi[1]) & 0xffff0000u);
    }
    return __builtin_bit_cast(bf16x8, o);
}

template <int BM, int BN, bool NARROW>
__global__ __launch_bounds__(F8_TPB, 2) void conv_fp8_kernel(
    ConvFp8Params p) {
    constexpr int WM = BM / 2, WN = BN / 2;     // wave tile
    constexpr int MI = WM / 16, NI = WN / 16;   // fragments per wave
    constexpr int ACH = BM * 8 / F8_TPB;        // A pieces per lane per tile
    constexpr int BCH = BN * 8 / F8_TPB;
    constexpr int TA = BM * F8_BK, TB = BN * F8_BK;
    constexpr int EP = WN + 4;                  // epilogue row pitch, floats
    constexpr int CG = WN / 16;                 // 16-channel groups per strip
    static_assert(4 * 16 * EP * 4 <= 2 * (TA + TB), "epilogue fits the ring");

    __shared__ __attribute__((aligned(16))) u8 lds[2 * (TA + TB)];

    const u8* __restrict__ X = p.x;
    const u8* __restrict__ Wt = p.w;
    const u8* __restrict__ Z = (const u8*)p.zbuf;

    const int tid = threadIdx.x;
    const int wave = tid / WAVE, lane = tid % WAVE;
    const int wm = wave >> 1, wn = wave & 1;
    const int srow = lane >> 3;                         // staged row & 7
    const int kpiece = ((lane & 7) ^ srow) * 16;        // logical k offset
    const int frow = lane & 15;                         // fragment row
    const int fq = (lane >> 4) * 2;                     // first logical piece
    const int ohow = p.OH * p.OW;
    const int KT = (p.K + F8_BK - 1) / F8_BK;
    const int ntiles = p.ntm * p.ntn;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tm = tile / p.ntn, tn = tile - tm * p.ntn;

        // the rows this lane stages: pixel -> (image row base, ih0, iw0)
        int a_pix[ACH], a_ih0[ACH], a_iw0[ACH];
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const int m = tm * BM + (i * 4 + wave) * 8 + srow;
            const int img = m / ohow, rem = m - img * ohow;
            const int oh = rem / p.OW, ow = rem - oh * p.OW;
            a_pix[i] = img * p.H;
            // a row past M fails every bounds check below
            a_ih0[i] = m < p.M ? oh * p.stride - p.pad : -(1 << 20);
            a_iw0[i] = ow * p.stride - p.pad;
        }

        auto stage = [&](int kt, int buf) {
            u8* As = lds + buf * (TA + TB);
            u8* Bs = As + TA;
            const int k = kt * F8_BK + kpiece;
            const bool kok = k < p.K;
            const int tap = k / p.Cin, c = k - tap * p.Cin;
            const int r = tap / p.S, s = tap - r * p.S;
#pragma unroll
            for (int i = 0; i < ACH; ++i) {
                const int ih = a_ih0[i] + r, iw = a_iw0[i] + s;
                const bool ok = kok && (unsigned)ih < (unsigned)p.H &&
                                (unsigned)iw < (unsigned)p.W;
                const u8* src = ok
                    ? X + ((long)(a_pix[i] + ih) * p.W + iw) * p.Cin + c
                    : Z;
                glds16_u8(src, As + (i * 4 + wave) * 8 * F8_BK);
            }
#pragma unroll
            for (int i = 0; i < BCH; ++i) {
                const int n = tn * BN + (i * 4 + wave) * 8 + srow;
                const u8* src = kok && n < p.Cout ? Wt + (long)n * p.K + k
                                                  : Z;
                glds16_u8(src, Bs + (i * 4 + wave) * 8 * F8_BK);
            }
        };

        f32x4 acc[MI][NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
                acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

        stage(0, 0);
        for (int kt = 0; kt < KT; ++kt) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            const u8* As = lds + (kt & 1) * (TA + TB);
            const u8* Bs = As + TA;
            i32x8 af[MI], bf[NI];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const int row = wm * WM + mi * 16 + frow;
                const u8* rp = As + row * F8_BK;
                const u32x4 lo = *(const u32x4*)(rp + ((fq ^ (row & 7)) << 4));
                const u32x4 hi =
                    *(const u32x4*)(rp + (((fq + 1) ^ (row & 7)) << 4));
                af[mi] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3],
                               (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int row = wn * WN + ni * 16 + frow;
                const u8* rp = Bs + row * F8_BK;
                const u32x4 lo = *(const u32x4*)(rp + ((fq ^ (row & 7)) << 4));
                const u32x4 hi =
                    *(const u32x4*)(rp + (((fq + 1) ^ (row & 7)) << 4));
                bf[ni] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3],
                               (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            }
            // the fragments are in registers before the next tile's loads
            // are issued, so no LDS read waits on a load in flight
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (kt + 1 < KT) stage(kt + 1, (kt + 1) & 1);
            if constexpr (NARROW) {
                // K < 128: step j multiplies bytes 8j .. 8j + 7 of every
                // lane's 32, widened to bf16, on the bf16 MFMA
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bf16x8 ah[MI], bh[NI];
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
                        ah[mi] = e4m3x8_to_bf16(af[mi][2 * j],
                                                af[mi][2 * j + 1]);
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        bh[ni] = e4m3x8_to_bf16(bf[ni][2 * j],
                                                bf[ni][2 * j + 1]);
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                        for (int ni = 0; ni < NI; ++ni)
                            acc[mi][ni] = MFMA_BF16_16x16x32(
                                ah[mi], bh[ni], acc[mi][ni]);
                }
            } else {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        acc[mi][ni] =
                            __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                                af[mi], bf[ni], acc[mi][ni], 0, 0, 0, 0, 0, 0);
            }
        }

        // epilogue, a 16-row strip of the wave tile at a time
        float* E = (float*)lds + wave * 16 * EP;
        const int er = lane / CG, eg = lane - er * CG;  // row, channel group
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            __syncthreads();    // ring (first strip) or strip reads done
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    E[((lane >> 4) * 4 + j) * EP + ni * 16 + frow] =
                        acc[mi][ni][j];
            __syncthreads();
            const int m = tm * BM + wm * WM + mi * 16 + er;
            const int c0 = tn * BN + wn * WN + eg * 16;
            if (lane < 16 * CG && m < p.M && c0 < p.Cout) {
                float v[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 a = *(const f32x4*)(E + er * EP + eg * 16 +
                                                    4 * q);
                    const f32x4 sc = *(const f32x4*)(p.scale + c0 + 4 * q);
                    const f32x4 bi = *(const f32x4*)(p.bias + c0 + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        v[4 * q + e] = a[e] * sc[e] + bi[e];
                }
                const long o = (long)m * p.Cout + c0;
                if (p.res) {
                    const u32x4 rq = *(const u32x4*)(p.res + o);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        v[4 * q + 0] += p.res_scale *
                            __builtin_amdgcn_cvt_f32_fp8((int)rq[q], 0);
                        v[4 * q + 1] += p.res_scale *
                            __builtin_amdgcn_cvt_f32_fp8((int)rq[q], 1);
                        v[4 * q + 2] += p.res_scale *
                            __builtin_amdgcn_cvt_f32_fp8((int)rq[q], 2);
                        v[4 * q + 3] += p.res_scale *
                            __builtin_amdgcn_cvt_f32_fp8((int)rq[q], 3);
                    }
                }
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    v[e] = fminf(fmaxf(v[e], p.act_lo), p.act_hi);
                if (p.out_fp8) {
                    *(u32x4*)((u8*)p.out + o) =
                        pack16_e4m3(v, p.out_inv_scale);
                } else {
                    bf16x8 h0, h1;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        h0[e] = f2bf(v[e]);
                        h1[e] = f2bf(v[8 + e]);
                    }
                    bf16* op = (bf16*)p.out + o;
                    store_bf16x8(op, h0);
                    store_bf16x8(op + 8, h1);
                }
            }
        }
        __syncthreads();        // strip reads done before the next staging
    }
}

template <typename T>
__global__ __launch_bounds__(256) void quantize_fp8_kernel(
    const T* __restrict__ x, u8* __restrict__ y, long n16, float inv) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < n16; i += (long)gridDim.x * blockDim.x) {
        float v[16];
        if constexpr (sizeof(T) == 2) {
            const bf16x8 a = load_bf16x8((const bf16*)x + 16 * i);
            const bf16x8 b = load_bf16x8((const bf16*)x + 16 * i + 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v[e] = bf2f(a[e]);
                v[8 + e] = bf2f(b[e]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 a = *(const f32x4*)((const float*)x + 16 * i +
                                                4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[4 * q + e] = a[e];
            }
        }
        *(u32x4*)(y + 16 * i) = pack16_e4m3(v, inv);
    }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

namespace defer_hip {

ConvFp8Plan plan_conv_fp8(long M, int Cout, int K, int max_blocks) {
    ConvFp8Plan pl;
    // the 128x128 tile where it fills: at least one full tile each way
    // (every ResNet layer 2-4 conv at batch >= 1); 64x64 for few rows or
    // narrow Cout, where a large tile would multiply mostly padding
    const bool large = M >= 128 && Cout >= 128;
    pl.bm = pl.bn = large ? 128 : 64;
    pl.ntm = (int)((M + pl.bm - 1) / pl.bm);
    pl.ntn = (Cout + pl.bn - 1) / pl.bn;
    pl.ktiles = (K + F8_BK - 1) / F8_BK;
    // a reduction shorter than one MFMA K step: the fp8 instruction's error
    // does not shrink with K, the bound a caller may hold it to does
    pl.narrow = K < F8_BK;
    pl.lds_bytes = 2 * (pl.bm + pl.bn) * F8_BK;
    const long tiles = (long)pl.ntm * pl.ntn;
    const long cap = max_blocks > 0 ? max_blocks : F8_GRID_CAP;
    pl.grid = (int)(tiles < cap ? tiles : cap);
    return pl;
}

ConvFp8Plan launch_conv_fp8(ConvFp8Params p, int max_blocks, hipStream_t s) {
    const ConvFp8Plan pl = plan_conv_fp8(p.M, p.Cout, p.K, max_blocks);
    p.ntm = pl.ntm;
    p.ntn = pl.ntn;
    const dim3 grid(pl.grid), block(F8_TPB);
    if (pl.bm == 128 && pl.narrow)
        hipLaunchKernelGGL((conv_fp8_kernel<128, 128, true>), grid, block, 0,
                           s, p);
    else if (pl.bm == 128)
        hipLaunchKernelGGL((conv_fp8_kernel<128, 128, false>), grid, block, 0,
                           s, p);
    else if (pl.narrow)
        hipLaunchKernelGGL((conv_fp8_kernel<64, 64, true>), grid, block, 0, s,
                           p);
    else
        hipLaunchKernelGGL((conv_fp8_kernel<64, 64, false>), grid, block, 0,
                           s, p);
    return pl;
}

void launch_quantize_fp8(const void* x, void* y, long n, bool f32,
                         float inv_scale, int max_blocks, hipStream_t s) {
    const long n16 = n / 16;
    long grid = (n16 + 255) / 256;
    const long cap = max_blocks > 0 ? max_blocks : 2048;
    if (grid > cap) grid = cap;
    if (f32)
        hipLaunchKernelGGL(quantize_fp8_kernel<float>, dim3((unsigned)grid),
                           dim3(256), 0, s, (const float*)x, (u8*)y, n16,
                           inv_scale);
    else
        hipLaunchKernelGGL(quantize_fp8_kernel<bf16>, dim3((unsigned)grid),
                           dim3(256), 0, s, (const bf16*)x, (u8*)y, n16,
                           inv_scale);
}

}  // namespace defer_hip
