// Convolution kernels for gfx950 (CDNA4), NHWC bf16, MFMA 16x16x32
// with fp32 accumulation. Three kernel families, selected by a measured
// per-shape policy in plan_conv, conv_plan.h (docs/OPTIMIZATION_LOG.md has
// the A/B numbers behind every choice):
//
//   conv_igemm_kernel — implicit GEMM, the general path (1x1s, deep-K
//     3x3s, strided convs, the dense head, the 7x7 stem's run-packed
//     gather);
//   conv_win_kernel   — window-reuse 3x3/s1: an 8x16 output tile stages
//     its input window to LDS once per 64-channel block and slides the
//     nine (r,s) offsets in LDS (9x less A staging);
//   conv_swin_kernel  — the small-Cin (<8, padded to 8) window variant
//     for VGG-style 3x3 stems.
//
// GEMM view: C[M, N] = A[M, K] x B[K, N]
//   M = NB*OH*OW (output pixels), N = Cout, K = R*S*Cin,
//   A row m = input patch of pixel m (gathered on the fly),
//   B = weights, stored OHWI [Cout][R][S][Cin] so B^T rows are contiguous.
//
// Structure (cdna_hip_programming.md §5, T3+T4 counted-vmcnt pipeline):
// template-parameterized BM x BN output tile, BK=64, TPB/64 waves,
// DA-deep LDS rings staged by global_load_lds width 16 (lane-linear
// dest; XOR swizzle applied to the *source* chunk index and the read
// address — rule 21). The stage cursor runs DA-1 K-tiles ahead; each
// iteration waits a COUNTED s_waitcnt vmcnt — never 0 mid-loop —
// and a raw s_barrier, so glds stay in flight across barriers and
// load latency hides under MFMA. Each block walks multiple m-tiles
// (grid-stride) so the pipeline never drains between tiles; when the
// whole K fits one tile, the weight tile is staged once (B_PERSIST).
//
// Address math is kept off the k-loop critical path:
//   - the m -> (batch, oh, ow) decomposition runs once per STAGED m-tile
//     (magic-multiply division, no v_rcp chains), cached per chunk;
//   - AMODE_CONV derives (c, r, s) from k with two umulhi magics;
//   - AMODE_RSC (Cin % 64 == 0, i.e. every non-stem conv) walks K in
//     (cin64-block, r, s)-major order so one k-tile is a single scalar
//     (r, s, cb) triple — the per-lane work is two adds and a bounds
//     check. The B gather applies the same permutation to the OHWI
//     weights in-flight, so A and B agree on the K order and no host
//     repack is needed.
// The fused epilogue runs OUTSIDE the k-loop (between tiles) so the hot
// loop carries no exec-masked epilogue code.
//
// Epilogue fuses folded-BN scale/bias, residual add and ReLU (the Keras
// Conv2D+BN+Add+ReLU stack the reference runs via model.predict,
// /root/reference/src/node.py:106), bounced through the just-freed LDS
// A-buffer so residual loads and bf16 stores are 8-B coalesced.
//
// GEMM mode (R=S=1, H=W=1, Cin=K): out[M,N] = x[M,K] @ w[N,K]^T — used
// for 1x1/s1 convs, the dense classifier head, and any explicit GEMM.
#include <cstdlib>

#include "common.h"
#include "kernels.h"
#include "conv_plan.h"

using defer_hip::ConvParams;

#define BK 64
#define NTHREADS 256
#define KCH (BK / 8)          // 16-B chunks per tile row (8)

// XOR swizzle: logical (row, k8) lives at physical k8p = k8 ^ (row & 7).
__device__ __forceinline__ int swz(int row, int k8) {
    return k8 ^ (row & 7);
}

// floor(n / d) for n*d < 2^32, via mul = ceil(2^32 / d) (d > 1).
__device__ __forceinline__ u32 umagic(u32 n, u32 mul, u32 d) {
    return d == 1 ? n : __umulhi(n, mul);
}

__device__ __forceinline__ void glds16(const bf16* src, bf16* lds_base) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)lds_base,
        16, 0, 0);
}

// DA: pipeline depth of the A/B LDS rings (DB must equal DA unless
// B_PERSIST, where the single B tile is staged once and DB is unused —
// an asymmetric deep-A/shallow-B variant was implemented and measured
// 6-22% slower: boundary activations are L3/L2-resident, so extra LDS
// per block costs more occupancy than deeper latency cover buys).
// WPS: minimum waves per SIMD (__launch_bounds__ 2nd arg) = blocks/CU of
// this 256-thread kernel. The MFMA-bound tile configs run 2 blocks/CU;
// the pure-bandwidth small-tile GEMM configs (1x1 convs, K<=512) trade
// registers for 3-4 co-resident blocks so more independent load streams
// and epilogues overlap.
template <int ACT, bool HAS_RES, int AMODE, bool B_PERSIST, int BM,
          int BN, int DA, int DB, int WPS = 2, int TPB = NTHREADS>
__global__ __launch_bounds__(TPB, WPS) void conv_igemm_kernel(
    ConvParams p) {
    const bf16* __restrict__ X = (const bf16*)p.x;
    const bf16* __restrict__ Wt = (const bf16*)p.w;
    const bf16* __restrict__ Z = (const bf16*)p.zbuf;
    const bf16* __restrict__ RES = (const bf16*)p.res;
    bf16* __restrict__ OUT = (bf16*)p.out;

    // wave tiling: WMW waves along m (32 rows each), WNW along n
    constexpr int NW = TPB / WAVE;              // waves per block
    constexpr int WMW = BM / 32;                // m-slabs of 32 rows
    constexpr int WNW = NW / WMW;               // waves along n
    constexpr int WN = BN / WNW;                // wave n-width
    constexpr int NI = WN / 16;                 // B frags per wave
    constexpr int ACH = BM * 8 / TPB;           // A chunks per thread
    constexpr int BCH = BN * 8 / TPB;           // B chunks per thread
    constexpr int OPS = ACH + (B_PERSIST ? 0 : BCH);
    // DB is only meaningful for B_PERSIST configs (unused ring slot);
    // both rings run at depth DA — an asymmetric deep-A/shallow-B
    // variant was measured 6-22% slower (L3-resident activations) and
    // removed (git history has the measurements).

    __shared__ __attribute__((aligned(16)))
    bf16 lds[(DA * BM + (B_PERSIST ? 1 : DA) * BN) * BK];
    bf16* A0 = lds;
    bf16* B0 = lds + DA * BM * BK;

    const int tid = threadIdx.x;
    const int wave = tid / WAVE;
    const int lane = tid % WAVE;
    const int wm = wave / WNW;                  // wave m index
    const int wn = wave % WNW;                  // wave n index
    const int n0 = blockIdx.y * BN;
    const int mtiles = (p.M + BM - 1) / BM;
    const int nk = (p.K + BK - 1) / BK;

    // ---- per-thread chunk geometry (constant across tiles)
    int a_row[ACH], a_k8[ACH];
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
        int chunk = wave * (ACH * 64) + i * 64 + lane;
        a_row[i] = chunk / KCH;
        a_k8[i] = swz(a_row[i], chunk % KCH);
    }
    int b_row[BCH], b_k8[BCH];
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
        int chunk = wave * (BCH * 64) + i * 64 + lane;
        b_row[i] = chunk / KCH;
        b_k8[i] = swz(b_row[i], chunk % KCH);
    }

    const int lo16 = lane & 15;
    const int hi4 = lane >> 4;
    // folded-BN scale/bias for this wave's n-columns, loaded once
    // (p.scale/p.bias always non-null; nullable per-element loads in the
    // epilogue made hipcc emit one vmcnt(0) per element).
    const float* __restrict__ SCALE = p.scale;
    const float* __restrict__ BIAS = p.bias;
    float sc[NI], bi[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        int n = n0 + wn * WN + ni * 16 + lo16;
        if (n >= p.Cout) n = p.Cout - 1;
        sc[ni] = SCALE[n];
        bi[ni] = BIAS[n];
    }

    // ---- per-chunk A state for the STAGED m-tile (refreshed when the
    // stage cursor crosses into a new m-tile — once per nk k-tiles).
    // RSC keeps an INCREMENTAL per-chunk pointer (advanced by a scalar
    // delta per k-tile) plus a (r,s)-validity bitmask precomputed here,
    // so the hot stage carries no multiplies and no coordinate math —
    // the k-loop was VALU-issue-bound with per-tile address rebuilds.
    long a_base[ACH];
    int a_ihb[ACH], a_iwb[ACH];
    bool a_mval[ACH];
    const bf16* a_ptr[ACH];      // RSC: current (cb, r, s) source address
    u32 a_vmask[ACH];            // RSC: bit (r*S+s) = window in-bounds
    const int d_s = p.Cin;                                // s+1
    const int d_r = (p.W - (p.S - 1)) * p.Cin;            // r+1, s=0
    const int d_cb = 64 - ((p.R - 1) * p.W + (p.S - 1)) * p.Cin;
    auto a_setup = [&](int mt) {
        const int m0 = mt * BM;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            int m = m0 + a_row[i];
            a_mval[i] = m < p.M;
            if (m >= p.M) m = p.M - 1;
            if (AMODE == AMODE_GEMM) {
                a_base[i] = (long)m * p.K + a_k8[i] * 8;
            } else if (AMODE == AMODE_RSC) {
                u32 t = umagic(m, p.owmul, p.OW);       // m / OW
                int ow = m - (int)t * p.OW;
                u32 nb = umagic(t, p.ohmul, p.OH);      // t / OH
                int oh = (int)t - (int)nb * p.OH;
                const int ihb = oh * p.stride - p.pad;
                const int iwb = ow * p.stride - p.pad;
                a_ptr[i] = X + (long)nb * p.H * p.W * p.Cin
                             + ((long)ihb * p.W + iwb) * p.Cin
                             + a_k8[i] * 8;
                u32 mask = 0;
                if (a_mval[i])
                    for (int r = 0; r < p.R; ++r)
                        for (int sI = 0; sI < p.S; ++sI)
                            if ((u32)(ihb + r) < (u32)p.H &&
                                (u32)(iwb + sI) < (u32)p.W)
                                mask |= 1u << (r * p.S + sI);
                a_vmask[i] = mask;
            } else if (AMODE == AMODE_STEM) {
                // spatially pre-padded input (pad absorbed into coords);
                // p.H/p.W are the PADDED dims, base points at the
                // window's first row run
                u32 t = umagic(m, p.owmul, p.OW);       // m / OW
                int ow = m - (int)t * p.OW;
                u32 nb = umagic(t, p.ohmul, p.OH);      // t / OH
                int oh = (int)t - (int)nb * p.OH;
                a_base[i] = ((long)nb * p.H + oh * p.stride) * p.W * p.Cin
                            + (long)(ow * p.stride) * p.Cin;
            } else {
                u32 t = umagic(m, p.owmul, p.OW);       // m / OW
                int ow = m - (int)t * p.OW;
                u32 nb = umagic(t, p.ohmul, p.OH);      // t / OH
                int oh = (int)t - (int)nb * p.OH;
                a_ihb[i] = oh * p.stride - p.pad;
                a_iwb[i] = ow * p.stride - p.pad;
                a_base[i] = (long)nb * p.H * p.W * p.Cin;
            }
        }
    };

    // stage cursor scalars (RSC walks (cb, r, s) incrementally — the
    // k-tile order IS (cb*R*S + r*S + s), no division anywhere; s_t
    // mirrors r*S+s for the validity-mask bit index)
    int s_mt = blockIdx.x, s_kt = 0;
    int s_cb = 0, s_r = 0, s_s = 0, s_t = 0;
    const bool kal = (p.K & 63) == 0;   // k < K by construction

    auto stage_a = [&](int buf) {
        bf16* A = A0 + buf * BM * BK;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const bf16* src = Z;
            if (AMODE == AMODE_GEMM) {
                if (kal) {
                    // K%64==0 (every 1x1/dense in practice): clamped
                    // rows read valid memory, no per-lane checks
                    src = X + a_base[i] + (long)s_kt * BK;
                } else {
                    int k = s_kt * BK + a_k8[i] * 8;
                    if (a_mval[i] && k < p.K)
                        src = X + a_base[i] + (long)s_kt * BK;
                }
            } else if (AMODE == AMODE_CONV) {
                int k = s_kt * BK + a_k8[i] * 8;
                u32 rs = umagic(k, p.cmul, p.Cin);      // k / Cin
                int c = k - (int)rs * p.Cin;
                u32 r = umagic(rs, p.smul, p.S);        // rs / S
                int sI = (int)rs - (int)r * p.S;
                int ih = a_ihb[i] + (int)r;
                int iw = a_iwb[i] + sI;
                if (a_mval[i] && k < p.K && (u32)ih < (u32)p.H &&
                    (u32)iw < (u32)p.W)
                    src = X + a_base[i] + ((long)ih * p.W + iw) * p.Cin
                              + c;
            } else if (AMODE == AMODE_STEM) {
                // K walks (r, run) with run = TR bytes of one padded
                // input row (p.S carries TR; all coords in-bounds by
                // construction, so no validity math at all)
                int k = s_kt * BK + a_k8[i] * 8;
                u32 r = umagic(k, p.smul, p.S);         // k / TR
                int t = k - (int)r * p.S;
                if (a_mval[i])
                    src = X + a_base[i]
                              + (long)r * p.W * p.Cin + t;
            } else {  // AMODE_RSC: incremental pointer + mask-bit select
                src = a_ptr[i];
                if (!((a_vmask[i] >> s_t) & 1u)) src = Z;
            }
            glds16(src, A + (wave * (ACH * 64) + i * 64) * 8);
        }
    };
    // B lane offsets are constant across k-tiles: per-tile addressing is
    // a SCALAR base (Wt + koff) + 32-bit lane offset, which lowers to
    // the saddr global_load_lds form — no per-lane 64-bit math in the
    // loop. Rows past Cout duplicate the last row (their columns are
    // never stored; the epilogue clamps), so no zero-page redirect.
    u32 b_voff[BCH];
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
        int n = n0 + b_row[i];
        if (n >= p.Cout) n = p.Cout - 1;
        b_voff[i] = (u32)((u64)n * (u64)p.K) + (u32)(b_k8[i] * 8);
    }
    auto stage_b = [&](int buf, int kt, int cb, int r, int sI) {
        bf16* B = B0 + buf * BN * BK;
        // RSC: same K permutation as A, applied to the OHWI weights
        const long koff = (AMODE == AMODE_RSC)
                              ? (long)(r * p.S + sI) * p.Cin + cb * 64
                              : (long)kt * BK;
        if (AMODE == AMODE_RSC || kal) {
            const bf16* bbase = Wt + koff;
#pragma unroll
            for (int i = 0; i < BCH; ++i)
                glds16(bbase + b_voff[i],
                       B + (wave * (BCH * 64) + i * 64) * 8);
        } else {
#pragma unroll
            for (int i = 0; i < BCH; ++i) {
                int n = n0 + b_row[i];
                long k = koff + b_k8[i] * 8;
                const bf16* src = (n < p.Cout && k < p.K)
                                      ? Wt + (long)n * p.K + k
                                      : Z;
                glds16(src, B + (wave * (BCH * 64) + i * 64) * 8);
            }
        }
    };

    f32x4 acc[2][NI];
    auto compute = [&](int abuf, int bbuf) {
        bf16* A = A0 + abuf * BM * BK;
        bf16* B = B0 + bbuf * BN * BK;
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks) {
            bf16x8 af[2], bfr[NI];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                int row = wm * 32 + mi * 16 + lo16;
                af[mi] = *reinterpret_cast<bf16x8*>(
                    A + row * BK + swz(row, ks * 4 + hi4) * 8);
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                int row = wn * WN + ni * 16 + lo16;
                bfr[ni] = *reinterpret_cast<bf16x8*>(
                    B + row * BK + swz(row, ks * 4 + hi4) * 8);
            }
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                    acc[mi][ni] =
                        MFMA_BF16_16x16x32(af[mi], bfr[ni], acc[mi][ni]);
        }
    };

    // ---- epilogue: LDS transpose bounce through the A buffer just
    // consumed; RH output rows per round (RH*BN f32 = one A buffer).
    constexpr int RH = (BM * BK * 2 / 4) / BN;   // 64/32/16 rows per round
    constexpr int ROUNDS = BM / RH;
    constexpr int CPR = RH * BN / 4 / TPB;       // 16-B chunks per thread
    auto epilogue = [&](int mt, int abuf) {
        float* scratch = (float*)(A0 + abuf * BM * BK);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();       // all waves done with A[abuf]
#pragma unroll
        for (int h = 0; h < ROUNDS; ++h) {
            const int r0 = h * RH;           // tile-local first row
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        int r = wm * 32 + mi * 16 + hi4 * 4 + e;
                        if (r < r0 || r >= r0 + RH) continue;
                        int c = wn * WN + ni * 16 + lo16;
                        int rl = r - r0;
                        int cs = c ^ (((rl >> 2) & 3) << 4);
                        scratch[rl * BN + cs] =
                            acc[mi][ni][e] * sc[ni] + bi[ni];
                    }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const bool interior =
                (mt * BM + BM <= p.M) && (n0 + BN <= p.Cout) &&
                (p.Cout % 8 == 0);     // 16-B aligned rows
            if (interior) {
                // 8-col chunks: 16-B residual loads and 16-B bf16 stores
                // (8-B stores made the 1x1 layers store-issue-bound, cf.
                // MI355X_MICROARCH store-tail note)
                constexpr int CP8 = RH * BN / 8 / TPB;
                f32x4 v4[CP8][2];
                bf16x8 rv[CP8];
                long off[CP8];
#pragma unroll
                for (int i = 0; i < CP8; ++i) {
                    int chunk = tid + i * TPB;
                    int rl = chunk / (BN / 8);
                    int c8 = (chunk % (BN / 8)) * 8;
                    int cs = c8 ^ (((rl >> 2) & 3) << 4);
                    off[i] = (long)(mt * BM + r0 + rl) * p.Cout + n0 + c8;
                    v4[i][0] = *reinterpret_cast<f32x4*>(
                        scratch + rl * BN + cs);
                    v4[i][1] = *reinterpret_cast<f32x4*>(
                        scratch + rl * BN + cs + 4);
                    if (HAS_RES)
                        rv[i] = *reinterpret_cast<const bf16x8*>(
                            RES + off[i]);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < CP8; ++i) {
                    bf16x8 o;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float v = v4[i][j / 4][j % 4];
                        if (HAS_RES) v += bf2f(rv[i][j]);
                        o[j] = f2bf(apply_act_hi(v, ACT, p.act_hi));
                    }
                    *reinterpret_cast<bf16x8*>(OUT + off[i]) = o;
                }
            } else {
#pragma unroll
                for (int i = 0; i < CPR; ++i) {
                    int chunk = tid + i * TPB;
                    int rl = chunk / (BN / 4);
                    int c4 = (chunk % (BN / 4)) * 4;
                    int cs = c4 ^ (((rl >> 2) & 3) << 4);
                    int m = mt * BM + r0 + rl;
                    int n = n0 + c4;
                    if (m >= p.M || n >= p.Cout) continue;
                    f32x4 v4 = *reinterpret_cast<f32x4*>(
                        scratch + rl * BN + cs);
                    long off = (long)m * p.Cout + n;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (n + j >= p.Cout) continue;
                        float v = v4[j];
                        if (HAS_RES) v += bf2f(RES[off + j]);
                        OUT[off + j] = f2bf(apply_act_hi(v, ACT, p.act_hi));
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();   // next round reuses scratch
        }
    };

    // ---- flattened (m-tile, k-tile) pipeline. The stage cursor runs
    // DA-1 tiles ahead of compute. Counted vmcnt: tile it's stages must
    // have landed by wait(it); newer stages stay in flight (the latency
    // cover — up to DA-1 compute phases).
    auto advance = [&]() {
        if (++s_kt == nk) {
            s_kt = 0;
            s_mt += gridDim.x;
            s_cb = 0; s_r = 0; s_s = 0; s_t = 0;
            if (s_mt < mtiles) a_setup(s_mt);
        } else if (AMODE == AMODE_RSC) {
            int d;
            if (++s_s == p.S) {
                s_s = 0;
                if (++s_r == p.R) {
                    s_r = 0; ++s_cb; s_t = 0; d = d_cb;
                } else {
                    ++s_t; d = d_r;
                }
            } else {
                ++s_t; d = d_s;
            }
#pragma unroll
            for (int i = 0; i < ACH; ++i) a_ptr[i] += d;
        }
    };
    if (s_mt < mtiles) a_setup(s_mt);
    if (B_PERSIST) stage_b(0, 0, 0, 0, 0);  // oldest ops: first wait drains
    int staged = 0;
#pragma unroll
    for (int d = 0; d < DA - 1; ++d) {
        if (s_mt < mtiles) {
            stage_a(d);
            if (!B_PERSIST) stage_b(d, s_kt, s_cb, s_r, s_s);
            advance();
            ++staged;
        }
    }

    // float allowance: up to DA-2 whole stages may stay in flight
    constexpr int NFLOAT = (DA - 2) * OPS;

    int it = 0;   // computed-iteration counter; tile i -> buffer i%DA
    for (int mt = blockIdx.x; mt < mtiles; mt += gridDim.x) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
                acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};
        for (int kt = 0; kt < nk; ++kt, ++it) {
            const int avail = staged - it - 1;
            if (DA >= 4 && avail >= 2)
                asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NFLOAT)
                             : "memory");
            else if (avail >= 1)
                asm volatile("s_waitcnt vmcnt(%0)" ::"i"(OPS)
                             : "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            // stage BEFORE compute: the refilled buffers were last read
            // by compute(it-1), which every wave finished before this
            // barrier — issuing the glds here buys one extra compute
            // phase of latency cover
            if (s_mt < mtiles) {
                stage_a((it + DA - 1) % DA);
                if (!B_PERSIST)
                    stage_b((it + DA - 1) % DA, s_kt, s_cb, s_r, s_s);
                advance();
                ++staged;
            }
            compute(it % DA, B_PERSIST ? 0 : it % DA);
        }
        // epilogue AFTER the next tiles' stages were issued: their glds
        // land in buffers disjoint from the scratch buffer (it-1)%DA
        epilogue(mt, (it - 1) % DA);
    }
}

// ---------------------------------------------------------------------------
// Window-reuse 3x3/s1/p1 convolution (AMODE_WIN as its own kernel).
//
// The implicit-GEMM kernel re-stages the SAME input bytes once per (r,s)
// k-tile — 9x for a 3x3 — and its BM128/BN128 configs demand ~117
// B/cyc/CU of L2 tile traffic vs ~56 available. Here a 2D output tile
// (TH=8 x TW=16 pixels = BM 128) stages its (TH+2)x(TW+2)x64ch input
// WINDOW to LDS once per 64-channel block and the nine (r,s) compute
// phases slide inside LDS: A-staging drops 9x -> ~1.1x (halo).
//
// LDS window layout [ihl][c8][iwl] in 16-B chunks, so an MFMA A-read's
// 16 lanes (cw = lane&15 consecutive) hit consecutive chunks —
// conflict-free ds_read_b128 — and the (r, s) slide is one scalar chunk
// offset (r*8*WW + s). The next window (cb+1, crossing m-tiles) is
// staged in 6 glds slices interleaved with phases 0..5, so the counted
// vmcnt keeps 3+ phases of load-latency cover without a FIFO conflict
// with the per-phase B stages (order: B first, then the slice).
#define WTW 16                         // window tile width (fixed)

template <int ACT, bool HAS_RES, int BN, int TH = 8, int TPB = NTHREADS,
          int WPS = 2>
__global__ __launch_bounds__(TPB, WPS) void conv_win_kernel(
    ConvParams p) {
    constexpr int TW = WTW;
    constexpr int BM = TH * TW;                 // 128 (TH8) / 64 (TH4)
    constexpr int WH = TH + 2, WW = TW + 2;     // window dims
    constexpr int WCH = WH * 8 * WW;            // 16-B chunks per window
    constexpr int NW = TPB / WAVE;              // waves per block
    constexpr int NSL = (WCH + NW * 64 - 1) / (NW * 64);  // slices/wave
    constexpr int DB = 2;
    constexpr int WMW = BM / 32;                // waves along m
    constexpr int WNW = NW / WMW;               // waves along n
    constexpr int WN = BN / WNW;
    constexpr int NI = WN / 16;
    constexpr int BCH = BN * 8 / TPB;
    const bf16* __restrict__ X = (const bf16*)p.x;
    const bf16* __restrict__ Wt = (const bf16*)p.w;
    const bf16* __restrict__ Z = (const bf16*)p.zbuf;
    const bf16* __restrict__ RES = (const bf16*)p.res;
    bf16* __restrict__ OUT = (bf16*)p.out;

    __shared__ __attribute__((aligned(16)))
    bf16 lds[(2 * WCH * 8) + DB * BN * BK];
    bf16* W0 = lds;                              // two window buffers
    bf16* B0 = lds + 2 * WCH * 8;

    const int tid = threadIdx.x;
    const int wave = tid / WAVE;
    const int lane = tid % WAVE;
    const int wm = wave / WNW;
    const int wn = wave % WNW;
    const int n0 = blockIdx.y * BN;
    const int lo16 = lane & 15;
    const int hi4 = lane >> 4;
    const int ncb = p.Cin / 64;
    const int ntw = (p.OW + TW - 1) / TW;
    const int nth = (p.OH + TH - 1) / TH;
    const int mtiles = p.NB * nth * ntw;
    const long nwin = (long)mtiles * ncb;

    // B lane offsets (scalar-base + 32-bit lane offset form)
    int b_row[BCH], b_k8[BCH];
    u32 b_voff[BCH];
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
        int chunk = wave * (BCH * 64) + i * 64 + lane;
        b_row[i] = chunk / KCH;
        b_k8[i] = swz(b_row[i], chunk % KCH);
        int n = n0 + b_row[i];
        if (n >= p.Cout) n = p.Cout - 1;
        b_voff[i] = (u32)((u64)n * (u64)p.K) + (u32)(b_k8[i] * 8);
    }
    auto stage_b = [&](int buf, int cb, int rs) {
        bf16* B = B0 + buf * BN * BK;
        const bf16* bbase = Wt + (long)rs * p.Cin + cb * 64;
#pragma unroll
        for (int i = 0; i < BCH; ++i)
            glds16(bbase + b_voff[i],
                   B + (wave * (BCH * 64) + i * 64) * 8);
    };


    // ---- window cursor: stages window (s_mt, s_cb). Per-window setup
    // keeps one SCALAR base (image + channel block) plus per-lane
    // 32-bit offsets and a 6-bit validity mask — the per-slice address
    // is rebuilt in stage_win_slice (register pressure: the first cut
    // of this kernel kept 6 pointers per lane and spilled).
    int s_mt = blockIdx.x, s_cb = 0;
    int w_loff[NSL];                  // per-lane element offsets
    u32 w_okm = 0;                    // bit j = slice j in bounds
    const bf16* w_base = X;           // + nb*H*W*Cin + cb*64 (uniform)
    int dst_buf = 0;                  // LDS buffer this window lands in
    long w_count = 0;                 // windows staged so far (parity)
    int c_nb = 0, c_oh0 = 0, c_ow0 = 0;   // compute-tile coords
    auto win_setup = [&]() {          // for (s_mt, s_cb)
        int mt = s_mt;
        int tw = mt % ntw;
        int t = mt / ntw;
        int th = t % nth;
        int nb = t / nth;
        int oh0 = th * TH, ow0 = tw * TW;
        w_base = X + (long)nb * p.H * p.W * p.Cin + s_cb * 64;
        w_okm = 0;
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
            // slot j covers chunk (j*NW + wave)*64 + lane
            int chunk = (j * NW + wave) * 64 + lane;
            bool in = chunk < WCH;
            if (!in) chunk = WCH - 1;
            int iwl = chunk % WW;
            int q = chunk / WW;
            int c8 = q % 8;
            int ihl = q / 8;
            int ih = oh0 - 1 + ihl;
            int iw = ow0 - 1 + iwl;
            if (in && (u32)ih < (u32)p.H && (u32)iw < (u32)p.W)
                w_okm |= 1u << j;
            w_loff[j] = (ih * p.W + iw) * p.Cin + c8 * 8;
        }
    };
    auto stage_win_slice = [&](int j) {
        // lanes past the last chunk must not WRITE (the clamped source
        // is harmless but an unguarded glds would land 16B past the
        // buffer — into the partner window / B ring)
        int chunk = (j * NW + wave) * 64 + lane;
        if (chunk < WCH) {
            const bf16* src =
                (w_okm >> j) & 1 ? w_base + w_loff[j] : Z;
            glds16(src, W0 + (long)dst_buf * WCH * 8 + chunk * 8);
        }
    };
    auto win_advance = [&]() {
        ++w_count;
        dst_buf ^= 1;
        if (++s_cb == ncb) {
            s_cb = 0;
            s_mt += gridDim.x;
        }
        if (w_count < nwin && s_mt < mtiles) win_setup();
    };

    f32x4 acc[2][NI];
    auto compute = [&](int wbuf, int rs, int bbuf) {
        const int r = rs / 3, s = rs % 3;
        bf16* WB = W0 + (long)wbuf * WCH * 8;
        bf16* B = B0 + bbuf * BN * BK;
        const int poff = r * (8 * WW) + s;       // (r,s) chunk offset
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks) {
            bf16x8 af[2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                int pp = wm * 32 + mi * 16 + lo16;       // tile pixel
                int base = (pp >> 4) * (8 * WW)           // r' rows
                           + (ks * 4 + hi4) * WW          // c8
                           + (pp & 15);                   // cw
                af[mi] = *reinterpret_cast<bf16x8*>(
                    WB + (base + poff) * 8);
            }
            // B frags in halves of <=4: caps live B registers at 16
            // (the BN128 instantiation spilled with all 8 live)
#pragma unroll
            for (int hf = 0; hf < (NI + 3) / 4; ++hf) {
                constexpr int HNI = NI < 4 ? NI : 4;
                bf16x8 bfr[HNI];
#pragma unroll
                for (int q = 0; q < HNI; ++q) {
                    int row = wn * WN + (hf * 4 + q) * 16 + lo16;
                    bfr[q] = *reinterpret_cast<bf16x8*>(
                        B + row * BK + swz(row, ks * 4 + hi4) * 8);
                }
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int q = 0; q < HNI; ++q)
                        acc[mi][hf * 4 + q] = MFMA_BF16_16x16x32(
                            af[mi], bfr[q], acc[mi][hf * 4 + q]);
            }
        }
    };

    // ---- epilogue: bounce through the finished window buffer.
    // RH rows per round, sized so RH*BN f32 fits the WCH*4-f32 buffer
    // and at least one 16-B chunk per thread per round.
    constexpr int RH0 = (WCH * 4 / BN) >= BM
                            ? BM
                            : ((WCH * 4 / BN) >= BM / 2 ? BM / 2
                                                        : BM / 4);
    constexpr int RH = (RH0 * BN >= TPB * 8) ? RH0 : BM;
    constexpr int ROUNDS = BM / RH;
    auto epilogue = [&](int nb, int oh0, int ow0, int wbuf) {
        float* scratch = (float*)(W0 + (long)wbuf * WCH * 8);
        // scale/bias loaded here, once per m-tile, not held across the
        // k-loop (register budget)
        float sc[NI], bi[NI];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            int n = n0 + wn * WN + ni * 16 + lo16;
            if (n >= p.Cout) n = p.Cout - 1;
            sc[ni] = p.scale[n];
            bi[ni] = p.bias[n];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const bool interior =
            (oh0 + TH <= p.OH) && (ow0 + TW <= p.OW) &&
            (n0 + BN <= p.Cout) && (p.Cout % 8 == 0);
#pragma unroll
        for (int h = 0; h < ROUNDS; ++h) {
            const int r0 = h * RH;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        int r = wm * 32 + mi * 16 + hi4 * 4 + e;
                        if (r < r0 || r >= r0 + RH) continue;
                        int c = wn * WN + ni * 16 + lo16;
                        int rl = r - r0;
                        int cs = c ^ (((rl >> 2) & 3) << 4);
                        scratch[rl * BN + cs] =
                            acc[mi][ni][e] * sc[ni] + bi[ni];
                    }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (interior) {
                constexpr int CP8 = RH * BN / 8 / TPB;
                f32x4 v4[CP8][2];
                bf16x8 rv[CP8];
                long off[CP8];
#pragma unroll
                for (int i = 0; i < CP8; ++i) {
                    int chunk = tid + i * TPB;
                    int rl = chunk / (BN / 8);
                    int c8 = (chunk % (BN / 8)) * 8;
                    int cs = c8 ^ (((rl >> 2) & 3) << 4);
                    int pp = r0 + rl;
                    long oh = oh0 + (pp >> 4), ow = ow0 + (pp & 15);
                    off[i] = (((long)nb * p.OH + oh) * p.OW + ow)
                                 * p.Cout + n0 + c8;
                    v4[i][0] = *reinterpret_cast<f32x4*>(
                        scratch + rl * BN + cs);
                    v4[i][1] = *reinterpret_cast<f32x4*>(
                        scratch + rl * BN + cs + 4);
                    if (HAS_RES)
                        rv[i] = *reinterpret_cast<const bf16x8*>(
                            RES + off[i]);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < CP8; ++i) {
                    bf16x8 o;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float v = v4[i][j / 4][j % 4];
                        if (HAS_RES) v += bf2f(rv[i][j]);
                        o[j] = f2bf(apply_act_hi(v, ACT, p.act_hi));
                    }
                    *reinterpret_cast<bf16x8*>(OUT + off[i]) = o;
                }
            } else {
                constexpr int CPR = RH * BN / 4 / TPB;
#pragma unroll
                for (int i = 0; i < CPR; ++i) {
                    int chunk = tid + i * TPB;
                    int rl = chunk / (BN / 4);
                    int c4 = (chunk % (BN / 4)) * 4;
                    int cs = c4 ^ (((rl >> 2) & 3) << 4);
                    int pp = r0 + rl;
                    int oh = oh0 + (pp >> 4), ow = ow0 + (pp & 15);
                    int n = n0 + c4;
                    if (oh >= p.OH || ow >= p.OW || n >= p.Cout)
                        continue;
                    f32x4 v4 = *reinterpret_cast<f32x4*>(
                        scratch + rl * BN + cs);
                    long off = (((long)nb * p.OH + oh) * p.OW + ow)
                                   * p.Cout + n;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (n + j >= p.Cout) continue;
                        float v = v4[j];
                        if (HAS_RES) v += bf2f(RES[off + j]);
                        OUT[off + j] = f2bf(apply_act_hi(v, ACT, p.act_hi));
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
    };

    // ---- main loop. Window w = (mt, cb) of THIS block's walk; 9 phases
    // each. Per phase j: wait -> barrier -> stage B(next tile) -> stage
    // one window slice (j<6, for window w+1) -> compute. vmcnt float:
    // the slice issued after B(cur) in the previous phase (1 glds/wave).
    const long local_wins =
        (blockIdx.x < mtiles)
            ? (long)((mtiles - 1 - blockIdx.x) / gridDim.x + 1) * ncb
            : 0;
    if (local_wins > 0) {
        win_setup();                  // window 0
#pragma unroll
        for (int j = 0; j < NSL; ++j) stage_win_slice(j);
        stage_b(0, 0, 0);             // B tile 0 = (cb 0, rs 0)
        win_advance();                // cursor -> window 1
    }
    long b_staged = 1;                // B tiles issued
    int b_cb = 0, b_rs = 1;           // next B tile's (cb, rs)
    long ph = 0;                      // linear phase = B-tile index
    long w = 0;                       // computed-window counter
    bool sliced_prev = false;

    for (int mt = blockIdx.x; mt < mtiles; mt += gridDim.x) {
        int tw = mt % ntw;
        int t = mt / ntw;
        c_oh0 = (t % nth) * TH;
        c_nb = t / nth;
        c_ow0 = tw * TW;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
                acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};
        for (int cb = 0; cb < ncb; ++cb, ++w) {
            const int cbuf = (int)(w & 1);
            for (int j = 0; j < 9; ++j, ++ph) {
                if (sliced_prev && !p.smul)   // p.smul: full-sync debug
                    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(1)
                                 : "memory");
                else
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (b_staged < local_wins * 9) {
                    stage_b((int)((ph + 1) & 1), b_cb, b_rs);
                    ++b_staged;
                    if (++b_rs == 9) {
                        b_rs = 0;
                        if (++b_cb == ncb) b_cb = 0;
                    }
                }
                // per-WAVE: a wave whose slice slot is entirely past
                // WCH issues no glds and must not float one
                bool sl = (j < NSL) && (w_count < local_wins) &&
                          (s_mt < mtiles) &&
                          ((j * NW + wave) * 64 < WCH);
                if (sl) stage_win_slice(j);
                sliced_prev = sl;
                compute(cbuf, j, (int)(ph & 1));
            }
            if (w + 1 < local_wins) win_advance();
        }
        epilogue(c_nb, c_oh0, c_ow0, (int)((w - 1) & 1));
    }
}
__global__ void pad_channels_kernel(const bf16* __restrict__ x,
                                    bf16* __restrict__ y, long rows, int C,
                                    int C8) {
    long total = rows * (C8 / 8);
    long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long gs = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total; i += gs) {
        int cb = (int)(i % (C8 / 8));
        long row = i / (C8 / 8);
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int c = cb * 8 + j;
            v[j] = (c < C) ? x[row * C + c] : (bf16)0.f;
        }
        store_bf16x8(y + row * C8 + cb * 8, v);
    }
}

// ---------------------------------------------------------------------------
// Spatial zero-pad NHWC: [NB,H,W,C] -> [NB,PH,PW,C], interior at
// (ph0, pw0). Feeds the STEM gather (pad absorbed into coordinates so the
// k-loop runs with zero validity math).
__global__ void pad2d_kernel(const bf16* __restrict__ x,
                             bf16* __restrict__ y, int NB, int H, int W,
                             int C, int PH, int PW, int ph0, int pw0) {
    const int rowlen = PW * C;
    for (int row = blockIdx.x; row < NB * PH; row += gridDim.x) {
        int ph = row % PH, nb = row / PH;
        int ih = ph - ph0;
        bf16* dst = y + (long)row * rowlen;
        if ((unsigned)ih >= (unsigned)H) {
            for (int j = threadIdx.x; j < rowlen; j += blockDim.x)
                dst[j] = (bf16)0.f;
        } else {
            const bf16* src = x + ((long)nb * H + ih) * W * C;
            const int i0 = pw0 * C, i1 = i0 + W * C;
            for (int j = threadIdx.x; j < rowlen; j += blockDim.x)
                dst[j] = (j >= i0 && j < i1) ? src[j - i0] : (bf16)0.f;
        }
    }
}

// Repack OHWI weights for the STEM K-order: wp[n][r*TR + s*C + c] =
// w[n][r][s][c], zero in the run padding (t >= S*C).
__global__ void stem_repack_w_kernel(const bf16* __restrict__ w,
                                     bf16* __restrict__ wp, int Cout,
                                     int R, int S, int C, int TR) {
    long total = (long)Cout * R * TR;
    long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long gs = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total; i += gs) {
        int t = (int)(i % TR);
        long u = i / TR;
        int r = (int)(u % R);
        int n = (int)(u / R);
        bf16 v = (bf16)0.f;
        if (t < S * C) v = w[((long)(n * R + r) * S + t / C) * C + t % C];
        wp[i] = v;
    }
}

// Repack OHWI weights for the small-Cin window kernel: j=(r*R+s)-major,
// 8 channels per position, K zero-padded to a multiple of 64:
// wp[n][j*8 + c] = w[n][j/R][j%R][c] (zero for c >= C or j >= R*R).
__global__ void swin_repack_w_kernel(const bf16* __restrict__ w,
                                     bf16* __restrict__ wp, int Cout,
                                     int R, int C, int Kpad) {
    long total = (long)Cout * Kpad;
    long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long gs = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total; i += gs) {
        int k = (int)(i % Kpad);
        int n = (int)(i / Kpad);
        int j = k >> 3, c = k & 7;
        bf16 v = (bf16)0.f;
        if (j < R * R && c < C)
            v = w[((long)n * R * R + j) * C + c];
        wp[i] = v;
    }
}

// ---------------------------------------------------------------------------
// Small-Cin window convolution (the two stem classes): Cin padded to 8
// (ONE 16-B chunk per input pixel), Cout 64, R in {3,7}, stride in
// {1,2}. An 8x16 output tile stages its input window
// ((7*STRIDE+R) x (15*STRIDE+R) pixels) to LDS once; the K loop walks
// j=(r,s)-major 8-channel chunks, so each MFMA A-fragment is one window
// pixel's chunk. The weights are repacked j-major with a zero tail
// (swin_repack_w_kernel), so k-tiles past R*R*8 multiply zeros and the
// A side just clamps j. Replaces the spatial-prepad stem gather (12-49x
// input re-reads) for the ResNet 7x7/s2 and VGG 3x3/s1 Cin=3 stems.
template <int ACT, int R, int STRIDE>
__global__ __launch_bounds__(NTHREADS, 2) void conv_swin_kernel(
    ConvParams p) {
    constexpr int TH = 8, TW = 16, BM = TH * TW, BN = 64;
    constexpr int NI = BN / 16;                 // 4 waves along m
    constexpr int BCH = BN / 32;
    constexpr int WH = (TH - 1) * STRIDE + R;   // window rows
    constexpr int WW = (TW - 1) * STRIDE + R;   // window cols
    constexpr int WCH = WH * WW;                // 16-B chunks per window
    constexpr int NW = NTHREADS / WAVE;         // waves per block (4)
    constexpr int NSL = (WCH + 255) / 256;      // glds slices per wave
    constexpr int KP = (R * R * 8 + 63) / 64 * 64;   // padded K
    constexpr int NK = KP / 64;                 // k-tiles (phases)
    const bf16* __restrict__ X = (const bf16*)p.x;   // NHWC, Cin = 8
    const bf16* __restrict__ Wt = (const bf16*)p.w;  // repacked [64][KP]
    const bf16* __restrict__ Z = (const bf16*)p.zbuf;
    bf16* __restrict__ OUT = (bf16*)p.out;

    __shared__ __attribute__((aligned(16)))
    bf16 lds[(2 * WCH + 2 * BN * 8 + BM * BN / 8) * 8];
    bf16* W0 = lds;                              // two window buffers
    bf16* B0 = lds + 2 * WCH * 8;                // two B tiles
    float* scratch = (float*)(B0 + 2 * BN * BK); // epilogue bounce

    const int tid = threadIdx.x;
    const int wave = tid / WAVE;
    const int lane = tid % WAVE;
    const int wm = wave;
    const int n0 = blockIdx.y * BN;
    const int lo16 = lane & 15;
    const int hi4 = lane >> 4;
    const int ntw = (p.OW + TW - 1) / TW;
    const int nth = (p.OH + TH - 1) / TH;
    const int mtiles = p.NB * nth * ntw;

    // B lane offsets (Kpad % 64 == 0: no bounds math)
    int b_row[BCH], b_k8[BCH];
    u32 b_voff[BCH];
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
        int chunk = wave * (BCH * 64) + i * 64 + lane;
        b_row[i] = chunk / KCH;
        b_k8[i] = swz(b_row[i], chunk % KCH);
        int n = n0 + b_row[i];
        if (n >= p.Cout) n = p.Cout - 1;
        b_voff[i] = (u32)((u64)n * (u64)KP) + (u32)(b_k8[i] * 8);
    }
    auto stage_b = [&](int buf, int kt) {
        bf16* B = B0 + buf * BN * BK;
        const bf16* bbase = Wt + kt * BK;
#pragma unroll
        for (int i = 0; i < BCH; ++i)
            glds16(bbase + b_voff[i],
                   B + (wave * (BCH * 64) + i * 64) * 8);
    };

    // ---- window cursor (one window per m-tile; Cin block count is 1)
    int s_mt = blockIdx.x;
    int w_loff[NSL];
    u32 w_okm = 0;
    const bf16* w_base = X;
    int dst_buf = 0;
    auto win_setup = [&]() {
        int mt = s_mt;
        int tw = mt % ntw;
        int t = mt / ntw;
        int th = t % nth;
        int nb = t / nth;
        int oh0 = th * TH, ow0 = tw * TW;
        w_base = X + (long)nb * p.H * p.W * 8;
        w_okm = 0;
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
            int chunk = (j * 4 + wave) * 64 + lane;
            bool in = chunk < WCH;
            if (!in) chunk = WCH - 1;
            int iwl = chunk % WW;
            int ihl = chunk / WW;
            int ih = oh0 * STRIDE - p.pad + ihl;
            int iw = ow0 * STRIDE - p.pad + iwl;
            if (in && (u32)ih < (u32)p.H && (u32)iw < (u32)p.W)
                w_okm |= 1u << j;
            w_loff[j] = (ih * p.W + iw) * 8;
        }
    };
    auto stage_win_slice = [&](int j) {
        int chunk = (j * NW + wave) * 64 + lane;
        if (chunk < WCH) {
            const bf16* src =
                (w_okm >> j) & 1 ? w_base + w_loff[j] : Z;
            glds16(src, W0 + (long)dst_buf * WCH * 8 + chunk * 8);
        }
    };

    f32x4 acc[2][NI];
    auto compute = [&](int wbuf, int kt, int bbuf) {
        bf16* WB = W0 + (long)wbuf * WCH * 8;
        bf16* B = B0 + bbuf * BN * BK;
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks) {
            int j = kt * 8 + ks * 4 + hi4;       // (r, s) position index
            if (j > R * R - 1) j = R * R - 1;    // zero-weight tail
            int r = j / R, sI = j % R;           // compile-time-const div
            bf16x8 af[2], bfr[NI];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                int pp = wm * 32 + mi * 16 + lo16;
                int chunk = ((pp >> 4) * STRIDE + r) * WW
                            + (pp & 15) * STRIDE + sI;
                af[mi] = *reinterpret_cast<bf16x8*>(WB + chunk * 8);
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                int row = ni * 16 + lo16;
                bfr[ni] = *reinterpret_cast<bf16x8*>(
                    B + row * BK + swz(row, ks * 4 + hi4) * 8);
            }
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                    acc[mi][ni] =
                        MFMA_BF16_16x16x32(af[mi], bfr[ni], acc[mi][ni]);
        }
    };

    // ---- epilogue (dedicated scratch; BN==64, RH=64, 2 rounds)
    constexpr int RH = 64;
    constexpr int ROUNDS = BM / RH;
    auto epilogue = [&](int nb, int oh0, int ow0) {
        float sc[NI], bi[NI];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            int n = n0 + ni * 16 + lo16;
            if (n >= p.Cout) n = p.Cout - 1;
            sc[ni] = p.scale[n];
            bi[ni] = p.bias[n];
        }
        const bool interior =
            (oh0 + TH <= p.OH) && (ow0 + TW <= p.OW) &&
            (n0 + BN <= p.Cout) && (p.Cout % 8 == 0);
#pragma unroll
        for (int h = 0; h < ROUNDS; ++h) {
            const int r0 = h * RH;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        int r = wm * 32 + mi * 16 + hi4 * 4 + e;
                        if (r < r0 || r >= r0 + RH) continue;
                        int c = ni * 16 + lo16;
                        int rl = r - r0;
                        int cs = c ^ (((rl >> 2) & 3) << 4);
                        scratch[rl * BN + cs] =
                            acc[mi][ni][e] * sc[ni] + bi[ni];
                    }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (interior) {
                constexpr int CP8 = RH * BN / 8 / NTHREADS;
                f32x4 v4[CP8][2];
                long off[CP8];
#pragma unroll
                for (int i = 0; i < CP8; ++i) {
                    int chunk = tid + i * NTHREADS;
                    int rl = chunk / (BN / 8);
                    int c8 = (chunk % (BN / 8)) * 8;
                    int cs = c8 ^ (((rl >> 2) & 3) << 4);
                    int pp = r0 + rl;
                    long oh = oh0 + (pp >> 4), ow = ow0 + (pp & 15);
                    off[i] = (((long)nb * p.OH + oh) * p.OW + ow)
                                 * p.Cout + n0 + c8;
                    v4[i][0] = *reinterpret_cast<f32x4*>(
                        scratch + rl * BN + cs);
                    v4[i][1] = *reinterpret_cast<f32x4*>(
                        scratch + rl * BN + cs + 4);
                }
#pragma unroll
                for (int i = 0; i < CP8; ++i) {
                    bf16x8 o;
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        o[j] = f2bf(apply_act_hi(v4[i][j / 4][j % 4], ACT,
                                                 p.act_hi));
                    *reinterpret_cast<bf16x8*>(OUT + off[i]) = o;
                }
            } else {
                constexpr int CPR = RH * BN / 4 / NTHREADS;
#pragma unroll
                for (int i = 0; i < CPR; ++i) {
                    int chunk = tid + i * NTHREADS;
                    int rl = chunk / (BN / 4);
                    int c4 = (chunk % (BN / 4)) * 4;
                    int cs = c4 ^ (((rl >> 2) & 3) << 4);
                    int pp = r0 + rl;
                    int oh = oh0 + (pp >> 4), ow = ow0 + (pp & 15);
                    int n = n0 + c4;
                    if (oh >= p.OH || ow >= p.OW || n >= p.Cout)
                        continue;
                    f32x4 v4 = *reinterpret_cast<f32x4*>(
                        scratch + rl * BN + cs);
                    long off = (((long)nb * p.OH + oh) * p.OW + ow)
                                   * p.Cout + n;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (n + j >= p.Cout) continue;
                        OUT[off + j] =
                            f2bf(apply_act_hi(v4[j], ACT, p.act_hi));
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();   // scratch reuse next round
        }
    };

    // ---- main loop: one window per m-tile, NK phases each. Per phase:
    // wait -> barrier -> stage B(next) -> stage next window's slice
    // (j < NSL) -> compute. vmcnt float: the slice issued after B(cur)
    // in the previous phase (one glds per wave).
    const long local_tiles =
        (blockIdx.x < mtiles)
            ? (long)((mtiles - 1 - blockIdx.x) / gridDim.x + 1)
            : 0;
    if (local_tiles > 0) {
        win_setup();
#pragma unroll
        for (int j = 0; j < NSL; ++j) stage_win_slice(j);
        stage_b(0, 0);
        // cursor -> next window
        dst_buf ^= 1;
        s_mt += gridDim.x;
        if (s_mt < mtiles) win_setup();
    }
    long b_staged = 1;
    long ph = 0;
    long w = 0;
    bool sliced_prev = false;

    for (int mt = blockIdx.x; mt < mtiles; mt += gridDim.x, ++w) {
        int tw = mt % ntw;
        int t = mt / ntw;
        const int oh0 = (t % nth) * TH;
        const int nb = t / nth;
        const int ow0 = tw * TW;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
                acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};
        for (int kt = 0; kt < NK; ++kt, ++ph) {
            if (sliced_prev && !p.smul)
                asm volatile("s_waitcnt vmcnt(%0)" ::"i"(1) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (b_staged < local_tiles * NK) {
                stage_b((int)((ph + 1) & 1), (int)((ph + 1) % NK));
                ++b_staged;
            }
            bool sl = (kt < NSL) && (w + 1 < local_tiles) &&
                      (s_mt < mtiles) &&
                      ((kt * 4 + wave) * 64 < WCH);
            if (sl) stage_win_slice(kt);
            sliced_prev = sl;
            compute((int)(w & 1), kt, (int)(ph & 1));
        }
        // all waves done reading this window/B before the epilogue
        // overwrites nothing (dedicated scratch) — but scratch itself is
        // reused across rounds, so the first write must wait for the
        // previous m-tile's last reads of scratch: covered by the
        // barrier inside epilogue rounds and the phase-0 vmcnt(0)+
        // barrier of the NEXT m-tile
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        epilogue(nb, oh0, ow0);
        if (w + 1 < local_tiles) {
            dst_buf ^= 1;
            s_mt += gridDim.x;
            if (s_mt < mtiles) win_setup();
        }
    }
}

// ---------------------------------------------------------------------------
// host launchers
namespace defer_hip {

static u32 magic32(u32 d) {          // ceil(2^32 / d), d > 1
    return d <= 1 ? 0u : (u32)(((1ull << 32) + d - 1) / d);
}

// The dispatch table: exactly the instantiations the plans of conv_plan.h
// can name (the invariants there say what is left out). A row lists its
// template arguments after ACT, HAS_RES once; the key, the printed name
// and the four (act, res) kernels all come from that one token list.
typedef void (*ConvKernel)(ConvParams);
template <int ACT, bool, int R, int STRIDE>   // conv_swin_kernel has no RES
constexpr ConvKernel swin_kernel = conv_swin_kernel<ACT, R, STRIDE>;
struct ConvRow {
    ConvPlan::Family family;
    const char* args;
    std::array<int, 7> key;
    ConvKernel kernel[3][2];   // [none, relu, hardswish][has_res]
};
#define ROW(F, K, ...)                                                    \
    {ConvPlan::F, #__VA_ARGS__, {{__VA_ARGS__}},                          \
     {{K<ACT_NONE, false, __VA_ARGS__>, K<ACT_NONE, true, __VA_ARGS__>},  \
      {K<ACT_RELU, false, __VA_ARGS__>, K<ACT_RELU, true, __VA_ARGS__>},  \
      {K<ACT_HARDSWISH, false, __VA_ARGS__>,                              \
       K<ACT_HARDSWISH, true, __VA_ARGS__>}}}
// a tile config without B_PERSIST serves all four gathers; with it (K
// fits one tile) only GEMM and CONV
#define IGEMM_ROWS(...)                                                   \
    ROW(IGEMM, conv_igemm_kernel, AMODE_GEMM, false, __VA_ARGS__),        \
    ROW(IGEMM, conv_igemm_kernel, AMODE_CONV, false, __VA_ARGS__),        \
    ROW(IGEMM, conv_igemm_kernel, AMODE_RSC, false, __VA_ARGS__),         \
    ROW(IGEMM, conv_igemm_kernel, AMODE_STEM, false, __VA_ARGS__)
#define IGEMM_ROWS_BP(...)                                                \
    ROW(IGEMM, conv_igemm_kernel, AMODE_GEMM, true, __VA_ARGS__),         \
    ROW(IGEMM, conv_igemm_kernel, AMODE_CONV, true, __VA_ARGS__)
static const ConvRow conv_rows[] = {
    //             BM,  BN, DA, DB, WPS
    IGEMM_ROWS_BP(128, 64, 4, 2, 2),
    IGEMM_ROWS(128, 64, 3, 3, 2),
    IGEMM_ROWS_BP(128, 64, 3, 3, 2),   // legacy
    IGEMM_ROWS(128, 128, 2, 2, 2),
    IGEMM_ROWS(64, 128, 3, 3, 2),
    IGEMM_ROWS_BP(64, 64, 4, 2, 4),
    IGEMM_ROWS(64, 64, 3, 3, 3),
    IGEMM_ROWS_BP(64, 64, 4, 2, 2),
    IGEMM_ROWS(64, 64, 3, 3, 2),
    IGEMM_ROWS_BP(64, 64, 3, 3, 2),    // legacy
    ROW(WIN, conv_win_kernel, 64, 8, 256, 2),   // BN, TH, TPB, WPS
    ROW(WIN, conv_win_kernel, 64, 4, 256, 2),
    ROW(SWIN, swin_kernel, 3, 1),               // R, stride
    ROW(SWIN, swin_kernel, 3, 2),
};
static const char* const family_names[] = {"igemm", "win", "ws", "swin"};

static const ConvRow& find_row(const ConvPlan& pl) {
    for (const ConvRow& r : conv_rows)
        if (r.family == pl.family && r.key == plan_key(pl)) return r;
    throw std::runtime_error("no kernel for this plan: " + to_string(pl));
}

std::string conv_kernel_args(const ConvPlan& pl, bool has_res) {
    const char* res = has_res ? "true" : "false";
    if (pl.family == ConvPlan::WS) return res;   // conv_ws_kernel<ACT, RES>
    if (pl.family == ConvPlan::SWIN) return find_row(pl).args;
    return std::string(res) + ", " + find_row(pl).args;
}

std::vector<std::string> conv_table_rows() {
    std::vector<std::string> rows;
    for (const ConvRow& r : conv_rows)
        rows.push_back(std::string(family_names[r.family]) + ": " + r.args);
    return rows;
}

void launch_conv_igemm(const ConvParams& p0, const ConvPlan& pl, int act,
                       bool has_res, hipStream_t s) {
    if (act < 0 || act > 2)
        throw std::runtime_error("launch_conv_igemm: act must be 0, 1 or 2");
    static_assert(CONV_BK == BK && WIN_TW == WTW, "conv_plan.h tile sizes");
    ConvParams p = p0;
    if (pl.family != ConvPlan::SWIN) {
        p.owmul = magic32((u32)p.OW);
        p.ohmul = magic32((u32)p.OH);
        p.cmul = magic32((u32)p.Cin);
        p.smul = magic32((u32)p.S);
    }
    if (pl.family != ConvPlan::IGEMM)
        p.smul = pl.full_sync ? 1u : 0u;   // full-sync debug flag
    hipLaunchKernelGGL(find_row(pl).kernel[act][has_res],
                       dim3(pl.grid_x, pl.grid_y), dim3(NTHREADS), 0, s, p);
}

static int grid1d(long work, int block) {
    long g = (work + block - 1) / block;
    return (int)(g < 2048 ? g : 2048);
}

void launch_pad_channels(const void* x, void* y, long rows, int C, int C8,
                         hipStream_t s) {
    hipLaunchKernelGGL(pad_channels_kernel,
                       dim3(grid1d(rows * (C8 / 8), 256)), dim3(256), 0, s,
                       (const bf16*)x, (bf16*)y, rows, C, C8);
}

void launch_pad2d(const void* x, void* y, int NB, int H, int W, int C,
                  int PH, int PW, int ph0, int pw0, hipStream_t s) {
    int rows = NB * PH;
    hipLaunchKernelGGL(pad2d_kernel,
                       dim3(rows < 2048 ? rows : 2048), dim3(256), 0, s,
                       (const bf16*)x, (bf16*)y, NB, H, W, C, PH, PW,
                       ph0, pw0);
}

void launch_swin_repack_w(const void* w, void* wp, int Cout, int R,
                          int C, int Kpad, hipStream_t s) {
    hipLaunchKernelGGL(swin_repack_w_kernel,
                       dim3(grid1d((long)Cout * Kpad, 256)), dim3(256),
                       0, s, (const bf16*)w, (bf16*)wp, Cout, R, C,
                       Kpad);
}

void launch_stem_repack_w(const void* w, void* wp, int Cout, int R, int S,
                          int C, int TR, hipStream_t s) {
    hipLaunchKernelGGL(stem_repack_w_kernel,
                       dim3(grid1d((long)Cout * R * TR, 256)), dim3(256),
                       0, s, (const bf16*)w, (bf16*)wp, Cout, R, S, C,
                       TR);
}

}  // namespace defer_hip
