// Grouped 3x3 convolution + folded BN + activation for gfx950, NHWC, bf16 on
// the MFMA and a plain fp32 kernel (ResNeXt's conv2: 32 or 64 groups of 4 to
// 32 channels):
//
//   y[n][oh][ow][k] = act(scale[k] * sum_{r,s,c<Cg} x[n][oh*st-p+r][ow*st-p+s]
//                         [g(k)*Cg + c] * w[k][r][s][c] + bias[k]),  g(k) = k/Cg
//
// Cin == Cout == C, C % 16 == 0, Cg in {4, 8, 16, 32}, stride 1 or 2, pad 0
// or 1, w is [C][3][3][Cg].
//
// Neither of the other conv designs fits. It is not a depthwise VALU kernel
// (there is a reduction over 36 to 288 values), and it is not conv.hip's
// implicit GEMM: a 16-channel output fragment reads only its own 16 input
// channels (its group's 32 at Cg = 32), so the channel slabs are independent
// problems with tiny weights and nothing to reduce across.
//
// bf16 kernel (gconv_kernel<CG32, ST>)
// ------------------------------------
// Split: (spatial output tile) x (64-channel block). A workgroup of 4 waves
// owns 64 channels (blockIdx.y), so a staged pixel is a 128-byte run of x,
// and grid-strides over 16-pixel-wide tiles (8 rows at stride 1, 3 rows at
// stride 2, whose (2*TH+1) x 33 window is the larger one) of its channels.
// Wave v owns the 16 output channels 16*v .. 16*v+15 of the block for every
// pixel of the tile.
//
// MFMA: v_mfma_f32_16x16x32_bf16 with the weights as the M operand (16
// output channels) and 16 pixels of a tile row as N, so a lane ends up with
// 4 consecutive channels of one pixel. K = 32 is
//   Cg <= 16: two taps x the slab's 16 channels. Lane (lo16, hi4) reads tap
//             2*t + (hi4 >> 1), 8-channel chunk hi4 & 1: five MFMAs per
//             16x16 fragment, t = 0..4, the tenth tap slot multiplies by 0.
//             For Cg = 4 and 8 the weight fragments are block-diagonal:
//             zeros outside the Cg x Cg blocks of the slab's 4 or 2 groups.
//   Cg = 32:  one tap x the group's 32 channels, chunk hi4: nine MFMAs per
//             fragment; waves 2g and 2g+1 share the input of group g.
// The weight fragments are built once per workgroup in registers (20 VGPRs,
// 36 at Cg = 32) and stay there for the whole kernel; LDS holds input
// windows only.
//
// Useful MFMA work is 9*Cg / 160 = 22 % / 45 % / 90 % at Cg = 4 / 8 / 16 and
// 100 % at Cg = 32. That is acceptable because the op is memory-bound even
// at the densified rate: a fragment issues 5 * 16*16*32*2 = 81,920 flop for
// 256 outputs, 320 flop per output, and an output moves about 4 bytes (2 in,
// 2 out at stride 1), so 80 flop/B; nine MFMAs give 144 flop/B. At the
// 4.5 TB/s the streaming kernels reach that is 0.36 and 0.65 PFLOP/s of
// issued MFMA work, 14 % and 26 % of the card's 2.5 PFLOP/s bf16 peak.
//
// Window in LDS (16-byte chunks of 8 channels), conv_ws.hip's row image: a
// window row is
//   [c8 = 0,2,4,6][WW slots] | pad | [c8 = 1,3,5,7][WW slots]
// with the odd chunks ODD (a multiple of 16 chunks = once round the banks)
// after their even partners: the 16 lanes a ds_read_b128 services together
// are 8 pixels of an even chunk and the other 8 pixels of its odd partner,
// which then cover the 64 banks exactly once. At stride 2 the slots of a row
// hold the even columns first, then the odd ones, so the 16 pixels of a tap
// (columns 2j + s) are 16 neighbouring slots again.
// The window of the NEXT tile is fetched with global_load_lds into the other
// buffer at the top of a tile and is waited for (vmcnt(0) + barrier) at the
// top of the next one; padding, channels >= C and the pad chunks are read
// from a zero buffer, so the MFMA loop has no bounds logic.
//
// Epilogue: v = fmaf(acc, scale, bias), the runtime act (one instantiation
// per (Cg class, stride), not per act) in fp32, one rounding to bf16, an
// 8-byte write of the lane's 4 channels into the finished window buffer
// ([pixel][64 channels], chunk index xor-swizzled with the pixel), and after
// a barrier 16-byte stores of whole 128-byte pixel runs.
//
// Accumulation order: every output has one chain from a zero accumulator,
// MFMA t = 0, 1, .. in rising order (tap pairs (0,1) (2,3) .. (8,-) at
// Cg <= 16, taps 0..8 at Cg = 32, tap = r*3 + s), with the hardware's fixed
// order inside an MFMA. No atomics, no split-K: run-to-run identical.
// Non-finite inputs are outside the contract: the zero slots multiply other
// groups' values by 0.
//
// Tried and left: waves split along pixels instead of channels (each wave
// would hold the weights of all four slabs, 80 to 144 VGPRs, for the same
// LDS traffic); a 4-row tile at stride 2 (two 39.7 KB windows pass the 64 KB
// of static LDS).
//
// fp32 kernel (gconv_f32_kernel): one lane per 4 output channels of a pixel
// (one group, Cg % 4 == 0), fmaf in the fixed order (r, s, c), taps in the
// padding skipped. Plain and deterministic; no throughput is claimed.
#include "common.h"
#include "kernels.h"

// no packed fp32 instructions in this file's kernels: the epilogue's pairs of
// fmaf / max / min are cheap next to the memory traffic either way
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

constexpr int GC_TPB = 256;
constexpr int GC_TW = 16;           // tile columns = the N of one MFMA
constexpr int GC_CB = 64;           // channels of a workgroup
constexpr int GC_GRID_CAP = 512;    // workgroups: 2 per CU

template <int ST>
struct GcGeom {
    static constexpr int TH = ST == 1 ? 8 : 3;          // tile rows
    static constexpr int WH = (TH - 1) * ST + 3;        // window rows
    static constexpr int WW = (GC_TW - 1) * ST + 3;     // window columns
    static constexpr int EVEN = (WW + 1) / 2;           // even columns (ST 2)
    static constexpr int ODD = (4 * WW + 15) / 16 * 16; // odd-c8 offset
    static constexpr int ROW = ODD + 4 * WW;            // chunks per row
    static constexpr int WCH = WH * ROW;                // chunks per window
    static constexpr int NSL = (WCH + GC_TPB - 1) / GC_TPB;
    // slot of tap column s relative to the slot of output column j
    static constexpr int tap_slot(int s) {
        return ST == 1 ? s : (s == 1 ? EVEN : s / 2);
    }
};

__device__ __forceinline__ void gc_glds16(const bf16* src, bf16* lds_base) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)lds_base, 16, 0,
        0);
}

__device__ __forceinline__ float gc_act(float v, int act) {
    if (act == ACT_HARDSWISH) return hardswish_f(v);
    if (act != ACT_NONE) v = fmaxf(v, 0.0f);
    if (act == ACT_RELU6) v = fminf(v, 6.0f);
    return v;
}

struct GcParams {
    const bf16* x;
    const bf16* w;
    const float* scale;
    const float* bias;
    const bf16* zbuf;
    bf16* y;
    int NB, H, W, C, OH, OW, Cg, pad, act;
};

template <bool CG32, int ST>
__global__ __launch_bounds__(GC_TPB, 2) void gconv_kernel(GcParams p) {
    typedef GcGeom<ST> G;
    constexpr int NT = CG32 ? 9 : 5;            // MFMAs per fragment
    constexpr int WEL = G::WCH * 8;             // bf16 per window buffer
    static_assert(G::TH * GC_TW * GC_CB <= WEL, "bounce fits the window");
    static_assert(2 * WEL * 2 <= 65536, "static LDS");

    __shared__ __attribute__((aligned(16))) bf16 lds[2 * WEL];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int lane = tid % WAVE;
    const int lo16 = lane & 15;
    const int hi4 = lane >> 4;
    const int cb0 = blockIdx.y * GC_CB;         // first channel of the block
    const int ntw = (p.OW + GC_TW - 1) / GC_TW;
    const int nth = (p.OH + G::TH - 1) / G::TH;
    const int mtiles = p.NB * nth * ntw;
    const int first = blockIdx.x;
    if (first >= mtiles) return;

    // ---- window staging: slice j of this wave is the 64 chunks from
    // (j*4 + wave)*64, one per lane (lane-linear in LDS)
    auto stage = [&](int mt, int buf) {
        const int tw = mt % ntw;
        const int t = mt / ntw;
        const int ih0 = (t % nth) * G::TH * ST - p.pad;
        const int iw0 = tw * GC_TW * ST - p.pad;
        const bf16* img = p.x + (long)(t / nth) * p.H * p.W * p.C;
#pragma unroll
        for (int j = 0; j < G::NSL; ++j) {
            const int piece = (j * 4 + wave) * 64;          // wave-uniform
            const int chunk = piece + lane;
            // lanes past the last chunk must not write: they would land in
            // the other window
            if (j < G::NSL - 1 || chunk < G::WCH) {
                const int ihl = chunk / G::ROW;
                const int pos = chunk - ihl * G::ROW;
                const bool odd = pos >= G::ODD;
                const int q = odd ? pos - G::ODD : pos;
                const int cp = q / G::WW;               // >= 4: pad chunks
                const int slot = q - cp * G::WW;
                const int col = ST == 1 ? slot
                    : (slot < G::EVEN ? 2 * slot : 2 * (slot - G::EVEN) + 1);
                const int ih = ih0 + ihl;
                const int iw = iw0 + col;
                const int ch = cb0 + cp * 16 + (odd ? 8 : 0);
                const bool in = (cp < 4) & (ch < p.C) &
                                ((u32)ih < (u32)p.H) & ((u32)iw < (u32)p.W);
                const int off = (ih * p.W + iw) * p.C + ch;
                const bf16* src = (in ? img : p.zbuf) + (in ? off : 0);
                gc_glds16(src, lds + (buf * G::WCH + piece) * 8);
            }
        }
    };
    stage(first, 0);

    // ---- weights: this wave's fragments, resident for the whole kernel.
    // Lane (lo16, hi4) holds output channel kch = its slab's lo16-th.
    const int kch = cb0 + wave * 16 + lo16;
    const bool wave_ok = cb0 + wave * 16 < p.C;     // C % 16 == 0: all or none
    bf16x8 wfr[NT];
    float sc[4], bi[4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j) wfr[t][j] = f2bf(0.0f);
#pragma unroll
    for (int e = 0; e < 4; ++e) sc[e] = bi[e] = 0.0f;
    if (wave_ok) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sc[e] = p.scale[cb0 + wave * 16 + hi4 * 4 + e];
            bi[e] = p.bias[cb0 + wave * 16 + hi4 * 4 + e];
        }
        if constexpr (CG32) {
#pragma unroll
            for (int t = 0; t < 9; ++t)
                wfr[t] = load_bf16x8(p.w + ((long)kch * 9 + t) * 32 + hi4 * 8);
        } else {
            const int cg = p.Cg;
            const int kgrp = lo16 / cg;             // kch's group in the slab
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const int tap = 2 * t + (hi4 >> 1);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int cs = (hi4 & 1) * 8 + j;       // slab channel
                    const int cgrp = cs / cg;
                    if (tap < 9 && cgrp == kgrp)
                        wfr[t][j] = p.w[((long)kch * 9 + tap) * cg +
                                        (cs - cgrp * cg)];
                }
            }
        }
    }

    // ---- the lane's place in a window: chunk c8 of the block, pixel lo16
    const int c8 = CG32 ? (wave >> 1) * 4 + hi4 : wave * 2 + (hi4 & 1);
    const int lane_el = ((c8 >> 1) * G::WW + (c8 & 1) * G::ODD + lo16) * 8;
    int toff[NT];                               // tap offsets, in bf16
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        // the zero slot (tap 9) reads tap 8's pixels and multiplies by 0
        const int tap = CG32 ? t : min(2 * t + (hi4 >> 1), 8);
        const int r = tap / 3, s = tap - r * 3;
        const int slot = ST == 1 ? s : (s == 1 ? G::EVEN : s >> 1);
        toff[t] = (r * G::ROW + slot) * 8;
    }

    int buf = 0;
    for (int mt = first; mt < mtiles; mt += gridDim.x) {
        const int tw = mt % ntw;
        const int t_ = mt / ntw;
        const int oh0 = (t_ % nth) * G::TH;
        const int nb = t_ / nth;
        const int ow0 = tw * GC_TW;
        const int nxt = mt + gridDim.x;

        // the one wait of a window: this tile's slices (issued a whole tile
        // ago) have landed, for every wave; every wave is also past the
        // previous read-out, so the other buffer is free to refill
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (nxt < mtiles) stage(nxt, buf ^ 1);

        const bf16* WB = lds + buf * WEL + lane_el;
        f32x4 acc[G::TH];
#pragma unroll
        for (int mi = 0; mi < G::TH; ++mi) acc[mi] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mi = 0; mi < G::TH; ++mi)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const bf16x8 xv = *reinterpret_cast<const bf16x8*>(
                    WB + mi * ST * G::ROW * 8 + toff[t]);
                acc[mi] = MFMA_BF16_16x16x32(wfr[t], xv, acc[mi]);
            }

        // ---- epilogue: bounce through the finished window buffer
        bf16* bounce = lds + buf * WEL;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();           // all waves done with window
        asm volatile("" ::: "memory");
#pragma unroll
        for (int mi = 0; mi < G::TH; ++mi) {
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                o[e] = f2bf(gc_act(fmaf(acc[mi][e], sc[e], bi[e]), p.act));
            const int px = mi * GC_TW + lo16;
            const int q = wave * 2 + (hi4 >> 1);
            *reinterpret_cast<bf16x4*>(
                bounce + px * GC_CB + ((q ^ (px & 7)) * 8) + (hi4 & 1) * 4) = o;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        constexpr int NOUT = G::TH * GC_TW * (GC_CB / 8);   // 16-byte stores
#pragma unroll
        for (int i = 0; i < (NOUT + GC_TPB - 1) / GC_TPB; ++i) {
            const int id = tid + i * GC_TPB;
            const int px = id >> 3, q = id & 7;
            const int oh = oh0 + (px >> 4), ow = ow0 + (px & 15);
            const int ch = cb0 + q * 8;
            if (id < NOUT && oh < p.OH && ow < p.OW && ch < p.C) {
                const bf16x8 v = *reinterpret_cast<const bf16x8*>(
                    bounce + px * GC_CB + ((q ^ (px & 7)) * 8));
                store_bf16x8(p.y + (((long)nb * p.OH + oh) * p.OW + ow) * p.C +
                                 ch, v);
            }
        }
        // the read-out retires at the next tile's top barrier; its buffer is
        // refilled only after that
        buf ^= 1;
    }
}

__global__ __launch_bounds__(GC_TPB) void gconv_f32_kernel(
    const float* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ scale, const float* __restrict__ bias,
    float* __restrict__ y, int NB, int H, int W, int C, int OH, int OW,
    int Cg, int stride, int pad, int act) {
    const int C4 = C / 4;
    const long total = (long)NB * OH * OW * C4;
    const long gstride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += gstride) {
        const int k = (int)(i % C4) * 4;
        long t = i / C4;
        const int ow = (int)(t % OW);
        t /= OW;
        const int oh = (int)(t % OH);
        const int n = (int)(t / OH);
        const int c0 = k / Cg * Cg;             // Cg % 4 == 0: one group
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int r = 0; r < 3; ++r) {
            const int ih = oh * stride - pad + r;
            if (ih < 0 || ih >= H) continue;
            for (int s = 0; s < 3; ++s) {
                const int iw = ow * stride - pad + s;
                if (iw < 0 || iw >= W) continue;
                const float* xp = x + (((long)n * H + ih) * W + iw) * C + c0;
                const float* wp = w + ((long)k * 9 + r * 3 + s) * Cg;
                for (int c = 0; c < Cg; c += 4) {
                    const f32x4 xv = *reinterpret_cast<const f32x4*>(xp + c);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 wv = *reinterpret_cast<const f32x4*>(
                            wp + (long)j * 9 * Cg + c);
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            acc[j] = fmaf(xv[u], wv[u], acc[j]);
                    }
                }
            }
        }
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[j] = gc_act(fmaf(acc[j], scale[k + j], bias[k + j]), act);
        *reinterpret_cast<f32x4*>(
            y + (((long)n * OH + oh) * OW + ow) * C + k) = o;
    }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

namespace defer_hip {

void launch_gconv(const void* x, const void* w, const float* scale,
                  const float* bias, const void* zbuf, void* y, int NB, int H,
                  int W, int C, int OH, int OW, int Cg, int stride, int pad,
                  int act, hipStream_t s) {
    GcParams p{(const bf16*)x, (const bf16*)w, scale, bias, (const bf16*)zbuf,
               (bf16*)y, NB, H, W, C, OH, OW, Cg, pad, act};
    const int th = stride == 1 ? GcGeom<1>::TH : GcGeom<2>::TH;
    const long tiles = (long)NB * ((OH + th - 1) / th) *
                       ((OW + GC_TW - 1) / GC_TW);
    if (tiles <= 0) return;
    const int cbs = (C + GC_CB - 1) / GC_CB;
    const long cap = GC_GRID_CAP / cbs > 0 ? GC_GRID_CAP / cbs : 1;
    const dim3 grid((unsigned)(tiles < cap ? tiles : cap), (unsigned)cbs);
    static void (*const kernel[2][2])(GcParams) = {
        {gconv_kernel<false, 1>, gconv_kernel<false, 2>},
        {gconv_kernel<true, 1>, gconv_kernel<true, 2>}};
    hipLaunchKernelGGL(kernel[Cg == 32][stride == 2], grid, dim3(GC_TPB), 0,
                       s, p);
}

void launch_gconv_f32(const float* x, const float* w, const float* scale,
                      const float* bias, float* y, int NB, int H, int W,
                      int C, int OH, int OW, int Cg, int stride, int pad,
                      int act, hipStream_t s) {
    const long total = (long)NB * OH * OW * (C / 4);
    if (total <= 0) return;
    const long g = (total + GC_TPB - 1) / GC_TPB;
    hipLaunchKernelGGL(gconv_f32_kernel, dim3((unsigned)(g < 8192 ? g : 8192)),
                       dim3(GC_TPB), 0, s, x, w, scale, bias, y, NB, H, W, C,
                       OH, OW, Cg, stride, pad, act);
}

}  // namespace defer_hip
