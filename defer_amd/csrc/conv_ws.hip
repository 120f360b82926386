// Weight-stationary window convolution for gfx950: 3x3 / stride 1 / pad 1,
// Cin = Cout = 64, bf16 NHWC (ResNet layer1's 3x3s, VGG block1_conv2).
//
// conv_win_kernel (conv.hip) stages the 8 KB weight tile of every (r,s)
// phase of every output tile from L2 into LDS — 72 KB of weights per
// 23 KB window, one block-wide barrier and one counted wait per phase for
// 16 MFMAs a wave. The whole 3x3x64x64 weight tensor is 72 KB, so here it
// never goes through LDS at all: each wave keeps the 36 B fragments of its
// 32 output channels in registers (144 VGPRs) for the whole kernel, the
// way stem_pool.hip keeps its 24. LDS holds only the input windows.
//
// Output is bit-identical to conv_win_kernel and to the AMODE_RSC
// implicit GEMM for this shape: same MFMA (16x16x32 bf16), same lane -> k
// mapping inside a fragment (channel chunk ks*4 + hi4), one accumulation
// chain per output from a zero accumulator with (r,s) ascending and the
// two 32-channel halves ascending inside each, and the same epilogue
// expression through the same fp32 LDS bounce.
//
// Tiling: an 8x16-pixel output tile per step, 256 threads as 2 waves along
// pixels (4 tile rows each) x 2 along channels (32 each). A wave runs
// 9 x 2 x 4 x 2 = 144 MFMAs per tile from 72 ds_read_b128 (each A
// fragment feeds both n-fragments) with no barrier and no vmcnt wait in
// between; the six glds slices of the NEXT tile's window are issued during
// the first six (r,s) phases into the other window buffer. Block-wide
// synchronisation is once per window (vmcnt(0) + barrier at the tile top)
// plus the four barriers of the two bounce rounds of the epilogue.
//
// Window image in LDS (16-B chunks of 8 channels): one window row is
//   [c8 = 0,2,4,6][18 px] | 8 unused | [c8 = 1,3,5,7][18 px]
// = 152 chunks, the odd chunks 80 after their even partners. The 16 lanes
// that ds_read_b128 services together are 8 pixels of chunk ks*4 + 2h and
// the other 8 pixels of chunk ks*4 + 2h + 1; with the partner row a
// multiple of 16 chunks (256 B, once round the 64 banks) away the two
// halves cover all 64 banks exactly once for every (r,s) shift.
// conv_win_kernel's [c8][18] rows put them 18 chunks apart, which makes
// two of the sixteen lanes collide (2 LDS cycles per lane group, 8 instead
// of 4 per fragment read).
#include <cstdlib>

#include "common.h"
#include "conv_plan.h"
#include "kernels.h"

using defer_hip::ConvParams;

#define WS_TPB 256
#define WS_TH 8
#define WS_TW 16
#define WS_WH (WS_TH + 2)           // window rows
#define WS_WW (WS_TW + 2)           // window columns
#define WS_ODD 80                   // chunk offset of the odd-c8 rows
#define WS_ROW 152                  // chunks per window row
#define WS_WCH (WS_WH * WS_ROW)     // chunks per window (24,320 B)
#define WS_NSL ((WS_WCH + WS_TPB - 1) / WS_TPB)   // glds slices per wave
#define WS_K (9 * 64)

__device__ __forceinline__ void ws_glds16(const bf16* src, bf16* lds_base) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)lds_base, 16, 0,
        0);
}

template <int ACT, bool HAS_RES>
__global__ __launch_bounds__(WS_TPB, 2) void conv_ws_kernel(ConvParams p) {
    constexpr int BM = WS_TH * WS_TW, BN = 64;
    constexpr int RH = BM / 2;                  // bounce rows per round
    const bf16* __restrict__ X = (const bf16*)p.x;
    const bf16* __restrict__ Wt = (const bf16*)p.w;
    const bf16* __restrict__ Z = (const bf16*)p.zbuf;
    const bf16* __restrict__ RES = (const bf16*)p.res;
    bf16* __restrict__ OUT = (bf16*)p.out;

    __shared__ __attribute__((aligned(16))) bf16 lds[2 * WS_WCH * 8];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int lane = tid % WAVE;
    const int lo16 = lane & 15;
    const int hi4 = lane >> 4;
    const int wm = wave >> 1;                   // pixel half (4 tile rows)
    const int wn = wave & 1;                    // channel half
    const int ntw = (p.OW + WS_TW - 1) / WS_TW;
    const int nth = (p.OH + WS_TH - 1) / WS_TH;
    const int mtiles = p.NB * nth * ntw;

    // ---- window staging: slice j of this wave is the 64 chunks from
    // (j*4 + wave)*64, one per lane (lane-linear in LDS). A chunk's place
    // in the window (row, column, channel chunk) never changes, but six
    // slices of it held in registers next to 144 of weights spill, so it
    // is rebuilt from the lane id at each use (about 25 VALU beside the
    // MFMAs); s_lane is re-made opaque once per tile to keep it that way.
    int s_lane = lane;
    const bf16* s_img = X;
    int s_oh0 = 0, s_ow0 = 0;
    auto win_setup = [&](int mt) {
        const int tw = mt % ntw;
        const int t = mt / ntw;
        s_oh0 = (t % nth) * WS_TH;
        s_ow0 = tw * WS_TW;
        s_img = X + (long)(t / nth) * p.H * p.W * 64;
        asm volatile("" : "+v"(s_lane));
    };
    // live = false (no next tile) turns the slice into zeros written to
    // the idle buffer, so the phases carry no branch around it
    auto stage_slice = [&](int j, int buf, bool live) {
        const int piece = (j * 4 + wave) * 64;          // wave-uniform
        const int chunk = piece + s_lane;
        // lanes past the last chunk must not write: they would land in
        // the partner window. Only the tail of the last slice is masked,
        // so lane 0 of an issuing wave is always active.
        if (j < WS_NSL - 1 || chunk < WS_WCH) {
            const int ihl = (int)__umulhi((u32)chunk,
                                          (0xFFFFFFFFu / WS_ROW) + 1);
            const int pos = chunk - ihl * WS_ROW;
            const bool odd = pos >= WS_ODD;
            const int q = odd ? pos - WS_ODD : pos;
            const int cp = (q * 3641) >> 16;             // q / 18, q < 80
            const int iwl = q - cp * WS_WW;
            const int ih = s_oh0 - 1 + ihl;
            const int iw = s_ow0 - 1 + iwl;
            // the 8 unused chunks of a row are written with zeros
            const bool in = live & (cp < 4) & ((u32)ih < (u32)p.H) &
                            ((u32)iw < (u32)p.W);
            const int off = (ih * p.W + iw) * 64 + cp * 16 + (odd ? 8 : 0);
            // two selects, not a branch round the address arithmetic
            const bf16* src = (in ? s_img : Z) + (in ? off : 0);
            ws_glds16(src, lds + (buf * WS_WCH + piece) * 8);
        }
    };

    const int first = blockIdx.x;
    if (first >= mtiles) return;
    win_setup(first);
#pragma unroll
    for (int j = 0; j < WS_NSL; ++j) stage_slice(j, 0, true);

    // ---- weights: every fragment this wave will ever need, straight from
    // the OHWI tensor (a fragment's 16 bytes are contiguous in
    // w[n][r][s][c]), resident for the whole kernel
    bf16x8 bfr[9][2][2];
    float sc[2], bi[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int n = wn * 32 + ni * 16 + lo16;
        sc[ni] = p.scale[n];
        bi[ni] = p.bias[n];
#pragma unroll
        for (int rs = 0; rs < 9; ++rs)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                bfr[rs][ks][ni] = load_bf16x8(
                    Wt + n * WS_K + rs * 64 + (ks * 4 + hi4) * 8);
    }

    // A fragment of tile row (wm*4 + mi) shifted by (r,s), k-step ks:
    // lane base + ((mi + r) * WS_ROW + ks * 2 * WS_WW + s) chunks
    const int a_lane = (wm * 4 * WS_ROW + (hi4 >> 1) * WS_WW +
                        (hi4 & 1) * WS_ODD + lo16) * 8;

    int buf = 0;
    for (int mt = first; mt < mtiles; mt += gridDim.x) {
        const int tw = mt % ntw;
        const int t = mt / ntw;
        const int oh0 = (t % nth) * WS_TH;
        const int nb = t / nth;
        const int ow0 = tw * WS_TW;
        const int nxt = mt + gridDim.x;
        const bool has_next = nxt < mtiles;

        // the one wait of a window: this tile's slices (issued a whole
        // tile ago) have landed, for every wave; every wave is also past
        // the previous epilogue, so the other buffer is free to refill
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (has_next) win_setup(nxt);

        const bf16* WB = lds + buf * (WS_WCH * 8) + a_lane;
        f32x4 acc[4][2];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
                acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};
        // 18 steps (rs, ks) of 4 A reads + 8 MFMAs. The reads of step
        // st + 1 are issued in front of the MFMAs of step st and pinned
        // there, so a fragment has 8 MFMAs (128 cycles) to arrive; left
        // alone hipcc sinks each read pair directly in front of its use.
        auto a_load = [&](bf16x8* af, int st) {
            const int rs = st >> 1, ks = st & 1;
            const int r = rs / 3, s = rs % 3;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                af[mi] = *reinterpret_cast<const bf16x8*>(
                    WB + ((mi + r) * WS_ROW + ks * 2 * WS_WW + s) * 8);
        };
        bf16x8 af[2][4];
        a_load(af[0], 0);
#pragma unroll
        for (int st = 0; st < 18; ++st) {
            const int rs = st >> 1, ks = st & 1;
            if (st + 1 < 18) a_load(af[(st + 1) & 1], st + 1);
            __builtin_amdgcn_sched_barrier(0);
            if (ks == 0 && rs < WS_NSL) stage_slice(rs, buf ^ 1, has_next);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    acc[mi][ni] = MFMA_BF16_16x16x32(
                        af[st & 1][mi], bfr[rs][ks][ni], acc[mi][ni]);
            __builtin_amdgcn_sched_barrier(0);
        }

        // ---- epilogue: fp32 bounce through the finished window buffer,
        // two rounds of 64 pixels (round h is written by the waves of
        // pixel half h), same swizzle and expressions as conv_win_kernel
        float* scratch = (float*)(lds + buf * (WS_WCH * 8));
        const bool interior =
            (oh0 + WS_TH <= p.OH) && (ow0 + WS_TW <= p.OW);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // all waves done with the window (h = 0) / the last round
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (wm == h) {
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int rl = mi * 16 + hi4 * 4 + e;
                            const int c = wn * 32 + ni * 16 + lo16;
                            const int cs = c ^ (((rl >> 2) & 3) << 4);
                            scratch[rl * BN + cs] =
                                acc[mi][ni][e] * sc[ni] + bi[ni];
                        }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const int r0 = h * RH;
            if (interior) {
                constexpr int CP8 = RH * BN / 8 / WS_TPB;       // 2
                f32x4 v4[CP8][2];
                bf16x8 rv[CP8];
                long off[CP8];
#pragma unroll
                for (int i = 0; i < CP8; ++i) {
                    const int chunk = tid + i * WS_TPB;
                    const int rl = chunk / (BN / 8);
                    const int c8 = (chunk % (BN / 8)) * 8;
                    const int cs = c8 ^ (((rl >> 2) & 3) << 4);
                    const int pp = r0 + rl;
                    const long oh = oh0 + (pp >> 4), ow = ow0 + (pp & 15);
                    off[i] = (((long)nb * p.OH + oh) * p.OW + ow) * BN + c8;
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
                constexpr int CPR = RH * BN / 4 / WS_TPB;       // 4
#pragma unroll
                for (int i = 0; i < CPR; ++i) {
                    const int chunk = tid + i * WS_TPB;
                    const int rl = chunk / (BN / 4);
                    const int c4 = (chunk % (BN / 4)) * 4;
                    const int cs = c4 ^ (((rl >> 2) & 3) << 4);
                    const int pp = r0 + rl;
                    const int oh = oh0 + (pp >> 4), ow = ow0 + (pp & 15);
                    if (oh >= p.OH || ow >= p.OW) continue;
                    f32x4 v4 = *reinterpret_cast<f32x4*>(
                        scratch + rl * BN + cs);
                    const long off =
                        (((long)nb * p.OH + oh) * p.OW + ow) * BN + c4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float v = v4[j];
                        if (HAS_RES) v += bf2f(RES[off + j]);
                        OUT[off + j] = f2bf(apply_act_hi(v, ACT, p.act_hi));
                    }
                }
            }
        }
        // the last round's bounce reads retire at the next tile's top
        // barrier; its buffer is refilled only after that
        buf ^= 1;
    }
}

namespace defer_hip {

ConvWsLaunch launch_conv_ws(const ConvParams& p, int act, bool has_res,
                            int max_blocks, hipStream_t s) {
    if (act < 0 || act > 2)
        throw std::runtime_error("launch_conv_ws: act must be 0, 1 or 2");
    static_assert(WS_TH == 8 && WS_TW == WIN_TW && WS_K == 9 * CONV_BK,
                  "conv_plan.h plans 8x16 tiles");
    // mode 1: the caller has chosen this kernel; the plan is its grid
    const ConvPlan pl = plan_conv(p, false, false, 1, max_blocks, '\0');
    if (pl.family != ConvPlan::WS)
        throw std::runtime_error("no kernel for this plan: " +
                                 to_string(pl));
    static void (*const kernel[3][2])(ConvParams) = {
        {conv_ws_kernel<ACT_NONE, false>, conv_ws_kernel<ACT_NONE, true>},
        {conv_ws_kernel<ACT_RELU, false>, conv_ws_kernel<ACT_RELU, true>},
        {conv_ws_kernel<ACT_HARDSWISH, false>,
         conv_ws_kernel<ACT_HARDSWISH, true>}};
    hipLaunchKernelGGL(kernel[act][has_res], dim3(pl.blocks),
                       dim3(WS_TPB), 0, s, p);
    return ConvWsLaunch{pl.blocks, pl.tiles_per_block};
}

}  // namespace defer_hip
