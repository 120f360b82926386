// Shifted-window attention of a Swin block for gfx950, in one kernel: bf16 on
// the MFMA and a plain fp32 kernel. qkv is the NHWC output of the block's qkv
// 1x1 conv, [N][H][W][3][heads][32]; out is [N][H][W][heads][32]; table is
// the learned relative-position bias, [(2w - 1)^2][heads]. With w the window
// side, s the shift and T = w * w:
//
//   shifted frame: (r', c') holds pixel ((r' + s) mod H, (c' + s) mod W)
//   window (r' / w, c' / w), token t = (r' % w) * w + (c' % w) = (i, j)
//   score(tq, tk) = (q . k) * 32^-0.5
//                   + table[(iq - ik + w - 1) * (2w - 1) + (jq - jk + w - 1)][h]
//                   + (s > 0 and region(tq) != region(tk) ? -100 : 0)
//   region of a shifted row r': 0 below H - w, 1 below H - s, else 2; columns
//   likewise with W; two tokens are apart when either differs
//   out[pixel of tq][h][:] = sum_tk softmax_tk(score)[tk] * v[pixel of tk][h][:]
//
// The roll, the window partition, their inverses, the bias gather and the
// mask are all addressing and integer compares in here: q, k and v are read
// in place from each token's source pixel and the output is written to the
// query's source pixel. No score, mask or partitioned tensor exists.
//
// Why not attention_kernel: a window is at most 64 keys of 32 channels, less
// than one of its key tiles. There is no key loop, so no online softmax, no
// K/V ring and no barrier; what is left is small enough for one wave.
//
// bf16 kernel (window_attention_kernel)
// -------------------------------------
// Split: one wave owns one (image, window, head) pair for the whole kernel. A
// workgroup is four waves over the flat pair index with the head fastest, so
// the waves of a block mostly read neighbouring 64-byte runs of the same
// pixels, heads = 3 wastes nothing, and only the last block can have idle
// waves (window_attention_geom). Waves never meet: each has its own 6.5 KB of
// LDS, there is no s_barrier, and a wave without a pair leaves at once.
//
// Token table: lane L works out token L once, with the kernel's only integer
// division: the pixel index of its source (tokens >= T take token T - 1, a
// pixel of the tensor) and a code, a = i * (2w - 1) + j in the low half and
// the region 3 * row_region + col_region in the high half. Both go to LDS.
// For a query code cq (with (w - 1) * 2w added to a) and a key code ck,
// d = cq - ck has the bias index, which is >= 0, in its low half and the
// region difference above it: the bias is bias_lds[d & 0xffff] and the pair
// is masked when (unsigned)d > 0xffff. Unshifted windows have region 0
// everywhere, so the same code serves them without a branch. A lane holds
// the codes of its 16 keys in registers (four 16-byte LDS reads).
//
// Bias: the head's column of the table, at most 225 values, is staged into
// LDS as fp32 once; a score's bias is one 4-byte LDS read whose index steps
// by one from query to query, so the 16 lanes of a key hit 16 banks.
//
// Q and K never touch LDS. The 64 padded tokens are four 16-row groups. Lane
// (lo16, hi4) of either MFMA operand wants channels hi4*8 .. hi4*8 + 7 of
// token g*16 + lo16: one 16-byte global load from the token's pixel (D = 32
// is exactly one K-step). S^T = K Q^T with K as the M operand, as in
// attention.hip: the lane then holds, for the query lo16 of group g, the keys
// kt*16 + hi4*4 + e of each 16-key subtile kt, i.e. a query's whole score row
// sits in four lanes, 16 scores each.
//
// Softmax, fp32, one pass: sc = fma(acc, 32^-0.5, bias) (- 100 if masked);
// t = sc * log2 e; keys >= T get -inf (token 0 is always live, so no row max
// is -inf); max over the lane's 16 and two xor-shuffles (^16, ^32);
// p = exp2(t - max); l sums the fp32 p, in the lane and then over the same
// two shuffles.
//
// V is the one operand that needs a transpose: the window's 64 x 32 tile goes
// through LDS, rows of 80 B (64 B + 16 B of padding: rows four apart, which
// the four hi4 groups of one 2-byte read touch, are 64 banks' worth / 4
// apart). O^T = V^T P^T: the lane's p of subtiles 2s and 2s + 1, rounded once
// to bf16, are the N operand of K-step s if k-slot hi4*8 + j stands for key
// s*32 + (j >> 2)*16 + hi4*4 + (j & 3); the V^T fragments are gathered in
// that order with 2-byte LDS reads (the form attention.hip verified against
// the documented operand layout), once per wave, for all four query groups.
// The result lane holds O^T[db*16 + hi4*4 + e][query lo16]: its own query, so
// 1 / l is a per-lane multiply; one rounding to bf16 and two 8-byte stores to
// the query's source pixel. Query rows >= T are computed and not stored.
//
// Per pair: 8 + 4 16-byte global loads per lane, 16 MFMAs for S and 16 for O
// at T = 49 (groups past T are skipped), no atomics, one fixed order:
// run-to-run identical.
//
// fp32 kernel (window_attention_f32_kernel): one wave per pair, one lane per
// query token, q and O in registers, the window's K and V in LDS (every lane
// reads the same key row: a broadcast). Two passes over the keys with the
// same score code, the max first, then p = exp2(t - max), l and O by fmaf in
// key order; O / l at the end. Plain and deterministic; no throughput is
// claimed.
#include "common.h"
#include "kernels.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

constexpr int WA_TPB = 256;
constexpr int WA_WAVES = WA_TPB / WAVE;     // pairs of a workgroup
constexpr int WA_D = 32;                    // head dim
constexpr int WA_TOK = 64;                  // padded tokens of a window
constexpr int WA_VP = WA_D + 8;             // bf16 per V row in LDS (80 B)
constexpr int WA_NB = 256;                  // bias column, >= (2*8 - 1)^2
constexpr float WA_SCALE = 0.17677669529663687f;    // 32^-0.5
constexpr float WA_LOG2E = 1.4426950408889634f;

struct WaParams {
    const void* qkv;
    const void* table;
    void* out;
    int H, W, heads, C, w, s, nwh, nww, T, pairs;
};

struct WaPair { int n, wr, wc, h; };

__device__ __forceinline__ WaPair wa_pair(const WaParams& p, int pair) {
    WaPair a;
    a.h = pair % p.heads;
    int win = pair / p.heads;
    a.wc = win % p.nww;
    win /= p.nww;
    a.wr = win % p.nwh;
    a.n = win / p.nwh;
    return a;
}

// Token t of the window: the index of its source pixel and its code (header).
__device__ __forceinline__ void wa_token(const WaParams& p, const WaPair& a,
                                         int t, int& pix, int& code) {
    const int tt = min(t, p.T - 1);
    const int i = tt / p.w, j = tt - i * p.w;
    const int rs = a.wr * p.w + i, cs = a.wc * p.w + j;    // shifted frame
    int r = rs + p.s, c = cs + p.s;
    if (r >= p.H) r -= p.H;
    if (c >= p.W) c -= p.W;
    pix = (a.n * p.H + r) * p.W + c;
    int reg = 0;
    if (p.s > 0) {
        const int rr = rs < p.H - p.w ? 0 : (rs < p.H - p.s ? 1 : 2);
        const int cc = cs < p.W - p.w ? 0 : (cs < p.W - p.s ? 1 : 2);
        reg = rr * 3 + cc;
    }
    code = t < p.T ? ((i * (2 * p.w - 1) + j) | (reg << 16)) : 0;
}

__global__ __launch_bounds__(WA_TPB) void window_attention_kernel(WaParams p) {
    __shared__ __attribute__((aligned(16))) bf16 vs_[WA_WAVES][WA_TOK * WA_VP];
    __shared__ __attribute__((aligned(16))) float bs_[WA_WAVES][WA_NB];
    __shared__ __attribute__((aligned(16))) int pixs_[WA_WAVES][WA_TOK];
    __shared__ __attribute__((aligned(16))) int codes_[WA_WAVES][WA_TOK];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int lane = tid % WAVE;
    const int lo16 = lane & 15;
    const int hi4 = lane >> 4;
    const int pair = blockIdx.x * WA_WAVES + wave;          // wave-uniform
    if (pair >= p.pairs) return;            // no barrier below: waves never meet
    const WaPair a = wa_pair(p, pair);
    bf16* vs = vs_[wave];
    float* bs = bs_[wave];
    int* pixs = pixs_[wave];
    int* codes = codes_[wave];
    const int T = p.T;

    // ---- the token table and the head's bias column
    {
        int pix, code;
        wa_token(p, a, lane, pix, code);
        pixs[lane] = pix;
        codes[lane] = code;
        const bf16* tab = (const bf16*)p.table + a.h;
        const int nb = (2 * p.w - 1) * (2 * p.w - 1);
        for (int i = lane; i < nb; i += WAVE) bs[i] = bf2f(tab[i * p.heads]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- Q and K fragments straight from the pixels; V through LDS
    const int C3 = 3 * p.C;
    const bf16* base = (const bf16*)p.qkv + a.h * WA_D;
    const int cadd = (p.w - 1) * 2 * p.w;   // (w-1)*(2w-1) + (w-1)
    bf16x8 qf[4], kf[4];
    int qpix[4], cq[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int tok = g * 16 + lo16;
        qpix[g] = pixs[tok];
        cq[g] = codes[tok] + cadd;
        const bf16* src = base + (long)qpix[g] * C3 + hi4 * 8;
        qf[g] = load_bf16x8(src);
        kf[g] = load_bf16x8(src + p.C);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int tok = i * 16 + (lane >> 2), ch = lane & 3;
        const bf16x8 v = load_bf16x8(base + (long)pixs[tok] * C3 + 2 * p.C +
                                     ch * 8);
        *reinterpret_cast<bf16x8*>(vs + tok * WA_VP + ch * 8) = v;
    }
    // the codes of the lane's keys kt*16 + hi4*4 + e, and which are padding
    int ck[16];
    unsigned pad = 0;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        const int4 c4 = *reinterpret_cast<const int4*>(codes + kt * 16 +
                                                        hi4 * 4);
        ck[kt * 4 + 0] = c4.x;
        ck[kt * 4 + 1] = c4.y;
        ck[kt * 4 + 2] = c4.z;
        ck[kt * 4 + 3] = c4.w;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (kt * 16 + hi4 * 4 + e >= T) pad |= 1u << (kt * 4 + e);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // V^T fragments: k-slot hi4*8 + j of K-step s is key s*32 + (j >> 2)*16 +
    // hi4*4 + (j & 3), channel db*16 + lo16
    bf16x8 vf[2][2];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                vf[db][s][j] = vs[(s * 32 + (j >> 2) * 16 + hi4 * 4 +
                                   (j & 3)) * WA_VP + db * 16 + lo16];

    bf16* out = (bf16*)p.out + a.h * WA_D + hi4 * 4;
    const int G = (T + 15) >> 4;                            // live query groups
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (g >= G) break;                                  // wave-uniform
        float t[16];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = MFMA_BF16_16x16x32(kf[kt], qf[g], acc);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = kt * 4 + e;
                const int d = cq[g] - ck[i];
                float sc = fmaf(acc[e], WA_SCALE, bs[d & 0xffff]);
                if ((unsigned)d > 0xffffu) sc += -100.0f;
                t[i] = (pad >> i & 1) ? -INFINITY : sc * WA_LOG2E;
            }
        }
        float mx = t[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) mx = fmaxf(mx, t[i]);
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float l = 0.0f;
        bf16x8 pf[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float pv = __builtin_amdgcn_exp2f(t[i] - mx);
            l += pv;
            pf[i >> 3][i & 7] = f2bf(pv);
        }
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const float inv = 1.0f / l;
        const bool live = g * 16 + lo16 < T;
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
            o = MFMA_BF16_16x16x32(vf[db][0], pf[0], o);
            o = MFMA_BF16_16x16x32(vf[db][1], pf[1], o);
            bf16x4 ov;
#pragma unroll
            for (int e = 0; e < 4; ++e) ov[e] = f2bf(o[e] * inv);
            if (live)
                *reinterpret_cast<bf16x4*>(out + (long)qpix[g] * p.C +
                                           db * 16) = ov;
        }
    }
}

__global__ __launch_bounds__(WAVE) void window_attention_f32_kernel(
    WaParams p) {
    __shared__ __attribute__((aligned(16))) float ks[WA_TOK * WA_D];
    __shared__ __attribute__((aligned(16))) float vs[WA_TOK * WA_D];
    __shared__ float bs[WA_NB];
    __shared__ int pixs[WA_TOK];
    __shared__ int codes[WA_TOK];

    const int lane = threadIdx.x;           // the query token
    const WaPair a = wa_pair(p, blockIdx.x);
    const int T = p.T;
    int pix, code;
    wa_token(p, a, lane, pix, code);
    pixs[lane] = pix;
    codes[lane] = code;
    {
        const float* tab = (const float*)p.table + a.h;
        const int nb = (2 * p.w - 1) * (2 * p.w - 1);
        for (int i = lane; i < nb; i += WAVE) bs[i] = tab[i * p.heads];
    }
    __syncthreads();

    const int C3 = 3 * p.C;
    const float* base = (const float*)p.qkv + a.h * WA_D;
#pragma unroll
    for (int i = 0; i < WA_TOK * WA_D / 4 / WAVE; ++i) {
        const int id = lane + i * WAVE;
        const int tok = id >> 3, c4 = (id & 7) * 4;
        const float* src = base + (long)pixs[tok] * C3 + c4;
        *reinterpret_cast<f32x4*>(ks + tok * WA_D + c4) =
            *reinterpret_cast<const f32x4*>(src + p.C);
        *reinterpret_cast<f32x4*>(vs + tok * WA_D + c4) =
            *reinterpret_cast<const f32x4*>(src + 2 * p.C);
    }
    float q[WA_D], o[WA_D];
#pragma unroll
    for (int i = 0; i < WA_D; i += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(
            base + (long)pix * C3 + i);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            q[i + u] = v[u];
            o[i + u] = 0.0f;
        }
    }
    __syncthreads();

    const int cq = code + (p.w - 1) * 2 * p.w;
    auto score = [&](int j) {
        const float* kr = ks + j * WA_D;
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < WA_D; ++i) s = fmaf(q[i], kr[i], s);
        const int d = cq - codes[j];
        float sc = fmaf(s, WA_SCALE, bs[d & 0xffff]);
        if ((unsigned)d > 0xffffu) sc += -100.0f;
        return sc * WA_LOG2E;
    };
    float mx = -INFINITY;
    for (int j = 0; j < T; ++j) mx = fmaxf(mx, score(j));
    float l = 0.0f;
    for (int j = 0; j < T; ++j) {
        const float tt = score(j) - mx;
        // below the normal range exp2 is 0 here, whatever the denormal mode
        const float pv = tt < -126.0f ? 0.0f : exp2f(tt);
        l += pv;
        const float* vr = vs + j * WA_D;
#pragma unroll
        for (int i = 0; i < WA_D; ++i) o[i] = fmaf(pv, vr[i], o[i]);
    }
    if (lane < T) {
        float* orow = (float*)p.out + (long)pix * p.C + a.h * WA_D;
#pragma unroll
        for (int i = 0; i < WA_D; i += 4) {
            f32x4 v;
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = o[i + u] / l;
            *reinterpret_cast<f32x4*>(orow + i) = v;
        }
    }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

namespace defer_hip {

WinAttnGeom window_attention_geom(int N, int H, int W, int heads, int w) {
    WinAttnGeom g;
    g.T = w * w;
    g.groups = (g.T + 15) / 16;
    g.windows = (H / w) * (W / w);
    g.pairs = (long)N * g.windows * heads;
    g.blocks = (g.pairs + WA_WAVES - 1) / WA_WAVES;
    g.idle_waves = (int)(g.blocks * WA_WAVES - g.pairs);
    g.lds_bytes = WA_WAVES * (WA_TOK * WA_VP * 2 + WA_NB * 4 + WA_TOK * 8);
    return g;
}

void launch_window_attention(const void* qkv, const void* table, void* out,
                             int N, int H, int W, int heads, int w, int shift,
                             bool f32, hipStream_t s) {
    const WinAttnGeom g = window_attention_geom(N, H, W, heads, w);
    if (g.pairs <= 0) return;
    WaParams p{qkv, table, out, H, W, heads, heads * WA_D, w, shift, H / w,
               W / w, g.T, (int)g.pairs};
    if (f32)
        hipLaunchKernelGGL(window_attention_f32_kernel,
                           dim3((unsigned)g.pairs), dim3(WAVE), 0, s, p);
    else
        hipLaunchKernelGGL(window_attention_kernel, dim3((unsigned)g.blocks),
                           dim3(WA_TPB), 0, s, p);
}

}  // namespace defer_hip
