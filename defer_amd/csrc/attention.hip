// Fused multi-head attention for gfx950: softmax(Q K^T / sqrt(D)) V in one
// kernel, bf16 on the MFMA and a plain fp32 kernel. qkv is [N][T][3][heads][D]
// (what one fused QKV linear writes), out is [N][T][heads][D], D = 64:
//
//   out[n][t][h][:] = sum_j P[n][h][t][j] * v[n][j][h][:]
//   P[n][h][t][:]   = softmax_j((q[n][t][h][:] . k[n][j][h][:]) * 0.125)
//
// q, k and v are read in place with row stride 3C; the score matrix and P
// never leave the CU. Non-causal, no mask, no dropout.
//
// bf16 kernel (attention_kernel<NQ>)
// ----------------------------------
// Split: a workgroup of 4 waves serves one (image, head, block of query
// rows). The query rows are cut into groups of 16 (G = ceil(T / 16)); a wave
// owns NQ groups for the whole kernel (NQ = 1 for G <= 4, else 2), wave w of
// a block the groups w and w + 4. A block takes gpb = ceil(G / nblk) groups
// with nblk = ceil(G / (4 * NQ)), so the blocks of a head are balanced:
// T = 197 is 13 groups in two blocks of 7 and 6, not 4 + 4 + 4 + 1
// (attention_geom, a pure function of T). A wave keeps its Q fragments in
// registers: Q is read from global memory once.
//
// K and V: tiles of 64 keys x 64 channels (8 KB each) through LDS, staged by
// global_load_lds, 16 B per lane, four per lane and tile. Two buffers each
// (32 KB): at the top of tile j every wave waits for its own loads
// (s_waitcnt vmcnt(0): tile j was issued a whole tile ago, nothing else is in
// flight) and meets the others at one s_barrier, after which tile j is
// complete and the other buffer is free; tile j + 1 is issued into it and is
// in flight while tile j is consumed. Keys >= T stage row T - 1 again, never
// anything beyond the tensor; their scores are masked and their p is 0.
//
// Scores, transposed: S^T = K Q^T on v_mfma_f32_16x16x32_bf16 with K as the
// M operand, two K-steps over D = 64. A lane (lo16, hi4) then holds, for the
// one query lo16, the keys kt*16 + hi4*4 + e (e < 4) of each 16-key
// subtile kt: 16 scores of one query per lane, so the row max is 15 max in
// the lane and two xor-shuffles (lanes ^16, ^32), and m, l and the rescale
// factor are per lane with no further traffic.
//
// Online softmax, fp32: t = s * (0.125 * log2 e); keys >= T get -inf (only
// the last tile has any, and it has at least one live key, so no max is
// -inf); m' = max(m, rowmax t); p = exp2(t - m'); O and l are scaled by
// exp2(m - m'); l sums the fp32 p (per lane, the four hi4 partial sums are
// added once at the end).
//
// P stays in registers. O^T = V^T P^T: P^T is the N operand, whose lane
// (lo16, hi4) wants 8 consecutive k of column lo16. The lane's p of subtiles
// 2s and 2s + 1, rounded to bf16 (nearest even), are exactly that if k-slot
// hi4*8 + j of K-step s stands for the key
//     s*32 + (j >> 2)*16 + hi4*4 + (j & 3).
// The order of keys inside a dot product is free as long as both operands
// agree, so the V^T fragments are gathered in this order: lane (lo16, hi4)
// of fragment (db, s) reads V[key(s, hi4, j)][db*16 + lo16] for j < 8 with
// 2-byte LDS reads. (gfx950's transposing ds_read_b64_tr_b16 would fetch the
// same fragment in two reads; the 2-byte gather is the form that could be
// checked against the documented operand layout without a device, and the
// fragments are shared by both query groups of a wave.) The result lane holds
// O^T[db*16 + hi4*4 + e][query lo16]: the lane's own query again, so the
// rescale is a per-lane multiply.
//
// LDS rows are 128 B, chunk = 16 B. K chunk c of row r sits at c ^ (r >> 1
// & 7): the 16 lanes of a ds_read_b128 (16 rows, one logical chunk) cover
// the 64 banks once. V chunk c of row r sits at c ^ 2*(r >> 2 & 3): the four
// hi4 groups of a 2-byte gather (rows 4 apart, the same two chunks) land in
// four different chunk pairs. global_load_lds writes lane-linear, so the
// swizzle is applied on the source side.
//
// Epilogue: l summed over hi4, O * (1 / l), one rounding to bf16, 8-byte
// writes into a 2 KB per-wave slab of the (finished) K buffers, 16-byte
// stores of out rows; query rows >= T are not stored.
//
// Order: key tiles 0, 1, .. for every row, the hardware's fixed order inside
// an MFMA, no atomics: run-to-run identical.
//
// fp32 kernel (attention_f32_kernel): 64 query rows per workgroup, four
// lanes per row, each with 16 of the 64 channels of q and O. K and V tiles of
// 64 keys in LDS (plain loads, one buffer). Per key: 16 fmaf, two
// xor-shuffles (the four lanes get the same bits), and the online softmax
// step with the same t, m, p and rescale as above, per key instead of per
// tile; O / l at the end. Plain and deterministic; no throughput is claimed.
#include "common.h"
#include "kernels.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

constexpr int AT_TPB = 256;
constexpr int AT_D = 64;                    // head dim
constexpr int AT_KT = 64;                   // keys per tile
constexpr int AT_TILE = AT_KT * AT_D;       // bf16 per staged tile
// softmax in base 2: exp(s * 0.125) = exp2(s * AT_C)
constexpr float AT_C = 0.125f * 1.4426950408889634f;

__device__ __forceinline__ void at_glds16(const bf16* src, bf16* lds_base) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)lds_base, 16, 0,
        0);
}

struct AtParams {
    const bf16* qkv;
    bf16* out;
    int T, heads, C, nblk, gpb;
};

template <int NQ>
__global__ __launch_bounds__(AT_TPB) void attention_kernel(AtParams p) {
    // K buffers 0 and 1, then V buffers 0 and 1
    __shared__ __attribute__((aligned(16))) bf16 lds[4 * AT_TILE];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int lane = tid % WAVE;
    const int lo16 = lane & 15;
    const int hi4 = lane >> 4;
    int bx = blockIdx.x;
    const int blk = bx % p.nblk;
    bx /= p.nblk;
    const int h = bx % p.heads;
    const int n = bx / p.heads;
    const int C3 = 3 * p.C;
    const int T = p.T;
    // q of row 0 of this image and head; k is C and v 2C further on
    const bf16* base = p.qkv + (long)n * T * C3 + h * AT_D;

    // ---- staging: piece i of this wave is the 64 chunks from (i*4 + wave)
    // * 64, one per lane, lane-linear in LDS; the lane picks the source chunk
    // that the swizzle puts there
    auto stage = [&](int tile, int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int piece = (i * 4 + wave) * 64;          // wave-uniform
            const int ch = piece + lane;
            const int r = ch >> 3, pc = ch & 7;
            // keys >= T stage row T - 1: inside the tensor, masked below
            const int key = min(tile * AT_KT + r, T - 1);
            const bf16* row = base + key * C3;
            const int kc = pc ^ ((r >> 1) & 7);
            const int vc = pc ^ (((r >> 2) & 3) * 2);
            at_glds16(row + p.C + kc * 8, lds + buf * AT_TILE + piece * 8);
            at_glds16(row + 2 * p.C + vc * 8,
                      lds + (2 + buf) * AT_TILE + piece * 8);
        }
    };
    stage(0, 0);

    // ---- this wave's query groups and their Q fragments (N operand of S^T:
    // lane (lo16, hi4) holds q[row lo16][s*32 + hi4*8 ..]). Rows >= T read
    // row T - 1; they are computed and not stored.
    int g[NQ];
    bool live[NQ];
    bf16x8 qf[NQ][2];
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
        g[qi] = blk * p.gpb + wave + 4 * qi;
        live[qi] = wave + 4 * qi < p.gpb && g[qi] * 16 < T;  // wave-uniform
        const int row = min(g[qi] * 16 + lo16, T - 1);
#pragma unroll
        for (int s = 0; s < 2; ++s)
            qf[qi][s] = load_bf16x8(base + row * C3 + s * 32 + hi4 * 8);
    }

    // ---- the lane's places in a tile
    // K: row kt*16 + lo16, logical chunk s*4 + hi4
    int koff[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
        koff[s] = lo16 * AT_D + (((s * 4 + hi4) ^ (lo16 >> 1)) * 8);
    // V: row s*32 + (j >> 2)*16 + hi4*4 + (j & 3), channel db*16 + lo16
    int voff[4];
#pragma unroll
    for (int db = 0; db < 4; ++db)
        voff[db] = hi4 * 4 * AT_D +
                   (((db * 2 + (lo16 >> 3)) ^ (hi4 * 2)) * 8) + (lo16 & 7);

    f32x4 o[NQ][4];
    float m[NQ], l[NQ];
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
        m[qi] = -INFINITY;
        l[qi] = 0.0f;
#pragma unroll
        for (int db = 0; db < 4; ++db) o[qi][db] = {0.f, 0.f, 0.f, 0.f};
    }

    const int ntiles = (T + AT_KT - 1) / AT_KT;
    for (int j = 0; j < ntiles; ++j) {
        const int buf = j & 1;
        // the one wait of a tile: this wave's loads of tile j have landed,
        // and past the barrier everyone's have and everyone is done with
        // tile j - 1, whose buffers are refilled next
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (j + 1 < ntiles) stage(j + 1, buf ^ 1);

        const bf16* KB = lds + buf * AT_TILE;
        const bf16* VB = lds + (2 + buf) * AT_TILE;
        bf16x8 kf[4][2];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                kf[kt][s] = *reinterpret_cast<const bf16x8*>(
                    KB + kt * 16 * AT_D + koff[s]);
        bf16x8 vf[4][2];
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    vf[db][s][e] = VB[(s * 32 + (e >> 2) * 16 + (e & 3)) *
                                          AT_D + voff[db]];
        const bool tail = (j + 1) * AT_KT > T;              // uniform

#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
            if (!live[qi]) continue;
            float t[16];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = MFMA_BF16_16x16x32(kf[kt][0], qf[qi][0], acc);
                acc = MFMA_BF16_16x16x32(kf[kt][1], qf[qi][1], acc);
#pragma unroll
                for (int e = 0; e < 4; ++e) t[kt * 4 + e] = acc[e] * AT_C;
            }
            if (tail) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = j * AT_KT + (i >> 2) * 16 + hi4 * 4 +
                                    (i & 3);
                    if (key >= T) t[i] = -INFINITY;
                }
            }
            float mx = t[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) mx = fmaxf(mx, t[i]);
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mn = fmaxf(m[qi], mx);
            const float alpha = __builtin_amdgcn_exp2f(m[qi] - mn);
            m[qi] = mn;
            float sum = 0.0f;
            bf16x8 pf[2];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float pv = __builtin_amdgcn_exp2f(t[i] - mn);
                sum += pv;
                pf[i >> 3][i & 7] = f2bf(pv);
            }
            l[qi] = l[qi] * alpha + sum;
#pragma unroll
            for (int db = 0; db < 4; ++db) {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[qi][db][e] *= alpha;
                o[qi][db] = MFMA_BF16_16x16x32(vf[db][0], pf[0], o[qi][db]);
                o[qi][db] = MFMA_BF16_16x16x32(vf[db][1], pf[1], o[qi][db]);
            }
        }
    }

    // ---- epilogue: every wave is done with the last tile, then each wave
    // bounces its groups through its own 16 x 64 slab of the K buffers
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    bf16* slab = lds + wave * 16 * AT_D;
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
        if (!live[qi]) continue;
        float ls = l[qi];
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        const float inv = 1.0f / ls;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            bf16x4 ov;
#pragma unroll
            for (int e = 0; e < 4; ++e) ov[e] = f2bf(o[qi][db][e] * inv);
            const int c = db * 2 + (hi4 >> 1);
            *reinterpret_cast<bf16x4*>(
                slab + lo16 * AT_D + ((c ^ (lo16 & 7)) * 8) + (hi4 & 1) * 4) =
                ov;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = lane + i * WAVE;
            const int row = id >> 3, c = id & 7;
            const int tq = g[qi] * 16 + row;
            const bf16x8 v = *reinterpret_cast<const bf16x8*>(
                slab + row * AT_D + ((c ^ (row & 7)) * 8));
            if (tq < T)
                store_bf16x8(p.out + ((long)n * T + tq) * p.C + h * AT_D +
                                 c * 8, v);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

constexpr int AF_ROWS = 64;                 // query rows of a workgroup

__global__ __launch_bounds__(AT_TPB) void attention_f32_kernel(
    const float* __restrict__ qkv, float* __restrict__ out, int T, int heads,
    int C, int nqb) {
    __shared__ __attribute__((aligned(16))) float ks[AT_KT * AT_D];
    __shared__ __attribute__((aligned(16))) float vs[AT_KT * AT_D];

    const int tid = threadIdx.x;
    int bx = blockIdx.x;
    const int qb = bx % nqb;
    bx /= nqb;
    const int h = bx % heads;
    const int n = bx / heads;
    const int C3 = 3 * C;
    const float* base = qkv + (long)n * T * C3 + h * AT_D;
    const int part = tid & 3;                   // 16-channel quarter
    const int tq = qb * AF_ROWS + (tid >> 2);   // query row
    const float* qrow = base + min(tq, T - 1) * C3 + part * 16;

    float q[16], o[16];
#pragma unroll
    for (int i = 0; i < 16; i += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(qrow + i);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            q[i + u] = v[u];
            o[i + u] = 0.0f;
        }
    }
    float m = -INFINITY, l = 0.0f;

    for (int k0 = 0; k0 < T; k0 += AT_KT) {
        __syncthreads();                        // the last tile is consumed
#pragma unroll
        for (int i = 0; i < AT_KT * AT_D / 4 / AT_TPB; ++i) {
            const int id = tid + i * AT_TPB;
            const int r = id >> 4, c4 = (id & 15) * 4;
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (k0 + r < T) {
                const float* row = base + (k0 + r) * C3 + c4;
                kv = *reinterpret_cast<const f32x4*>(row + C);
                vv = *reinterpret_cast<const f32x4*>(row + 2 * C);
            }
            *reinterpret_cast<f32x4*>(ks + r * AT_D + c4) = kv;
            *reinterpret_cast<f32x4*>(vs + r * AT_D + c4) = vv;
        }
        __syncthreads();
        const int kn = min(AT_KT, T - k0);      // live keys of the tile
        for (int j = 0; j < kn; ++j) {
            const float* kr = ks + j * AT_D + part * 16;
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < 16; ++i) s = fmaf(q[i], kr[i], s);
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            const float t = s * AT_C;
            const float mn = fmaxf(m, t);
            const float alpha = exp2f(m - mn);
            const float pv = exp2f(t - mn);
            m = mn;
            l = l * alpha + pv;
            const float* vr = vs + j * AT_D + part * 16;
#pragma unroll
            for (int i = 0; i < 16; ++i) o[i] = fmaf(pv, vr[i], o[i] * alpha);
        }
    }
    if (tq < T) {
        float* orow = out + ((long)n * T + tq) * C + h * AT_D + part * 16;
#pragma unroll
        for (int i = 0; i < 16; i += 4) {
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

AttnGeom attention_geom(int T) {
    AttnGeom a;
    a.G = (T + 15) / 16;
    a.NQ = a.G <= 4 ? 1 : 2;
    a.nblk = (a.G + 4 * a.NQ - 1) / (4 * a.NQ);
    a.gpb = (a.G + a.nblk - 1) / a.nblk;
    a.lds_bytes = 4 * AT_TILE * 2;
    return a;
}

void launch_attention(const void* qkv, void* out, int N, int T, int heads,
                      bool f32, hipStream_t s) {
    if (N <= 0 || T <= 0 || heads <= 0) return;
    const int C = heads * AT_D;
    if (f32) {
        const int nqb = (T + AF_ROWS - 1) / AF_ROWS;
        hipLaunchKernelGGL(attention_f32_kernel,
                           dim3((unsigned)((long)N * heads * nqb)),
                           dim3(AT_TPB), 0, s, (const float*)qkv, (float*)out,
                           T, heads, C, nqb);
        return;
    }
    const AttnGeom a = attention_geom(T);
    AtParams p{(const bf16*)qkv, (bf16*)out, T, heads, C, a.nblk, a.gpb};
    const dim3 grid((unsigned)((long)N * heads * a.nblk));
    if (a.NQ == 1)
        hipLaunchKernelGGL(attention_kernel<1>, grid, dim3(AT_TPB), 0, s, p);
    else
        hipLaunchKernelGGL(attention_kernel<2>, grid, dim3(AT_TPB), 0, s, p);
}

}  // namespace defer_hip
