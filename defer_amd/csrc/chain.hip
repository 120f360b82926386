// Chained 1x1 expand + residual + act -> next block's 1x1 reduce for
// gfx950 (the ResNet bottleneck boundary add_k -> res*_conv1):
//
//   y  = act3((A[M,K1] @ W3[N1,K1]^T) * s3 + b3 + RES[M,N1])  -> bf16, global
//   a2 = act1((y[M,N1] @ W1[N2,N1]^T) * s1 + b1)              -> bf16, global
//
// y is the widest tensor of the block; the standalone conv1 launch reads
// it straight back from memory. Both convs are pointwise over pixels, so
// a tile of BM rows of y is exactly the A tile conv1 needs: this kernel
// keeps it in LDS and removes that read pass (y is still written — the
// next residual add consumes it).
//
// Deliberately a SEPARATE kernel from conv_igemm_kernel (same reasoning
// as prebn.hip). One workgroup owns BM=64 rows and the full N1 width:
//   - the A panel [64 x K1] is staged to LDS once per m-tile
//     (global_load_lds, XOR-swizzled like conv.hip); the next tile's
//     panel is issued while the current tile's a2 is stored;
//   - N1 is walked in 64-column chunks j. Per chunk: W3 rows j*64.. and
//     the W1 column slice j*64.. are staged (L2-resident); GEMM1 gives
//     acc1[64x64]; the fp32 LDS bounce of conv.hip's epilogue hands each
//     thread 8 consecutive columns of one row, which get the residual,
//     act3 and the bf16 round, go to global y AND into an LDS y-tile in
//     MFMA A-operand layout; GEMM2 accumulates acc2[64 x N2] over j;
//   - after the last chunk acc2 gets s1/b1/act1, is bounced as bf16 and
//     stored with 16-B stores.
// LDS: (K1 + K1 + N2) * 128 B + 16 KiB = 40..80 KiB -> 2-3 blocks/CU
// for the layer1/layer2 shape classes, 112..144 KiB (one block) for the
// layer3 ones.
//
// Loads are issued ahead of their use: the residual chunk RES(j+1) — the
// HBM-bound stream — right after the W1(j) stage, a whole chunk early
// (epilogue 1 waits vmcnt(2), so exactly those two loads stay in
// flight); W1(j) before GEMM1(j); W3(j+1) before GEMM2(j); the next A
// panel under the a2 store phase. Every global_load_lds sits after the
// last LDS write of its phase: the compiler drains pending LDS DMA in
// front of LDS stores. Co-resident blocks cover the rest.
//
// Bit-identity: GEMM1 accumulates k ascending with the igemm 16x16x32
// fragment mapping and the same epilogue expression; GEMM2 consumes the
// bf16-rounded y, j ascending and k ascending inside a chunk — the same
// per-element order as a standalone GEMM-mode launch. Both outputs match
// the two-launch path bit for bit (tests/test_conv_chain_gpu.py).
#include "common.h"
#include "kernels.h"

#define CH_BM 64
#define CH_TPB 256
#define CH_SCR (32 * 64 * 2)        // fp32 bounce, 32 rows, in bf16 units
#define CH_YT (64 * 64)             // y-tile, bf16 units

__device__ __forceinline__ int ch_swz(int row, int k8) {
    return k8 ^ (row & 7);
}

__device__ __forceinline__ void ch_glds16(const bf16* src, bf16* lds_base) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)lds_base,
        16, 0, 0);
}

template <int K1, int N2, int WPS>
__global__ __launch_bounds__(CH_TPB, WPS) void conv1x1_chain_kernel(
    const bf16* __restrict__ X,      // [M][K1]
    const bf16* __restrict__ W3,     // [N1][K1]
    const float* __restrict__ S3,    // [N1]
    const float* __restrict__ B3,    // [N1]
    const bf16* __restrict__ RES,    // [M][N1]
    bf16* __restrict__ Y,            // [M][N1]
    const bf16* __restrict__ W1,     // [N2][N1]
    const float* __restrict__ S1,    // [N2]
    const float* __restrict__ B1,    // [N2]
    bf16* __restrict__ A2,           // [M][N2]
    int M, int N1, int act3, int act1) {
    constexpr int NK1 = K1 / 64;             // k-tiles of GEMM1
    constexpr int NT2 = N2 / 64;             // 64-row tiles of the W1 slice
    constexpr int WN2 = N2 / 2;              // GEMM2 wave n-width
    constexpr int NI2 = WN2 / 16;
    constexpr int OST = N2 + 8;              // bf16 out-bounce row stride

    __shared__ __attribute__((aligned(16)))
    bf16 lds[CH_BM * K1 + 64 * K1 + N2 * 64 + CH_SCR + CH_YT];
    bf16* Ap = lds;                          // NK1 tiles [64][64]
    bf16* W3b = Ap + CH_BM * K1;             // NK1 tiles [64 n][64 k]
    bf16* W1b = W3b + 64 * K1;               // [N2][64]
    float* scratch = (float*)(W1b + N2 * 64);
    bf16* ytile = W1b + N2 * 64 + CH_SCR;
    bf16* obuf = W1b;                        // epilogue 2: W1b..ytile end

    const int tid = threadIdx.x;
    const int wave = tid / WAVE;
    const int lane = tid % WAVE;
    const int wm = wave >> 1;                // 32-row slab
    const int wn = wave & 1;
    const int lo16 = lane & 15;
    const int hi4 = lane >> 4;
    const int mtiles = (M + CH_BM - 1) / CH_BM;
    const int NJ = N1 / 64;

    // staging geometry of one [64][64] tile: 2 chunks of 16 B per thread
    int t_row[2], t_k8[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int chunk = wave * 128 + i * 64 + lane;
        t_row[i] = chunk / 8;
        t_k8[i] = ch_swz(t_row[i], chunk % 8);
    }
    auto stage_a = [&](int mt) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int m = mt * CH_BM + t_row[i];
            if (m >= M) m = M - 1;           // clamped rows are never stored
            const bf16* src = X + (long)m * K1 + t_k8[i] * 8;
#pragma unroll
            for (int kt = 0; kt < NK1; ++kt)
                ch_glds16(src + kt * 64,
                          Ap + kt * 4096 + (wave * 128 + i * 64) * 8);
        }
    };
    auto stage_w3 = [&](int j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bf16* src =
                W3 + (long)(j * 64 + t_row[i]) * K1 + t_k8[i] * 8;
#pragma unroll
            for (int kt = 0; kt < NK1; ++kt)
                ch_glds16(src + kt * 64,
                          W3b + kt * 4096 + (wave * 128 + i * 64) * 8);
        }
    };
    auto stage_w1 = [&](int j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bf16* src =
                W1 + (long)t_row[i] * N1 + j * 64 + t_k8[i] * 8;
#pragma unroll
            for (int t = 0; t < NT2; ++t)
                ch_glds16(src + (long)t * 64 * N1,
                          W1b + t * 4096 + (wave * 128 + i * 64) * 8);
        }
    };

    float sc1[NI2], bi1[NI2];
#pragma unroll
    for (int ni = 0; ni < NI2; ++ni) {
        int n = wn * WN2 + ni * 16 + lo16;
        sc1[ni] = S1[n];
        bi1[ni] = B1[n];
    }

    // epilogue-1 chunk geometry: one 8-column chunk per thread per round
    const int e_rl = tid >> 3;               // round-local row 0..31
    const int e_c8 = (tid & 7) * 8;
    const int e_cs = e_c8 ^ (((e_rl >> 2) & 3) << 4);

    int mt = blockIdx.x;
    if (mt >= mtiles) return;
    stage_a(mt);
    stage_w3(0);
    float sc3n[2], bi3n[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        int n = wn * 32 + ni * 16 + lo16;
        sc3n[ni] = S3[n];
        bi3n[ni] = B3[n];
    }

    // residual chunk (rows m0.., columns j*64..) of this thread's two
    // epilogue-1 rounds; rows past M are clamped and never stored
    auto res_load = [&](bf16x8* rv, int m0, int j) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int m = m0 + h * 32 + e_rl;
            if (m >= M) m = M - 1;
            rv[h] = load_bf16x8(RES + (long)m * N1 + j * 64 + e_c8);
        }
    };
    bf16x8 rvn[2];
    res_load(rvn, mt * CH_BM, 0);

    for (; mt < mtiles; mt += gridDim.x) {
        const int m0 = mt * CH_BM;
        const bool more = mt + (int)gridDim.x < mtiles;
        f32x4 acc2[2][NI2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI2; ++ni)
                acc2[mi][ni] = {0.f, 0.f, 0.f, 0.f};

        for (int j = 0; j < NJ; ++j) {
            // A panel + W3(j) landed; every wave is past GEMM2(j-1) (or
            // the previous tile's out-bounce), so W1b / ytile are free
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const int jn = j + 1 < NJ ? j + 1 : 0;
            // s3/b3 and the residual run one chunk ahead (wrapping to
            // chunk 0 of the next tile): the residual is the HBM stream,
            // and a whole chunk of work covers its latency
            float sc3[2], bi3[2];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                sc3[ni] = sc3n[ni];
                bi3[ni] = bi3n[ni];
                int n = jn * 64 + wn * 32 + ni * 16 + lo16;
                sc3n[ni] = S3[n];
                bi3n[ni] = B3[n];
            }
            bf16x8 rv[2];
            rv[0] = rvn[0];
            rv[1] = rvn[1];
            stage_w1(j);
            // exactly two loads, unconditionally, AFTER the W1 stage: the
            // counted wait in front of epilogue 1 lets them stay in flight
            res_load(rvn, (j + 1 < NJ || !more) ? m0 : m0 + (int)gridDim.x
                                                          * CH_BM, jn);

            // ---- GEMM1: acc1[64x64] = Apanel @ W3_j^T (igemm mapping)
            f32x4 acc1[2][2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    acc1[mi][ni] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kt = 0; kt < NK1; ++kt)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    bf16x8 af[2], bfr[2];
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi) {
                        int row = wm * 32 + mi * 16 + lo16;
                        af[mi] = *reinterpret_cast<bf16x8*>(
                            Ap + kt * 4096 + row * 64
                               + ch_swz(row, ks * 4 + hi4) * 8);
                    }
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) {
                        int row = wn * 32 + ni * 16 + lo16;
                        bfr[ni] = *reinterpret_cast<bf16x8*>(
                            W3b + kt * 4096 + row * 64
                                + ch_swz(row, ks * 4 + hi4) * 8);
                    }
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni)
                            acc1[mi][ni] = MFMA_BF16_16x16x32(
                                af[mi], bfr[ni], acc1[mi][ni]);
                }
            // W1(j) landed; only the two residual loads for the next
            // chunk, issued after it, may stay in flight. A panel and W3b
            // are free after the barrier
            asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();

            // ---- epilogue 1: two 32-row rounds through the fp32 bounce
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (wm == h) {
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                int rl = mi * 16 + hi4 * 4 + e;
                                int c = wn * 32 + ni * 16 + lo16;
                                int cs = c ^ (((rl >> 2) & 3) << 4);
                                scratch[rl * 64 + cs] =
                                    acc1[mi][ni][e] * sc3[ni] + bi3[ni];
                            }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                f32x4 v0 = *reinterpret_cast<f32x4*>(
                    scratch + e_rl * 64 + e_cs);
                f32x4 v1 = *reinterpret_cast<f32x4*>(
                    scratch + e_rl * 64 + e_cs + 4);
                bf16x8 o;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    float v = q < 4 ? v0[q] : v1[q - 4];
                    v += bf2f(rv[h][q]);
                    o[q] = f2bf(apply_act(v, act3));
                }
                const int r = h * 32 + e_rl;
                if (m0 + r < M)
                    store_bf16x8(Y + (long)(m0 + r) * N1 + j * 64 + e_c8, o);
                // same 8 columns = one 16-B chunk of the A-operand layout
                store_bf16x8(ytile + r * 64 + ch_swz(r, tid & 7) * 8, o);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            }
            // next chunk's W3 (wraps to W3(0) of the next tile). Issued
            // AFTER the chunk's last LDS write: the compiler drains
            // pending LDS DMA before any ds_write, so staging earlier
            // would only stall the bounce. GEMM2 (LDS reads only) is its
            // latency cover.
            if (j + 1 < NJ || more) stage_w3(jn);

            // ---- GEMM2: acc2[64 x N2] += ytile @ W1_j^T
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 af[2];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    int row = wm * 32 + mi * 16 + lo16;
                    af[mi] = *reinterpret_cast<bf16x8*>(
                        ytile + row * 64 + ch_swz(row, ks * 4 + hi4) * 8);
                }
#pragma unroll
                for (int ni = 0; ni < NI2; ++ni) {
                    int row = wn * WN2 + ni * 16 + lo16;
                    bf16x8 bfr = *reinterpret_cast<bf16x8*>(
                        W1b + row * 64 + ch_swz(row, ks * 4 + hi4) * 8);
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
                        acc2[mi][ni] = MFMA_BF16_16x16x32(af[mi], bfr,
                                                          acc2[mi][ni]);
                }
            }
        }

        // ---- epilogue 2: s1/b1 + act1 on the accumulator, bf16 bounce
        // (padded rows: the four hi4 groups land 16 banks apart)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();        // W1b/scratch/ytile are free
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI2; ++ni)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int r = wm * 32 + mi * 16 + hi4 * 4 + e;
                    int c = wn * WN2 + ni * 16 + lo16;
                    float v = acc2[mi][ni][e] * sc1[ni] + bi1[ni];
                    obuf[r * OST + c] = f2bf(apply_act(v, act1));
                }
        // next tile's A panel: after the last LDS write of this tile
        // (see the W3 note), under the out-bounce reads and a2 stores
        if (more) stage_a(mt + gridDim.x);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int i = 0; i < N2 / 32; ++i) {
            int chunk = tid + i * CH_TPB;
            int r = chunk / (N2 / 8);
            int c8 = (chunk % (N2 / 8)) * 8;
            bf16x8 o = load_bf16x8(obuf + r * OST + c8);
            if (m0 + r < M)
                store_bf16x8(A2 + (long)(m0 + r) * N2 + c8, o);
        }
        // the next chunk's top barrier orders these reads before W1b is
        // refilled
    }
    // no LDS DMA may outlive the block (the last chunk stages nothing;
    // this documents the invariant)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

namespace defer_hip {

namespace {

// Shape classes where the fused kernel measured faster than the two
// launches (tools/chainbench.py, MI355X, batch 256 / batch 64; the gain
// must exceed the spread of the repeats). Everything else stays on two
// launches unless forced.
struct ChainWin { int K1, N1, N2; };
const ChainWin kChainWins[] = {
    // fused vs two launches, us, min..max of 3 repeats, batch 256 | 64
    {64, 256, 64},     // 202..231 vs 355..359 | 47..48 vs 78..79
    {64, 256, 128},    // 236..274 vs 438..448 | 65..66 vs 101..102
    {128, 512, 128},   // 129..132 vs 257..258 | 35..35 vs 56..56
    {128, 512, 256},   // 158..161 vs 313..313 | 43..44 vs 73..73
    {256, 1024, 256},  // 135..136 vs 147..147 | 36..36 vs 42..43
    // measured, not adopted (1 block/CU):
    // {256, 1024, 512}   210..212 vs 212..212 | 55..55 vs 54..55
};

bool chain_policy(int K1, int N1, int N2) {
    for (const ChainWin& w : kChainWins)
        if (w.K1 == K1 && w.N1 == N1 && w.N2 == N2) return true;
    return false;
}

}  // namespace

bool launch_conv1x1_chain(const void* x, const void* w3, const float* s3,
                          const float* b3, const void* res, void* y,
                          bool relu3, const void* w1, const float* s1,
                          const float* b1, void* a2, bool relu1, int M,
                          int K1, int N1, int N2, bool force,
                          int max_blocks, hipStream_t s) {
    if (M <= 0 || N1 < 64 || N1 % 64 != 0) return false;
    if (!force && !chain_policy(K1, N1, N2)) return false;
    const int mtiles = (M + CH_BM - 1) / CH_BM;
    const int a3 = relu3 ? ACT_RELU : ACT_NONE;
    const int a1 = relu1 ? ACT_RELU : ACT_NONE;
#define CHAIN(K1v, N2v, WPSv)                                             \
    do {                                                                  \
        int gx = 256 * WPSv;                                              \
        if (max_blocks > 0) gx = max_blocks;                              \
        if (gx > mtiles) gx = mtiles;                                     \
        hipLaunchKernelGGL((conv1x1_chain_kernel<K1v, N2v, WPSv>),        \
                           dim3(gx), dim3(CH_TPB), 0, s, (const bf16*)x,  \
                           (const bf16*)w3, s3, b3, (const bf16*)res,     \
                           (bf16*)y, (const bf16*)w1, s1, b1, (bf16*)a2,  \
                           M, N1, a3, a1);                                \
        return true;                                                      \
    } while (0)
    if (K1 == 64 && N2 == 64) CHAIN(64, 64, 3);
    if (K1 == 64 && N2 == 128) CHAIN(64, 128, 3);
    if (K1 == 128 && N2 == 128) CHAIN(128, 128, 2);
    if (K1 == 128 && N2 == 256) CHAIN(128, 256, 2);
    if (K1 == 256 && N2 == 256) CHAIN(256, 256, 1);
    if (K1 == 256 && N2 == 512) CHAIN(256, 512, 1);
#undef CHAIN
    return false;
}

}  // namespace defer_hip
