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
// of four waves for the layer1/layer2 shape classes. The layer3 classes
// (K1 = 256: 120 / 152 KiB, one block per CU) run the same phases with
// EIGHT waves, so that every SIMD still holds two (NW = 8, "DEEP" below):
// GEMM1 and GEMM2 split 2 x 4 over the waves, epilogue 1 is one 64-row
// round that all eight waves write (16 KiB bounce), and the barrier
// after GEMM1 is folded into the bounce's own, three per chunk. Where the
// K1 = 256, N2 = 256 class has more than one round of 64-row tiles per CU it
// runs 128-row tiles instead (BM = 128, chain_tile128 below), which stage
// the weights half as often per row.
//
// Loads are issued ahead of their use: the residual chunk RES(j+1) — the
// HBM-bound stream — right after the W1(j) stage, a whole chunk early
// (epilogue 1 waits vmcnt(2), so exactly those two loads stay in
// flight; one load and vmcnt(1) with eight waves); W1(j) before GEMM1(j); W3(j+1) before GEMM2(j); the next A
// panel under the a2 store phase. Every global_load_lds sits after the
// last LDS write of its phase: the compiler drains pending LDS DMA in
// front of LDS stores. Co-resident blocks cover the rest.
//
// PROJ (K1 = 64, N2 = 64, four waves): the residual is not a tensor but the
// block's 1x1 projection shortcut, RES = bf16((XP[M,64] @ WP[N1,64]^T) * sp
// + bp), which the kernel makes per chunk: a third GEMM of GEMM1's size on
// the same fragment mapping, so a lane holds acc1 and the shortcut for the
// same (row, column) and adds them in front of the bounce. Its operands go
// from global straight to registers (XP fragments once per tile, issued
// under the a2 stores; WP fragments, sp and bp a chunk ahead); nothing of
// it touches LDS. With no residual stream to wait behind, W1(j+1) is staged
// together with W3(j+1) into a second W1 slice (48 KiB, still three blocks
// a CU), and a chunk waits for memory once, at its top.
//
// Bit-identity: GEMM1 accumulates k ascending with the igemm 16x16x32
// fragment mapping and the same epilogue expression; GEMM2 consumes the
// bf16-rounded y, j ascending and k ascending inside a chunk — the same
// per-element order as a standalone GEMM-mode launch. Both outputs match
// the two-launch path bit for bit (tests/test_conv_chain_gpu.py). PROJ's
// shortcut is one k-tile, ks ascending, then acc * sp + bp rounded to bf16,
// as the projection's own GEMM-mode launch stores it, and it enters y by
// the same fp32 add as a loaded residual
// (tests/test_conv_chain_proj_gpu.py).
#include "common.h"
#include "kernels.h"

#define CH_BM 64
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

// The 128-row tile of the K1 = 256 classes (eight waves, one block per CU).
// A chunk stages the same 64 KiB of W3 and W1 as the 64-row tile does, for
// twice the rows, so the weight stream through LDS per output row is halved.
//   - waves are 4 row slabs of 32 x 2 across n: GEMM1 32 x 32 per wave and
//     chunk, GEMM2 32 x N2/2;
//   - the A panel [128 x K1] is staged to LDS once per tile like the 64-row
//     one; the next tile's is issued with W3(0) in the last chunk, under its
//     GEMM2 (the panel is free once every wave is past the last GEMM1).
//     Held in registers instead (64 a lane, loaded in the GEMM1 mapping as
//     PROJ's XP is) it did not fit: with acc2 (64), acc1 and the look-ahead
//     sets the kernel needed 256 registers and spilled 10 to 15, and the
//     reloads, which count on vmcnt, drained the W1 stage inside GEMM1;
//   - epilogue 1 is two 64-row rounds through the 16 KiB bounce (two
//     residual loads a thread stay in flight, vmcnt(2)); epilogue 2 is two
//     64-row rounds through the bounce and the y-tile (32 KiB, rows of N2
//     bf16 with the 16-B chunk index XORed by the row group, in place of
//     the padded stride that would not fit), clear of both weight slices.
// LDS: A panel 64 KiB + W3 chunk 32 KiB + W1 slice 32 KiB + bounce 16 KiB +
// y-tile 16 KiB = 160 KiB, all a CU has: no second weight slice. Fragment
// mapping, accumulation order (k ascending; j, then k) and epilogue
// expressions are the 64-row tile's: both outputs are bit-identical to it
// and to the two launches (tests/test_conv_chain_bm128_gpu.py).
template <int K1, int N2>
__device__ __forceinline__ void chain_tile128(
    const bf16* __restrict__ X, const bf16* __restrict__ W3,
    const float* __restrict__ S3, const float* __restrict__ B3,
    const bf16* __restrict__ RES, bf16* __restrict__ Y,
    const bf16* __restrict__ W1, const float* __restrict__ S1,
    const float* __restrict__ B1, bf16* __restrict__ A2,
    int M, int N1, int act3, int act1) {
    constexpr int BM = 128;
    constexpr int TPB = 8 * WAVE;
    constexpr int NK1 = K1 / 64;             // k-tiles of the W3 chunk
    constexpr int NT2 = N2 / 64;             // 64-row tiles of the W1 slice
    constexpr int WN2 = N2 / 2;              // GEMM2 wave n-width
    constexpr int NI2 = WN2 / 16;
    constexpr int ER = 64;                   // rows per epilogue round
    constexpr int NR = BM / ER;
    constexpr int SCR = ER * 64 * 2;         // fp32 bounce, in bf16 units
    constexpr int YT = BM * 64;              // y-tile, bf16 units
    static_assert(ER * N2 <= SCR + YT, "out-bounce fits");
    static_assert(N2 * 8 % TPB == 0, "whole out-bounce chunks per thread");

    __shared__ __attribute__((aligned(16)))
    bf16 lds[BM * K1 + 64 * K1 + N2 * 64 + SCR + YT];
    static_assert(sizeof(lds) <= 163840, "one block's LDS");
    bf16* Ap = lds;                          // NK1 tiles [128][64]
    bf16* W3b = Ap + BM * K1;                // NK1 tiles [64 n][64 k]
    bf16* W1b = W3b + 64 * K1;               // NT2 tiles [64 n][64 k]
    float* scratch = (float*)(W1b + N2 * 64);
    bf16* ytile = W1b + N2 * 64 + SCR;       // [128][64]
    bf16* obuf = (bf16*)scratch;             // epilogue 2: scratch + ytile

    const int tid = threadIdx.x;
    const int wave = tid / WAVE;
    const int lane = tid % WAVE;
    const int wm = wave >> 1;                // 32-row slab, 0..3
    const int wn = wave & 1;
    const int lo16 = lane & 15;
    const int hi4 = lane >> 4;
    const int mtiles = (M + BM - 1) / BM;
    const int NJ = N1 / 64;

    // staging geometry of one [64][64] tile: one 16-B chunk per thread
    const int t_row = tid / 8;
    const int t_k8 = ch_swz(t_row, tid % 8);
    auto stage_w3 = [&](int j) {
        const bf16* src = W3 + (long)(j * 64 + t_row) * K1 + t_k8 * 8;
#pragma unroll
        for (int kt = 0; kt < NK1; ++kt)
            ch_glds16(src + kt * 64, W3b + kt * 4096 + wave * 64 * 8);
    };
    auto stage_w1 = [&](int j) {
        const bf16* src = W1 + (long)t_row * N1 + j * 64 + t_k8 * 8;
#pragma unroll
        for (int t = 0; t < NT2; ++t)
            ch_glds16(src + (long)t * 64 * N1,
                      W1b + t * 4096 + wave * 64 * 8);
    };
    // the panel's k-tiles are two such tiles high: rows t_row and t_row + 64
    // (the same swizzle: 64 keeps row & 7)
    auto stage_a = [&](int mt) {
#pragma unroll
        for (int i = 0; i < BM / 64; ++i) {
            int m = mt * BM + i * 64 + t_row;
            if (m >= M) m = M - 1;           // clamped rows are never stored
            const bf16* src = X + (long)m * K1 + t_k8 * 8;
#pragma unroll
            for (int kt = 0; kt < NK1; ++kt)
                ch_glds16(src + kt * 64,
                          Ap + kt * (BM * 64) + i * 4096 + wave * 64 * 8);
        }
    };

    // epilogue chunk geometry: one 8-column chunk per thread per round
    const int e_rl = tid >> 3;               // round-local row 0..63
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
    auto res_load = [&](bf16x8* rv, int m0, int j) {
#pragma unroll
        for (int h = 0; h < NR; ++h) {
            int m = m0 + h * ER + e_rl;
            if (m >= M) m = M - 1;
            rv[h] = load_bf16x8(RES + (long)m * N1 + j * 64 + e_c8);
        }
    };
    bf16x8 rvn[NR];
    res_load(rvn, mt * BM, 0);

    for (; mt < mtiles; mt += gridDim.x) {
        const int m0 = mt * BM;
        const bool more = mt + (int)gridDim.x < mtiles;
        f32x4 acc2[2][NI2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI2; ++ni)
                acc2[mi][ni] = {0.f, 0.f, 0.f, 0.f};

        for (int j = 0; j < NJ; ++j) {
            // A panel, W3(j) and the look-ahead registers landed;
            // every wave is past GEMM2(j-1) (or the previous tile's
            // out-bounce), so W1b, the bounce and the y-tile are free
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const int jn = j + 1 < NJ ? j + 1 : 0;
            // look-ahead registers handed over by explicit moves here,
            // where nothing is in flight (see the 64-row tile's DEEP)
            bf16x8 rv[NR];
#pragma unroll
            for (int h = 0; h < NR; ++h) {
                u32x4 t = __builtin_bit_cast(u32x4, rvn[h]), c;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    asm volatile("v_mov_b32 %0, %1"
                                 : "=v"(c[q]) : "v"(t[q]) : "memory");
                rv[h] = __builtin_bit_cast(bf16x8, c);
            }
            float sc3[2], bi3[2];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3"
                             : "=&v"(sc3[ni]), "=&v"(bi3[ni])
                             : "v"(sc3n[ni]), "v"(bi3n[ni]) : "memory");
                int n = jn * 64 + wn * 32 + ni * 16 + lo16;
                sc3n[ni] = S3[n];
                bi3n[ni] = B3[n];
            }
            stage_w1(j);
            // exactly NR loads, unconditionally, AFTER the W1 stage: the
            // counted wait in front of epilogue 1 lets them stay in flight
            res_load(rvn, (j + 1 < NJ || !more)
                              ? m0 : m0 + (int)gridDim.x * BM, jn);
            // hipcc would sink the stage into the middle of GEMM1 and the
            // residual loads to its end, and halve the cover of both
            __builtin_amdgcn_sched_barrier(0);

            // ---- GEMM1: acc1[128x64] = Apanel @ W3_j^T (igemm mapping)
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
                            Ap + kt * (BM * 64) + row * 64
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
            // W1(j) landed; only the NR residual loads issued after it may
            // stay in flight. The bounce's own barrier publishes W1(j)
            asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
            static_assert(NR == 2, "the counted wait leaves NR loads");

            // ---- epilogue 1: two rounds of 64 rows through the fp32
            // bounce; the four waves whose slabs lie in the round write it
#pragma unroll
            for (int h = 0; h < NR; ++h) {
                if (wm * 32 / ER == h) {
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                int rl = wm * 32 % ER + mi * 16 + hi4 * 4 + e;
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
                const int r = h * ER + e_rl;
                if (m0 + r < M)
                    store_bf16x8(Y + (long)(m0 + r) * N1 + j * 64 + e_c8, o);
                // same 8 columns = one 16-B chunk of the A-operand layout
                store_bf16x8(ytile + r * 64 + ch_swz(r, tid & 7) * 8, o);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            }
            // next chunk's W3 (wraps to W3(0) of the next tile), after the
            // chunk's last LDS write, and in the last chunk the next tile's
            // A panel: every wave is past its last GEMM1. GEMM2 (LDS reads
            // only) is their latency cover
            if (j + 1 < NJ || more) stage_w3(jn);
            if (j + 1 == NJ && more) stage_a(mt + (int)gridDim.x);

            // ---- GEMM2: acc2[128 x N2] += ytile @ W1_j^T
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

        // ---- epilogue 2: s1/b1 + act1 on the accumulator, two rounds of
        // 64 rows through a bf16 bounce (the four row groups a wave writes
        // at once land 8 banks apart). s1/b1 are read here, once a tile,
        // and not held across the chunks
        float sc1[NI2], bi1[NI2];
#pragma unroll
        for (int ni = 0; ni < NI2; ++ni) {
            int n = wn * WN2 + ni * 16 + lo16;
            sc1[ni] = S1[n];
            bi1[ni] = B1[n];
        }
#pragma unroll
        for (int h = 0; h < NR; ++h) {
            // h = 0: every wave is past GEMM2, the bounce and the y-tile
            // are free; h = 1: round 0 has been read
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (wm * 32 / ER == h) {
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI2; ++ni)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            int r = wm * 32 % ER + mi * 16 + hi4 * 4 + e;
                            int c = wn * WN2 + ni * 16 + lo16;
                            int cs = c ^ (((r >> 2) & 3) << 4);
                            float v = acc2[mi][ni][e] * sc1[ni] + bi1[ni];
                            obuf[r * N2 + cs] = f2bf(apply_act(v, act1));
                        }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
#pragma unroll
            for (int i = 0; i < N2 * 8 / TPB; ++i) {
                int chunk = tid + i * TPB;
                int r = chunk / (N2 / 8);
                int c8 = (chunk % (N2 / 8)) * 8;
                bf16x8 o = load_bf16x8(
                    obuf + r * N2 + (c8 ^ (((r >> 2) & 3) << 4)));
                if (m0 + h * ER + r < M)
                    store_bf16x8(A2 + (long)(m0 + h * ER + r) * N2 + c8, o);
            }
        }
        // the next chunk's top barrier orders these reads before the bounce
        // is written again
    }
    // no LDS DMA may outlive the block (the last chunk stages nothing;
    // this documents the invariant)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// BM = 128 (K1 = 256, eight waves) is chain_tile128 above; everything below
// is the 64-row tile
template <int K1, int N2, int NW, int WPS, bool PROJ = false, int BM = CH_BM>
__global__ __launch_bounds__(NW * WAVE, WPS) void conv1x1_chain_kernel(
    const bf16* __restrict__ X,      // [M][K1]
    const bf16* __restrict__ W3,     // [N1][K1]
    const float* __restrict__ S3,    // [N1]
    const float* __restrict__ B3,    // [N1]
    const bf16* __restrict__ RES,    // [M][N1] (unused with PROJ)
    bf16* __restrict__ Y,            // [M][N1]
    const bf16* __restrict__ W1,     // [N2][N1]
    const float* __restrict__ S1,    // [N2]
    const float* __restrict__ B1,    // [N2]
    bf16* __restrict__ A2,           // [M][N2]
    const bf16* __restrict__ XP,     // PROJ: [M][64] shortcut input
    const bf16* __restrict__ WP,     // PROJ: [N1][64]
    const float* __restrict__ SP,    // PROJ: [N1]
    const float* __restrict__ BP,    // PROJ: [N1]
    int M, int N1, int act3, int act1) {
    static_assert(BM == CH_BM || (BM == 128 && NW == 8 && !PROJ),
                  "128-row tiles are built for eight waves, no projection");
    if constexpr (BM == 128) {
        chain_tile128<K1, N2>(X, W3, S3, B3, RES, Y, W1, S1, B1, A2, M, N1,
                              act3, act1);
        return;
    }
    constexpr int TPB = NW * WAVE;
    constexpr bool DEEP = NW == 8;           // two waves per SIMD, one block
    constexpr int WNS = NW / 2;              // waves across n (2 row slabs)
    constexpr int WN1 = 64 / WNS;            // GEMM1 wave n-width
    constexpr int NI1 = WN1 / 16;
    constexpr int NK1 = K1 / 64;             // k-tiles of GEMM1
    constexpr int NT2 = N2 / 64;             // 64-row tiles of the W1 slice
    constexpr int WN2 = N2 / WNS;            // GEMM2 wave n-width
    constexpr int NI2 = WN2 / 16;
    constexpr int OST = N2 + 8;              // bf16 out-bounce row stride
    constexpr int CPT = 512 / TPB;           // 16-B chunks of a tile/thread
    constexpr int ER = TPB / 8;              // rows per epilogue-1 round
    constexpr int NR = CH_BM / ER;           // epilogue-1 rounds
    constexpr int SCR = ER * 64 * 2;         // fp32 bounce, in bf16 units
    static_assert(NW == 4 || NW == 8, "2 x 2 or 2 x 4 waves");
    static_assert(!PROJ || (K1 == 64 && NW == 4),
                  "the projected residual is built for the K1 = 64 class");
    static_assert(CH_BM * OST <= N2 * 64 + SCR + CH_YT, "out-bounce fits");
    // PROJ keeps two W1 slices (48 KiB in all, still three blocks a CU):
    // W1(j+1) is staged with W3(j+1), a chunk ahead, into the slice GEMM2(j)
    // does not read, so no stage is waited for in the middle of a chunk.
    // Its out-bounce lies in the fp32 bounce and the y-tile, clear of both
    // slices
    constexpr int W1S = PROJ ? 2 : 1;
    static_assert(!PROJ || CH_BM * OST <= SCR + CH_YT, "out-bounce fits");

    __shared__ __attribute__((aligned(16)))
    bf16 lds[CH_BM * K1 + 64 * K1 + W1S * N2 * 64 + SCR + CH_YT];
    bf16* Ap = lds;                          // NK1 tiles [64][64]
    bf16* W3b = Ap + CH_BM * K1;             // NK1 tiles [64 n][64 k]
    bf16* W1b = W3b + 64 * K1;               // W1S x [N2][64]
    float* scratch = (float*)(W1b + W1S * N2 * 64);
    bf16* ytile = W1b + W1S * N2 * 64 + SCR;
    // epilogue 2: W1b..ytile end (PROJ: scratch..ytile end)
    bf16* obuf = PROJ ? (bf16*)scratch : W1b;

    const int tid = threadIdx.x;
    const int wave = tid / WAVE;
    const int lane = tid % WAVE;
    const int wm = wave / WNS;               // 32-row slab
    const int wn = wave % WNS;
    const int lo16 = lane & 15;
    const int hi4 = lane >> 4;
    const int mtiles = (M + CH_BM - 1) / CH_BM;
    const int NJ = N1 / 64;

    // staging geometry of one [64][64] tile: CPT chunks of 16 B per thread
    int t_row[CPT], t_k8[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        int chunk = wave * (64 * CPT) + i * 64 + lane;
        t_row[i] = chunk / 8;
        t_k8[i] = ch_swz(t_row[i], chunk % 8);
    }
    auto stage_a = [&](int mt) {
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            int m = mt * CH_BM + t_row[i];
            if (m >= M) m = M - 1;           // clamped rows are never stored
            const bf16* src = X + (long)m * K1 + t_k8[i] * 8;
#pragma unroll
            for (int kt = 0; kt < NK1; ++kt)
                ch_glds16(src + kt * 64,
                          Ap + kt * 4096 + (wave * (64 * CPT) + i * 64) * 8);
        }
    };
    auto stage_w3 = [&](int j) {
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            const bf16* src =
                W3 + (long)(j * 64 + t_row[i]) * K1 + t_k8[i] * 8;
#pragma unroll
            for (int kt = 0; kt < NK1; ++kt)
                ch_glds16(src + kt * 64,
                          W3b + kt * 4096 + (wave * (64 * CPT) + i * 64) * 8);
        }
    };
    auto stage_w1 = [&](int j, int slice) {
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            const bf16* src =
                W1 + (long)t_row[i] * N1 + j * 64 + t_k8[i] * 8;
#pragma unroll
            for (int t = 0; t < NT2; ++t)
                ch_glds16(src + (long)t * 64 * N1,
                          W1b + slice * (N2 * 64) + t * 4096
                              + (wave * (64 * CPT) + i * 64) * 8);
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
    const int e_rl = tid >> 3;               // round-local row 0..ER-1
    const int e_c8 = (tid & 7) * 8;
    const int e_cs = e_c8 ^ (((e_rl >> 2) & 3) << 4);

    int mt = blockIdx.x;
    if (mt >= mtiles) return;
    stage_a(mt);
    stage_w3(0);
    float sc3n[NI1], bi3n[NI1];
#pragma unroll
    for (int ni = 0; ni < NI1; ++ni) {
        int n = wn * WN1 + ni * 16 + lo16;
        sc3n[ni] = S3[n];
        bi3n[ni] = B3[n];
    }

    // residual chunk (rows m0.., columns j*64..) of this thread's
    // epilogue-1 rounds; rows past M are clamped and never stored
    auto res_load = [&](bf16x8* rv, int m0, int j) {
#pragma unroll
        for (int h = 0; h < NR; ++h) {
            int m = m0 + h * ER + e_rl;
            if (m >= M) m = M - 1;
            rv[h] = load_bf16x8(RES + (long)m * N1 + j * 64 + e_c8);
        }
    };
    bf16x8 rvn[NR];
    // PROJ: the residual is (XP @ WP^T) * sp + bp rounded to bf16, made
    // here. Operand fragments go straight from global to registers in the
    // GEMM1 mapping: XP once per tile, WP / sp / bp one chunk ahead
    bf16x8 xpf[2][2], wpf[NI1][2];
    float spn[NI1], bpn[NI1];
    auto xp_load = [&](int m0) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            int m = m0 + wm * 32 + mi * 16 + lo16;
            if (m >= M) m = M - 1;           // clamped rows are never stored
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                xpf[mi][ks] =
                    load_bf16x8(XP + (long)m * 64 + (ks * 4 + hi4) * 8);
        }
    };
    auto wp_load = [&](int j) {
#pragma unroll
        for (int ni = 0; ni < NI1; ++ni) {
            int n = j * 64 + wn * WN1 + ni * 16 + lo16;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                wpf[ni][ks] =
                    load_bf16x8(WP + (long)n * 64 + (ks * 4 + hi4) * 8);
        }
    };
    int w1s = 0;                             // PROJ: slice GEMM2 reads
    if constexpr (PROJ) {
        stage_w1(0, 0);
        xp_load(mt * CH_BM);
        wp_load(0);
#pragma unroll
        for (int ni = 0; ni < NI1; ++ni) {
            int n = wn * WN1 + ni * 16 + lo16;
            spn[ni] = SP[n];
            bpn[ni] = BP[n];
        }
    } else {
        res_load(rvn, mt * CH_BM, 0);
    }

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
            // and a whole chunk of work covers its latency.
            // DEEP hands them over with a move it places itself, here,
            // where the wait above has covered their loads. The compiler
            // places its copy at the end of the chunk and, unable to count
            // across the back edge, waits there for vmcnt(0): the W3 stage
            // and the residual load would drain in the middle of GEMM2
            bf16x8 rv[NR];
            // PROJ: XP, WP(j), sp/bp(j) landed with the wait above. One
            // k-tile, ks ascending, then the igemm epilogue expression and
            // its bf16 round: the value the projection launch would store
            // (kept as bf16 pairs: 8 registers across GEMM1, not 16)
            u32 rp[2][NI1][2];
            if constexpr (PROJ) {
                f32x4 accp[2][NI1];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI1; ++ni)
                        accp[mi][ni] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < NI1; ++ni)
                            accp[mi][ni] = MFMA_BF16_16x16x32(
                                xpf[mi][ks], wpf[ni][ks], accp[mi][ni]);
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI1; ++ni)
#pragma unroll
                        for (int e = 0; e < 4; e += 2) {
                            bf16x2 t;
                            t[0] = f2bf(accp[mi][ni][e] * spn[ni] + bpn[ni]);
                            t[1] = f2bf(accp[mi][ni][e + 1] * spn[ni]
                                        + bpn[ni]);
                            rp[mi][ni][e / 2] = __builtin_bit_cast(u32, t);
                        }
            }
#pragma unroll
            for (int h = 0; h < NR; ++h) {
                if constexpr (PROJ) {
                } else if constexpr (DEEP) {
                    u32x4 t = __builtin_bit_cast(u32x4, rvn[h]), c;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        asm volatile("v_mov_b32 %0, %1"
                                     : "=v"(c[q]) : "v"(t[q]) : "memory");
                    rv[h] = __builtin_bit_cast(bf16x8, c);
                } else {
                    rv[h] = rvn[h];
                }
            }
            float sc3[NI1], bi3[NI1];
#pragma unroll
            for (int ni = 0; ni < NI1; ++ni) {
                if constexpr (DEEP) {
                    asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3"
                                 : "=&v"(sc3[ni]), "=&v"(bi3[ni])
                                 : "v"(sc3n[ni]), "v"(bi3n[ni]) : "memory");
                } else {
                    sc3[ni] = sc3n[ni];
                    bi3[ni] = bi3n[ni];
                }
                int n = jn * 64 + wn * WN1 + ni * 16 + lo16;
                sc3n[ni] = S3[n];
                bi3n[ni] = B3[n];
                if constexpr (PROJ) {
                    spn[ni] = SP[n];
                    bpn[ni] = BP[n];
                }
            }
            if constexpr (PROJ) {
                // W1(j) is in its slice already (staged a chunk ago); the
                // WP fragments of the next chunk take the registers the
                // projection GEMM above has just read, and nothing in this
                // chunk waits for them
                wp_load(jn);
            } else {
                stage_w1(j, 0);
                // exactly NR loads, unconditionally, AFTER the W1 stage:
                // the counted wait in front of epilogue 1 lets them stay
                // in flight
                res_load(rvn, (j + 1 < NJ || !more)
                                  ? m0 : m0 + (int)gridDim.x * CH_BM, jn);
            }

            // ---- GEMM1: acc1[64x64] = Apanel @ W3_j^T (igemm mapping)
            f32x4 acc1[2][NI1];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI1; ++ni)
                    acc1[mi][ni] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kt = 0; kt < NK1; ++kt)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    bf16x8 af[2], bfr[NI1];
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi) {
                        int row = wm * 32 + mi * 16 + lo16;
                        af[mi] = *reinterpret_cast<bf16x8*>(
                            Ap + kt * 4096 + row * 64
                               + ch_swz(row, ks * 4 + hi4) * 8);
                    }
#pragma unroll
                    for (int ni = 0; ni < NI1; ++ni) {
                        int row = wn * WN1 + ni * 16 + lo16;
                        bfr[ni] = *reinterpret_cast<bf16x8*>(
                            W3b + kt * 4096 + row * 64
                                + ch_swz(row, ks * 4 + hi4) * 8);
                    }
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < NI1; ++ni)
                            acc1[mi][ni] = MFMA_BF16_16x16x32(
                                af[mi], bfr[ni], acc1[mi][ni]);
                }
            // W1(j) landed; only the NR residual loads for the next
            // chunk, issued after it, may stay in flight. A panel and W3b
            // are free after the barrier; DEEP has nothing to free here
            // (W3b is restaged two barriers later) and lets the bounce's
            // own barrier publish W1(j). PROJ waits for nothing here: its
            // W1(j) landed at the chunk top, and W3b and the W1 slices are
            // restaged only behind the bounce's barriers, which every wave
            // reaches after its GEMM1 reads
            if constexpr (PROJ)
                ;
            else if constexpr (NR == 2)
                asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
            if constexpr (!DEEP && !PROJ) __builtin_amdgcn_s_barrier();

            // ---- epilogue 1: NR rounds of ER rows through the fp32
            // bounce; the waves whose slab lies in the round write it
#pragma unroll
            for (int h = 0; h < NR; ++h) {
                if (NR == 1 || wm * 32 / ER == h) {
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < NI1; ++ni)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                int rl = wm * 32 % ER + mi * 16 + hi4 * 4 + e;
                                int c = wn * WN1 + ni * 16 + lo16;
                                int cs = c ^ (((rl >> 2) & 3) << 4);
                                float v = acc1[mi][ni][e] * sc3[ni] + bi3[ni];
                                // the same fp32 add of the same operands
                                // as the reading side's below
                                if constexpr (PROJ)
                                    v += __builtin_bit_cast(
                                        float,
                                        e % 2 ? rp[mi][ni][e / 2] & 0xffff0000u
                                              : rp[mi][ni][e / 2] << 16);
                                scratch[rl * 64 + cs] = v;
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
                    if constexpr (!PROJ) v += bf2f(rv[h][q]);
                    o[q] = f2bf(apply_act(v, act3));
                }
                const int r = h * ER + e_rl;
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
            if (j + 1 < NJ || more) {
                stage_w3(jn);
                if constexpr (PROJ) stage_w1(jn, w1s ^ 1);
            }

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
                        W1b + (PROJ ? w1s * (N2 * 64) : 0) + row * 64
                            + ch_swz(row, ks * 4 + hi4) * 8);
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
                        acc2[mi][ni] = MFMA_BF16_16x16x32(af[mi], bfr,
                                                          acc2[mi][ni]);
                }
            }
            if constexpr (PROJ) w1s ^= 1;
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
        if constexpr (PROJ)
            if (more) xp_load((mt + (int)gridDim.x) * CH_BM);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int i = 0; i < N2 * 8 / TPB; ++i) {
            int chunk = tid + i * TPB;
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
    // fused vs two launches, us, min..max of 2 x 3 repeats, batch 256 | 64
    {64, 256, 64},     // 189..219 vs 338..349 | 43..51 vs 73..80
    {64, 256, 128},    // 222..228 vs 419..422 | 57..59 vs 99..101
    {128, 512, 128},   // 124..127 vs 251..255 | 35..36 vs 56..57
    {128, 512, 256},   // 155..158 vs 307..311 | 42..44 vs 72..72
    // eight waves (four waves, one per SIMD: 134..136 | 36..37 and
    // 207..213 | 55..56, the second a draw with two launches)
    {256, 1024, 256},  // 111..118 vs 142..149 | 30..31 vs 42..43
    {256, 1024, 512},  // 149..154 vs 207..211 | 37..40 vs 54..54
};

bool chain_policy(int K1, int N1, int N2) {
    for (const ChainWin& w : kChainWins)
        if (w.K1 == K1 && w.N1 == N1 && w.N2 == N2) return true;
    return false;
}

// Tile height of the K1 = 256, N2 = 256 instantiation: 128 rows where they
// measured faster than 64 (tools/chainbench.py --bm, MI355X, N1 = 1024, us,
// min..max of 2 x 3 repeats; 128 rows | 64 rows | 64-row tiles):
//   batch 256   91.3..95.0 | 116.2..127.5 | 784
//   batch 128   46.8..48.1 |  57.2..57.7  | 392
//   batch 64    44.8..46.5 |  30.5..31.0  | 196 (98 blocks on 256 CUs)
// The gate is the 64-row tile count: above 256 the 64-row form runs more
// than one round of tiles per CU, at and below it 128 rows would leave CUs
// without a tile.
bool bm128_policy(int M) { return (M + CH_BM - 1) / CH_BM > 256; }

}  // namespace

ChainLaunch launch_conv1x1_chain(const void* x, const void* w3,
                                 const float* s3, const float* b3,
                                 const void* res, void* y, bool relu3,
                                 const void* w1, const float* s1,
                                 const float* b1, void* a2, bool relu1,
                                 int M, int K1, int N1, int N2, bool force,
                                 int max_blocks, int bm, hipStream_t s) {
    if (M <= 0 || N1 < 64 || N1 % 64 != 0) return {0, 0};
    if (!force && !chain_policy(K1, N1, N2)) return {0, 0};
    const int a3 = relu3 ? ACT_RELU : ACT_NONE;
    const int a1 = relu1 ? ACT_RELU : ACT_NONE;
    if (K1 == 256 && N2 == 256 && (bm == 128 || (bm == 0 && bm128_policy(M)))) {
        const int mtiles = (M + 127) / 128;
        int gx = 256;
        if (max_blocks > 0) gx = max_blocks;
        if (gx > mtiles) gx = mtiles;
        if (max_blocks <= 0) {               // even rounds, as below
            int rounds = (mtiles + gx - 1) / gx;
            gx = (mtiles + rounds - 1) / rounds;
        }
        hipLaunchKernelGGL(
            (conv1x1_chain_kernel<256, 256, 8, 1, false, 128>), dim3(gx),
            dim3(8 * WAVE), 0, s, (const bf16*)x, (const bf16*)w3, s3, b3,
            (const bf16*)res, (bf16*)y, (const bf16*)w1, s1, b1, (bf16*)a2,
            (const bf16*)nullptr, (const bf16*)nullptr,
            (const float*)nullptr, (const float*)nullptr, M, N1, a3, a1);
        return {gx, 128};
    }
    const int mtiles = (M + CH_BM - 1) / CH_BM;
#define CHAIN(K1v, N2v, NWv, WPSv)                                        \
    do {                                                                  \
        int gx = 256 * WPSv;                                              \
        if (max_blocks > 0) gx = max_blocks;                              \
        if (gx > mtiles) gx = mtiles;                                     \
        /* one block per CU: the last round of tiles would leave most  */ \
        /* CUs idle, so spread the same rounds evenly (784 tiles: 196  */ \
        /* blocks x 4, not 256 blocks of which 16 run a fourth)        */ \
        if (WPSv == 1 && max_blocks <= 0) {                               \
            int rounds = (mtiles + gx - 1) / gx;                          \
            gx = (mtiles + rounds - 1) / rounds;                          \
        }                                                                 \
        hipLaunchKernelGGL((conv1x1_chain_kernel<K1v, N2v, NWv, WPSv>),   \
                           dim3(gx), dim3(NWv * WAVE), 0, s,              \
                           (const bf16*)x, (const bf16*)w3, s3, b3,       \
                           (const bf16*)res, (bf16*)y, (const bf16*)w1,   \
                           s1, b1, (bf16*)a2, (const bf16*)nullptr,       \
                           (const bf16*)nullptr, (const float*)nullptr,   \
                           (const float*)nullptr, M, N1, a3, a1);         \
        return {gx, CH_BM};                                               \
    } while (0)
    if (K1 == 64 && N2 == 64) CHAIN(64, 64, 4, 3);
    if (K1 == 64 && N2 == 128) CHAIN(64, 128, 4, 3);
    if (K1 == 128 && N2 == 128) CHAIN(128, 128, 4, 2);
    if (K1 == 128 && N2 == 256) CHAIN(128, 256, 4, 2);
    if (K1 == 256 && N2 == 256) CHAIN(256, 256, 8, 1);
    if (K1 == 256 && N2 == 512) CHAIN(256, 512, 8, 1);
#undef CHAIN
    return {0, 0};
}

int launch_conv1x1_chain_proj(const void* x, const void* w3, const float* s3,
                              const float* b3, const void* xp,
                              const void* wp, const float* sp,
                              const float* bp, void* y, bool relu3,
                              const void* w1, const float* s1,
                              const float* b1, void* a2, bool relu1, int M,
                              int K1, int KP, int N1, int N2, bool force,
                              int max_blocks, hipStream_t s) {
    if (M <= 0 || N1 < 64 || N1 % 64 != 0) return 0;
    if (K1 != 64 || KP != 64 || N2 != 64) return 0;
    const int mtiles = (M + CH_BM - 1) / CH_BM;
    // Policy: the measured class, at every size. Kernel vs the projection
    // launch plus the chain launch (tools/chainbench.py, us, min..max of
    // 2 x 3 repeats): batch 256 222..278 vs 342..358, batch 64 52..54 vs
    // 82..83, batch 16 24..24 vs 30..31, batch 8 13..14 vs 20..20, batch 1
    // (49 tiles) 8.5..9.4 vs 12.1..12.3: no tile-count gate
    if (!force && N1 != 256) return 0;
    int gx = 256 * 3;
    if (max_blocks > 0) gx = max_blocks;
    if (gx > mtiles) gx = mtiles;
    hipLaunchKernelGGL((conv1x1_chain_kernel<64, 64, 4, 3, true>), dim3(gx),
                       dim3(4 * WAVE), 0, s, (const bf16*)x,
                       (const bf16*)w3, s3, b3, (const bf16*)nullptr,
                       (bf16*)y, (const bf16*)w1, s1, b1, (bf16*)a2,
                       (const bf16*)xp, (const bf16*)wp, sp, bp, M, N1,
                       relu3 ? ACT_RELU : ACT_NONE,
                       relu1 ? ACT_RELU : ACT_NONE);
    return gx;
}

}  // namespace defer_hip
