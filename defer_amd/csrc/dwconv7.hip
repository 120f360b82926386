// 7x7 depthwise convolution, stride 1, padding 3, NHWC, bf16 and fp32
// (the first layer of every ConvNeXt block):
//
//   y[n][oh][ow][c] = sum_{r,s} x[n][oh-3+r][ow-3+s][c] * w[r][s][c] + bias[c]
//
// dwconv.hip keeps the weights in registers and leaves the horizontal
// overlap of neighbouring columns to L1. Neither stretches to 7x7: 49 taps x
// 8 channels are 392 fp32 registers, and every input vector would be fetched
// by seven neighbouring lanes. Here the window and the weights live in LDS.
//
// Work split. A workgroup of 256 lanes owns a TH x TW spatial tile of one
// image times a block of CBV channel vectors (a vector is 16 bytes: 8 bf16
// or 4 fp32; the CBV vectors of a pixel are one contiguous run). blockIdx.y
// is the channel block, so a workgroup stages its 49 x CBV weight vectors
// once; blockIdx.x walks the (image, tile) pairs grid-stride.
//
// Staging. Per tile the workgroup copies the (TH+6) x (TW+6) input window of
// its channel block into LDS once, with 16-byte global loads and 16-byte LDS
// writes; positions outside the image (and channel vectors past C in the
// last block) are written as zeros, so the arithmetic has no border cases.
// An input element is therefore read from global memory once per tile that
// contains it, halo included, and never once per tap or per neighbouring
// lane. The pixel pitch in LDS is CBV vectors plus 0..3 vectors of padding,
// chosen on the host so that the 16 lanes one ds_read_b128 pass serves
// (CBV channel vectors of one output run, then the next run, 4 pixels on)
// fall on distinct banks. That padded pitch, and the zero fill, are why the
// window goes through registers rather than global_load_lds, which writes a
// wave's 64 x 16 bytes to one unpadded run.
//
// Lane work. A lane owns one channel vector and a run of P = 4 adjacent
// outputs of one row. For each tap row r = 0..6 it reads the P + 6 = 10
// window vectors under the run and the 7 weight vectors of the row from LDS
// and slides the window over them in registers: 17 16-byte LDS reads feed
// 7 * P * V fmaf, i.e. 17 / 224 = 0.076 reads per fmaf in bf16 (V = 8) and
// 17 / 112 = 0.152 in fp32 (V = 4); tap by tap it would be 2 reads per V
// fmaf, 0.25 and 0.5.
//
// Arithmetic. fp32 fmaf in the fixed tap order r, then s, for every output;
// the bias is added in fp32; one rounding to the output dtype. No atomics
// and no split sums: results are identical from run to run.
//
// Tile policy (dw7_geom): TH = ceil(H / ceil(H / 8)) and TW = 16, or W
// rounded up to 4 when W < 16, so 56, 28, 14 and 7 rows all split into
// whole 7-row tiles; CBV is the power of two in 4..16 that gives the 256
// lanes one item each (8 for a 7 x 16 tile, 16 for the 7 x 8 tile of a 7x7
// image), halved while window + weights pass 64 KiB.
//
// Offsets inside an image are 32-bit (the binding checks H * W * C < 2^31);
// the image base is 64-bit. All loops over taps and the run have constant
// bounds and are unrolled: no scratch. One template serves both dtypes.
#include "common.h"
#include "kernels.h"

// no packed fp32 instructions in this file's kernels
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

constexpr int D7_TPB = 256;
constexpr int D7_P = 4;             // outputs of a lane's run
constexpr int D7_R = 7;
constexpr int D7_GRID_CAP = 1024;   // workgroups along x

struct D7Bf16 {
    typedef bf16 T;
    typedef bf16x8 Vec;
    static constexpr int V = 8;
    static __device__ __forceinline__ float get(const Vec& v, int j) {
        return bf2f(v[j]);
    }
    static __device__ __forceinline__ void set(Vec& v, int j, float f) {
        v[j] = f2bf(f);
    }
};

struct D7F32 {
    typedef float T;
    typedef f32x4 Vec;
    static constexpr int V = 4;
    static __device__ __forceinline__ float get(const Vec& v, int j) {
        return v[j];
    }
    static __device__ __forceinline__ void set(Vec& v, int j, float f) {
        v[j] = f;
    }
};

template <typename E>
__global__ __launch_bounds__(D7_TPB) void dwconv7_kernel(
    const typename E::T* __restrict__ x, const typename E::T* __restrict__ w,
    const float* __restrict__ bias, typename E::T* __restrict__ y,
    defer_hip::Dw7Geom g) {
    typedef typename E::Vec Vec;
    constexpr int V = E::V;
    extern __shared__ __attribute__((aligned(16))) unsigned char d7_smem[];
    Vec* wl = reinterpret_cast<Vec*>(d7_smem);            // [49][CBV]
    Vec* win = wl + D7_R * D7_R * g.CBV;                  // [WH][WW][PV]

    const int tid = threadIdx.x;
    const int CV = g.C / V;
    const int cv0 = blockIdx.y * g.CBV;
    const int WW = g.TW + 6, WH = g.TH + 6;
    const int runs = g.TW / D7_P;

    Vec zero;
#pragma unroll
    for (int j = 0; j < V; ++j) E::set(zero, j, 0.0f);

    // the block's weights, once: [tap][cvl]
    for (int i = tid; i < D7_R * D7_R * g.CBV; i += D7_TPB) {
        const int cvl = i % g.CBV, k = i / g.CBV;
        const int cv = cv0 + cvl;
        wl[i] = cv < CV ? *reinterpret_cast<const Vec*>(w + k * g.C + cv * V)
                        : zero;
    }

    const int tiles_img = g.nth * g.ntw;
    for (long t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const int n = (int)(t / tiles_img);
        const int ti = (int)(t - (long)n * tiles_img);
        const int oh0 = (ti / g.ntw) * g.TH, ow0 = (ti % g.ntw) * g.TW;
        const long img = (long)n * g.H * g.W * g.C;
        const typename E::T* xn = x + img;

        // every lane is done with the previous window
        __syncthreads();
        for (int i = tid; i < WH * WW * g.CBV; i += D7_TPB) {
            const int cvl = i % g.CBV, px = i / g.CBV;
            const int col = px % WW, row = px / WW;
            const int ih = oh0 - 3 + row, iw = ow0 - 3 + col;
            const int cv = cv0 + cvl;
            const bool ok = ih >= 0 && ih < g.H && iw >= 0 && iw < g.W &&
                            cv < CV;
            Vec v = zero;
            if (ok)
                v = *reinterpret_cast<const Vec*>(
                    xn + (ih * g.W + iw) * g.C + cv * V);
            win[px * g.PV + cvl] = v;
        }
        __syncthreads();

        for (int it = tid; it < g.TH * runs * g.CBV; it += D7_TPB) {
            const int cvl = it % g.CBV, q = it / g.CBV;
            const int run = q % runs, orow = q / runs;
            const int cv = cv0 + cvl;
            const int oh = oh0 + orow, owr = ow0 + run * D7_P;
            if (cv >= CV || oh >= g.H || owr >= g.W) continue;

            float acc[D7_P][V];
#pragma unroll
            for (int o = 0; o < D7_P; ++o)
#pragma unroll
                for (int j = 0; j < V; ++j) acc[o][j] = 0.0f;

            const Vec* wrow = win + (orow * WW + run * D7_P) * g.PV + cvl;
            // a real loop over the tap rows: unrolled, the compiler hoists
            // all 119 LDS reads above the arithmetic and spills
#pragma unroll 1
            for (int r = 0; r < D7_R; ++r) {
                float xf[D7_P + 6][V];
#pragma unroll
                for (int k = 0; k < D7_P + 6; ++k) {
                    const Vec v = wrow[(r * WW + k) * g.PV];
#pragma unroll
                    for (int j = 0; j < V; ++j) xf[k][j] = E::get(v, j);
                }
#pragma unroll
                for (int s = 0; s < D7_R; ++s) {
                    const Vec wv = wl[(r * D7_R + s) * g.CBV + cvl];
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        const float wj = E::get(wv, j);
#pragma unroll
                        for (int o = 0; o < D7_P; ++o)
                            acc[o][j] = fmaf(xf[o + s][j], wj, acc[o][j]);
                    }
                }
            }

            float bi[V];
#pragma unroll
            for (int j = 0; j < V; ++j) bi[j] = bias[cv * V + j];
            typename E::T* yp = y + img + (oh * g.W + owr) * g.C + cv * V;
#pragma unroll
            for (int o = 0; o < D7_P; ++o) {
                if (owr + o >= g.W) continue;
                Vec out;
#pragma unroll
                for (int j = 0; j < V; ++j) E::set(out, j, acc[o][j] + bi[j]);
                *reinterpret_cast<Vec*>(yp + o * g.C) = out;
            }
        }
    }
}

template <typename E>
void launch_d7(const void* x, const void* w, const float* bias, void* y,
               const defer_hip::Dw7Geom& g, int max_blocks, hipStream_t s) {
    typedef typename E::T T;
    if (g.tiles <= 0) return;
    long gx = max_blocks > 0 ? max_blocks : D7_GRID_CAP;
    if (gx > g.tiles) gx = g.tiles;
    hipLaunchKernelGGL(dwconv7_kernel<E>, dim3((unsigned)gx, g.ncb),
                       dim3(D7_TPB), g.lds_bytes, s, (const T*)x, (const T*)w,
                       bias, (T*)y, g);
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

namespace defer_hip {

Dw7Geom dw7_geom(int NB, int H, int W, int C, int vec) {
    Dw7Geom g{};
    g.N = NB; g.H = H; g.W = W; g.C = C;
    const int CV = C / vec;
    g.nth = (H + 7) / 8;
    g.TH = (H + g.nth - 1) / g.nth;
    g.TW = W >= 16 ? 16 : (W + D7_P - 1) / D7_P * D7_P;
    g.ntw = (W + g.TW - 1) / g.TW;
    const int lanes = g.TH * (g.TW / D7_P);
    int cbv = 4;
    while (cbv < 16 && cbv * 2 * lanes <= D7_TPB) cbv *= 2;
    for (;; cbv /= 2) {
        g.CBV = cbv < CV ? cbv : CV;
        // the pad that puts the next run's vectors (P pixels on) right
        // after this run's in the 16 vector slots of a 256-byte bank row
        int pad = 1;
        for (int p = 0; p < 4; ++p)
            if ((D7_P * (g.CBV + p)) % 16 == g.CBV % 16) { pad = p; break; }
        g.PV = g.CBV + pad;
        g.lds_bytes = 16 * (D7_R * D7_R * g.CBV +
                            (g.TH + 6) * (g.TW + 6) * g.PV);
        if (g.lds_bytes <= 64 * 1024 || cbv == 1) break;
    }
    g.ncb = (CV + g.CBV - 1) / g.CBV;
    g.tiles = (long)NB * g.nth * g.ntw;
    return g;
}

void launch_dwconv7(const void* x, const void* w, const float* bias, void* y,
                    int NB, int H, int W, int C, bool f32, int max_blocks,
                    hipStream_t s) {
    const Dw7Geom g = dw7_geom(NB, H, W, C, f32 ? 4 : 8);
    if (f32) launch_d7<D7F32>(x, w, bias, y, g, max_blocks, s);
    else launch_d7<D7Bf16>(x, w, bias, y, g, max_blocks, s);
}

}  // namespace defer_hip
