// LayerNorm over the channel (last, contiguous) dim, bf16 and fp32:
//
//   y[row][c] = (x[row][c] - mean) / sqrt(var + eps) * weight[c] + bias[c]
//
// mean and the biased var are taken per row of C values at run time. In
// NHWC a pixel's channels are one contiguous run, so a row is a handful of
// 16-byte vectors (8 bf16 or 4 fp32) and this is one streaming pass.
//
// Work split. A group of G lanes (a power of two, 1..64, inside one wave)
// owns a row; lane l of the group holds the vectors l, l + G, l + 2G, ... of
// the row, VPL of them, so the group's loads and stores are contiguous runs.
// The row is read from global memory once, held unpacked in fp32 registers,
// and written once. G follows C: the host picks the VPL in {1, 2, 3, 4, 6,
// 8} whose G * VPL wastes the fewest vector slots (C = 96 in bf16 is 12
// vectors: VPL 3, G 4, sixteen rows per wave and no idle lane; C = 768 is
// VPL 3, G 32; C = 2048 is VPL 4, G 64). A 256-lane workgroup holds 256 / G
// rows and walks the rows grid-stride; weight and bias are loaded once per
// lane, before the loop.
//
// Statistics, in fp32, two passes over the registers: the sum, then the sum
// of squared differences from the mean (never E[x^2] - E[x]^2, which loses
// every digit when |mean| >> sigma). A lane adds its values in the fixed
// order (vector, element); the group's lanes combine by an xor-shuffle tree
// over the masks G/2, ..., 1, so every lane ends with the same bits. mean,
// var and the normalised value are never rounded to bf16; one rounding at
// the end. x - mean is exactly 0 on a constant row whose sum is exact, and
// the output is then bias, bit for bit. No atomics, no host sync, no LDS,
// no scratch; identical from run to run.
#include "common.h"
#include "kernels.h"

// no packed fp32 instructions in this file's kernels
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

constexpr int LN_TPB = 256;
constexpr int LN_GRID_CAP = 4096;

struct LnBf16 {
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

struct LnF32 {
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

// sum over the G lanes of a group; G is uniform over the grid
__device__ __forceinline__ float ln_group_sum(float v, int G) {
    for (int m = G >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, WAVE);
    return v;
}

template <typename E, int VPL>
__global__ __launch_bounds__(LN_TPB) void layernorm_kernel(
    const typename E::T* __restrict__ x, const float* __restrict__ weight,
    const float* __restrict__ bias, typename E::T* __restrict__ y, long rows,
    int C, int G, float eps) {
    typedef typename E::Vec Vec;
    constexpr int V = E::V;
    const int CV = C / V;
    const int l = threadIdx.x & (G - 1);
    const int rpb = LN_TPB / G;                  // rows of a workgroup
    const float fc = (float)C;   // divided by, so a constant row is exact

    float wf[VPL][V], bf[VPL][V];
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
        const int cv = l + k * G;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            wf[k][j] = cv < CV ? weight[cv * V + j] : 0.0f;
            bf[k][j] = cv < CV ? bias[cv * V + j] : 0.0f;
        }
    }

    // a group's lanes share the row, so they leave the loop together and
    // every shuffle below stays inside a group of live lanes
    for (long row = (long)blockIdx.x * rpb + threadIdx.x / G; row < rows;
         row += (long)gridDim.x * rpb) {
        const typename E::T* xr = x + row * C;
        float v[VPL][V];
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            const int cv = l + k * G;
            if (cv < CV) {
                const Vec raw = *reinterpret_cast<const Vec*>(xr + cv * V);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    v[k][j] = E::get(raw, j);
                    sum += v[k][j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) v[k][j] = 0.0f;
            }
        }
        const float mean = ln_group_sum(sum, G) / fc;

        float sq = 0.0f;
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            const bool live = l + k * G < CV;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                v[k][j] = live ? v[k][j] - mean : 0.0f;
                sq = fmaf(v[k][j], v[k][j], sq);
            }
        }
        const float var = ln_group_sum(sq, G) / fc;
        const float rstd = 1.0f / sqrtf(var + eps);

        typename E::T* yr = y + row * C;
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            const int cv = l + k * G;
            if (cv >= CV) continue;
            Vec out;
#pragma unroll
            for (int j = 0; j < V; ++j)
                E::set(out, j, fmaf(v[k][j] * rstd, wf[k][j], bf[k][j]));
            *reinterpret_cast<Vec*>(yr + cv * V) = out;
        }
    }
}

template <typename E>
void launch_ln(const void* x, const float* weight, const float* bias,
               void* y, long rows, int C, float eps,
               const defer_hip::LnPlan& pl, int max_blocks, hipStream_t s) {
    typedef typename E::T T;
    typedef void (*Kernel)(const T*, const float*, const float*, T*, long,
                           int, int, float);
    Kernel k = nullptr;
    switch (pl.VPL) {
        case 1: k = layernorm_kernel<E, 1>; break;
        case 2: k = layernorm_kernel<E, 2>; break;
        case 3: k = layernorm_kernel<E, 3>; break;
        case 4: k = layernorm_kernel<E, 4>; break;
        case 6: k = layernorm_kernel<E, 6>; break;
        default: k = layernorm_kernel<E, 8>; break;
    }
    const int rpb = LN_TPB / pl.G;
    long grid = (rows + rpb - 1) / rpb;
    const long cap = max_blocks > 0 ? max_blocks : LN_GRID_CAP;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(LN_TPB), 0, s,
                       (const T*)x, weight, bias, (T*)y, rows, C, pl.G, eps);
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

namespace defer_hip {

LnPlan layernorm_plan(int C, int vec) {
    static const int vpls[] = {1, 2, 3, 4, 6, 8};
    const int CV = C / vec;
    LnPlan best{0, 0};
    int best_waste = 1 << 30;
    for (int vpl : vpls) {
        const int need = (CV + vpl - 1) / vpl;
        int G = 1;
        while (G < need) G *= 2;
        if (G > WAVE) continue;
        const int waste = G * vpl - CV;
        if (waste < best_waste) {
            best_waste = waste;
            best = {G, vpl};
        }
    }
    return best;   // G == 0: C / vec > 512 vectors, no kernel
}

void launch_layernorm(const void* x, const float* weight, const float* bias,
                      void* y, long rows, int C, float eps, bool f32,
                      int max_blocks, hipStream_t s) {
    if (rows <= 0) return;
    const LnPlan pl = layernorm_plan(C, f32 ? 4 : 8);
    if (f32) launch_ln<LnF32>(x, weight, bias, y, rows, C, eps, pl,
                              max_blocks, s);
    else launch_ln<LnBf16>(x, weight, bias, y, rows, C, eps, pl, max_blocks,
                           s);
}

}  // namespace defer_hip
