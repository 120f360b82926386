// Squeeze-excite, NHWC, bf16 and fp32 (MobileNetV3, and with other gates
// the EfficientNet / MnasNet / RegNetY family):
//
//   s[n][c] = mean over h, w of x[n][h][w][c]
//   z[n][r] = act(sum_c w1[r][c] * s[n][c] + b1[r])
//   g[n][c] = hardsigmoid(sum_r w2[c][r] * z[n][r] + b2[c])
//   y[n][h][w][c] = x[n][h][w][c] * g[n][c]
//
// Two kernels. se_gate_kernel makes g in fp32, one workgroup per image:
// s, z and g are never rounded to bf16, every sum is fp32 in a fixed order
// and there are no atomics, so a run repeats bit for bit.
// channel_scale_kernel streams x once more and writes y.
//
// The pool is the part of the gate kernel that moves bytes. Its lanes are
// laid out as (channel vector of 16 bytes) x (pixel group): with CV channel
// vectors a block of 512 lanes forms 512 / CV pixel groups, group g takes
// the pixels g, g + groups, ..., and neighbouring lanes take neighbouring
// channel vectors, so a wave reads contiguous runs and all lanes load
// whatever C is (504 of 512 at C = 72, 480 at C = 960 bf16). Each lane sums
// its pixels in rising order, the groups are summed through LDS in rising
// order, and s stays in LDS. More than 512 channel vectors are served 512 at
// a time. The block is 512 lanes, not 256, because one block is all an image
// gets: with 256 the FCs of the 960 / 240 block took twice as many passes.
//
// The two FCs are small (at most 240 x 960 in MobileNetV3) and their
// weights are the same for every block, so they are read straight from
// global memory (L2). A row of the weight matrix is one dot product: the
// lanes of a power-of-two group of up to 64 lanes take its 16-byte vectors
// in turn, and the group is reduced by xor shuffles, a fixed tree. A group
// is as small as the row allows with four vectors per lane, and takes four
// rows at once, so a lane has 16 loads in flight (se_fc). w2's rows are Cr
// long: where Cr is no multiple of the vector they are unaligned and are
// read element by element.
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int SE_TPB = 512;

struct SeBf16 {
    typedef bf16 T;
    typedef bf16x8 Vec;
    static constexpr int V = 8;
    static __device__ __forceinline__ float get(const Vec& v, int j) {
        return bf2f(v[j]);
    }
    static __device__ __forceinline__ void set(Vec& v, int j, float f) {
        v[j] = f2bf(f);
    }
    static __device__ __forceinline__ float tof(T v) { return bf2f(v); }
};

struct SeF32 {
    typedef float T;
    typedef f32x4 Vec;
    static constexpr int V = 4;
    static __device__ __forceinline__ float get(const Vec& v, int j) {
        return v[j];
    }
    static __device__ __forceinline__ void set(Vec& v, int j, float f) {
        v[j] = f;
    }
    static __device__ __forceinline__ float tof(T v) { return v; }
};

// out(r, sum_k w[r][k] * in[k]) for every row r of w [rows][cols]; in is in
// LDS, 16-byte aligned. VEC: cols % V == 0, so every row is 16-byte aligned
// and is read as vectors; otherwise element by element. Every lane of the
// block must call this (shuffles, uniform trip counts).
//
// The weights come from L2, a microsecond away, so what a lane has in flight
// decides the time: a group of G lanes takes SE_RU rows at once and SE_IU
// items of each, all SE_RU * SE_IU loads issued before the first fmaf. Loads
// past the end of a row or of the matrix read the last item or row instead
// (in bounds) and are left out of the sum. A row's sum keeps one order: the
// lane's items in rising order, then the xor tree.
constexpr int SE_RU = 4, SE_IU = 4;

template <typename E, bool VEC, typename Out>
__device__ __forceinline__ void se_fc(const typename E::T* __restrict__ w,
                                      int rows, int cols, const float* in,
                                      Out&& out) {
    typedef typename E::Vec Vec;
    typedef typename std::conditional<VEC, Vec, typename E::T>::type Item;
    constexpr int V = VEC ? E::V : 1;
    const int items = cols / V;
    int G = 1;                          // lanes per row, a power of two
    while (G * SE_IU < items && G < WAVE) G <<= 1;
    const int rpp = SE_TPB / G;         // lane groups of the block
    const int l = threadIdx.x % G, sub = threadIdx.x / G;
    for (int r0 = 0; r0 < rows; r0 += rpp * SE_RU) {
        float acc[SE_RU];
#pragma unroll
        for (int u = 0; u < SE_RU; ++u) acc[u] = 0.0f;
        for (int it0 = 0; it0 < items; it0 += G * SE_IU) {
            Item wv[SE_RU][SE_IU];
#pragma unroll
            for (int u = 0; u < SE_RU; ++u) {
                const int r = min(r0 + u * rpp + sub, rows - 1);
#pragma unroll
                for (int i = 0; i < SE_IU; ++i) {
                    const int it = min(it0 + i * G + l, items - 1);
                    wv[u][i] = *reinterpret_cast<const Item*>(
                        w + (long)r * cols + it * V);
                }
            }
#pragma unroll
            for (int i = 0; i < SE_IU; ++i) {
                const int it = it0 + i * G + l;
                if (it >= items) continue;
                if constexpr (VEC) {
#pragma unroll
                    for (int q = 0; q < V / 4; ++q) {
                        const f32x4 sv = *reinterpret_cast<const f32x4*>(
                            in + it * V + q * 4);
#pragma unroll
                        for (int u = 0; u < SE_RU; ++u)
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                acc[u] = fmaf(E::get(wv[u][i], q * 4 + e),
                                              sv[e], acc[u]);
                    }
                } else {
                    const float sv = in[it];
#pragma unroll
                    for (int u = 0; u < SE_RU; ++u)
                        acc[u] = fmaf(E::tof(wv[u][i]), sv, acc[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < SE_RU; ++u) {
            for (int off = G >> 1; off > 0; off >>= 1)
                acc[u] += __shfl_xor(acc[u], off);
            const int r = r0 + u * rpp + sub;
            if (r < rows && l == 0) out(r, acc[u]);
        }
    }
}

template <typename E>
__global__ __launch_bounds__(SE_TPB) void se_gate_kernel(
    const typename E::T* __restrict__ x, const typename E::T* __restrict__ w1,
    const float* __restrict__ b1, const typename E::T* __restrict__ w2,
    const float* __restrict__ b2, float* __restrict__ g, int HW, int C,
    int Cr, int act) {
    typedef typename E::Vec Vec;
    constexpr int V = E::V;
    extern __shared__ __attribute__((aligned(16))) float se_lds[];
    float* s = se_lds;                  // [C] means
    float* z = se_lds + C;              // [Cr] hidden values, C % 4 == 0
    __shared__ float part[V * SE_TPB];  // [j][lane] partial sums of a lane

    const int tid = threadIdx.x;
    const int n = blockIdx.x;
    const int CV = C / V;
    const typename E::T* xn = x + (long)n * HW * C;
    const float hw = (float)HW;

    for (int cv0 = 0; cv0 < CV; cv0 += SE_TPB) {
        const int nvec = min(SE_TPB, CV - cv0);
        const int PG = SE_TPB / nvec;           // pixel groups
        const int v = tid % nvec, pg = tid / nvec;
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.0f;
        if (pg < PG) {
            const typename E::T* xc = xn + (long)(cv0 + v) * V;
            int p = pg;
            // eight loads in flight; the adds keep the rising pixel order
            for (; p + 7 * PG < HW; p += 8 * PG) {
                Vec a[8];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    a[u] = *reinterpret_cast<const Vec*>(
                        xc + (long)(p + u * PG) * C);
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int j = 0; j < V; ++j) acc[j] += E::get(a[u], j);
            }
            for (; p < HW; p += PG) {
                const Vec a = *reinterpret_cast<const Vec*>(
                    xc + (long)p * C);
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] += E::get(a, j);
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) part[j * SE_TPB + tid] = acc[j];
        __syncthreads();
        for (int idx = tid; idx < nvec * V; idx += SE_TPB) {
            const int j = idx / nvec, vv = idx % nvec;
            float sum = 0.0f;
            for (int q = 0; q < PG; ++q)
                sum += part[j * SE_TPB + q * nvec + vv];
            s[(cv0 + vv) * V + j] = sum / hw;
        }
        __syncthreads();
    }

    se_fc<E, true>(w1, Cr, C, s, [&](int r, float a) {
        if (b1) a += b1[r];
        z[r] = act == ACT_RELU ? fmaxf(a, 0.0f) : a;
    });
    __syncthreads();
    float* gn = g + (long)n * C;
    auto gate = [&](int c, float a) {
        if (b2) a += b2[c];
        gn[c] = hardsigmoid_f(a);
    };
    if (Cr % V == 0) se_fc<E, true>(w2, C, Cr, z, gate);
    else se_fc<E, false>(w2, C, Cr, z, gate);
}

// y = x * g[n][c]; total vectors of x, hwcv = HW * CV vectors per image
template <typename E>
__global__ void channel_scale_kernel(const typename E::T* __restrict__ x,
                                     const float* __restrict__ g,
                                     typename E::T* __restrict__ y,
                                     long total, long hwcv, int CV) {
    typedef typename E::Vec Vec;
    constexpr int V = E::V;
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total; i += stride) {
        const long n = i / hwcv;
        const int cv = (int)(i % CV);
        const float* gp = g + (n * CV + cv) * V;
        const Vec v = *reinterpret_cast<const Vec*>(x + i * V);
        Vec o;
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
            const f32x4 gv = *reinterpret_cast<const f32x4*>(gp + q * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                E::set(o, q * 4 + e, E::get(v, q * 4 + e) * gv[e]);
        }
        *reinterpret_cast<Vec*>(y + i * V) = o;
    }
}

int grid1d(long work, int block) {
    long g = (work + block - 1) / block;
    return (int)(g < 2048 ? g : 2048);
}

template <typename E>
void launch_gate(const void* x, const void* w1, const float* b1,
                 const void* w2, const float* b2, float* g, int NB, int HW,
                 int C, int Cr, int act, hipStream_t s) {
    typedef typename E::T T;
    const size_t lds = (size_t)(C + Cr) * sizeof(float);
    hipLaunchKernelGGL(se_gate_kernel<E>, dim3(NB), dim3(SE_TPB), lds, s,
                       (const T*)x, (const T*)w1, b1, (const T*)w2, b2, g,
                       HW, C, Cr, act);
}

template <typename E>
void launch_scale(const void* x, const float* g, void* y, long NB, long HW,
                  int C, hipStream_t s) {
    typedef typename E::T T;
    const int CV = C / E::V;
    const long hwcv = HW * CV, total = NB * hwcv;
    hipLaunchKernelGGL(channel_scale_kernel<E>, dim3(grid1d(total, 256)),
                       dim3(256), 0, s, (const T*)x, g, (T*)y, total, hwcv,
                       CV);
}

}  // namespace

namespace defer_hip {

void launch_se_gate(const void* x, const void* w1, const float* b1,
                    const void* w2, const float* b2, float* g, int NB,
                    int HW, int C, int Cr, int act, bool f32,
                    hipStream_t s) {
    if (NB <= 0) return;
    if (f32)
        launch_gate<SeF32>(x, w1, b1, w2, b2, g, NB, HW, C, Cr, act, s);
    else
        launch_gate<SeBf16>(x, w1, b1, w2, b2, g, NB, HW, C, Cr, act, s);
}

void launch_channel_scale(const void* x, const float* g, void* y, long NB,
                          long HW, int C, bool f32, hipStream_t s) {
    if (NB * HW <= 0) return;
    if (f32) launch_scale<SeF32>(x, g, y, NB, HW, C, s);
    else launch_scale<SeBf16>(x, g, y, NB, HW, C, s);
}

}  // namespace defer_hip
