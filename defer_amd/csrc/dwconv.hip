// Depthwise convolution + folded BN + activation, NHWC, bf16 and fp32
// (MobileNetV2's 3x3 depthwise layers; 5x5 for the MNASNet family):
//
//   y[n][oh][ow][c] = act(scale[c] * sum_{r,s} x[n][oh*st-pad+r][ow*st-pad+s][c]
//                                              * w[r][s][c] + bias[c])
//
// There is no reduction over channels, so K is 9 or 25 and this is a VALU
// kernel bound by memory, not an MFMA one. The lane mapping is the pools'
// (pool.hip): channels are the fast dim of x, w and y, one lane owns one
// 16-byte channel vector (8 bf16 or 4 fp32) and neighbouring lanes take the
// neighbouring channel vectors, then the neighbouring output columns, so a
// wave's loads and stores are contiguous runs.
//
// Register reuse: a lane walks a vertical strip of TH output rows of its
// column. It loads every input row of the strip once (R vectors, unpacked
// to fp32 once) and adds it into each of the <= ceil(R/stride) output rows
// it is a tap row of, so an input vector is fetched (TH-1)*stride+R times
// per TH outputs instead of R*R times per output; the horizontal overlap
// between neighbouring columns is left to L1. Input rows arrive in rising
// order, so every output accumulates its taps in the fixed order (r, then
// s) by fmaf in fp32 with one rounding at the end: no atomics, no split,
// run-to-run identical. Taps in the zero padding are computed as x = 0.
//
// The 3x3 weights of a lane stay unpacked in registers across the strip and
// across grid-stride steps that keep the lane's channels; the 5x5 ones
// (25 x 8 fp32 would not fit) are re-read at use, from L1, and a 5x5 strip
// is 2 rows where a 3x3 one is 4.
// Every loop over taps and strip rows has constant bounds and is unrolled,
// so all arrays are registers (no scratch). One template serves both
// dtypes: dwconv_kernel<DwBf16, R, stride> and dwconv_kernel<DwF32, ...>.
#include "common.h"
#include "kernels.h"

namespace {

// output rows per lane: the accumulators of a strip, the unpacked taps of
// one input row and the weights must all fit in registers
constexpr int dw_th(int R) { return R == 3 ? 4 : 2; }
constexpr int DW_TPB = 256;

struct DwBf16 {
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

struct DwF32 {
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

template <typename E, int R, int ST>
__global__ __launch_bounds__(DW_TPB) void dwconv_kernel(
    const typename E::T* __restrict__ x, const typename E::T* __restrict__ w,
    const float* __restrict__ scale, const float* __restrict__ bias,
    typename E::T* __restrict__ y, int N, int H, int W, int C, int OH,
    int OW, int pad, int act) {
    typedef typename E::Vec Vec;
    constexpr int V = E::V;
    constexpr int DW_TH = dw_th(R);
    constexpr int ROWS = (DW_TH - 1) * ST + R;   // input rows of a strip
    constexpr bool W_REGS = R == 3;
    constexpr int Q_UNROLL = W_REGS ? ROWS : 1;

    const int CV = C / V;
    const int NS = (OH + DW_TH - 1) / DW_TH;     // strips per column
    const long total = (long)N * NS * OW * CV;
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long gstride = (long)gridDim.x * blockDim.x;

    float wf[W_REGS ? R * R : 1][V];
    float sc[V], bi[V];
    int cur_cv = -1;

    for (long i = i0; i < total; i += gstride) {
        const int cv = (int)(i % CV);
        long t = i / CV;
        const int ow = (int)(t % OW);
        t /= OW;
        const int oh0 = (int)(t % NS) * DW_TH;
        const int n = (int)(t / NS);
        const int c = cv * V;

        if (cv != cur_cv) {
            cur_cv = cv;
            if constexpr (W_REGS) {
#pragma unroll
                for (int k = 0; k < R * R; ++k) {
                    Vec v = *reinterpret_cast<const Vec*>(
                        w + (long)k * C + c);
#pragma unroll
                    for (int j = 0; j < V; ++j) wf[k][j] = E::get(v, j);
                }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                sc[j] = scale[c + j];
                bi[j] = bias[c + j];
            }
        }

        float acc[DW_TH][V];
#pragma unroll
        for (int o = 0; o < DW_TH; ++o)
#pragma unroll
            for (int j = 0; j < V; ++j) acc[o][j] = 0.0f;

        const int ih0 = oh0 * ST - pad, iw0 = ow * ST - pad;
        const typename E::T* xn = x + (long)n * H * W * C + c;
        // one input row: R channel vectors, zeros where the tap lies in
        // the padding. Branch-free: such a tap loads the nearest pixel of
        // the image (always in bounds, H, W >= 1) and drops the value.
        auto load_row = [&](int q, Vec (&dst)[R]) {
            const int ih = ih0 + q;
            const bool row_ok = ih >= 0 && ih < H;
            const int ihc = min(max(ih, 0), H - 1);
#pragma unroll
            for (int s = 0; s < R; ++s) {
                const int iw = iw0 + s;
                const bool ok = row_ok && iw >= 0 && iw < W;
                const int iwc = min(max(iw, 0), W - 1);
                Vec v = *reinterpret_cast<const Vec*>(
                    xn + ((long)ihc * W + iwc) * C);
#pragma unroll
                for (int j = 0; j < V; ++j)
                    E::set(dst[s], j, ok ? E::get(v, j) : 0.0f);
            }
        };
        // the loads run one row ahead of the arithmetic; the scheduling
        // barriers keep the compiler from hoisting every row's loads to
        // the top, which costs more registers than the kernel has
        Vec raw[R], nxt[R];
        load_row(0, raw);
        // 3x3: unrolled, so the tap row r of every output is a constant
        // and indexes the weight registers. 5x5: a real loop, r is a
        // number and its weights are re-read, which also keeps the
        // compiler from gathering all 25 vectors in registers.
#pragma unroll Q_UNROLL
        for (int q = 0; q < ROWS; ++q) {
            if (q + 1 < ROWS) load_row(q + 1, nxt);
            __builtin_amdgcn_sched_barrier(0);
            float xf[R][V];
#pragma unroll
            for (int s = 0; s < R; ++s)
#pragma unroll
                for (int j = 0; j < V; ++j) xf[s][j] = E::get(raw[s], j);
#pragma unroll
            for (int o = 0; o < DW_TH; ++o) {
                const int r = q - o * ST;        // tap row of output o
                if (r < 0 || r >= R) continue;
#pragma unroll
                for (int s = 0; s < R; ++s) {
                    Vec wv;
                    if constexpr (!W_REGS)
                        wv = *reinterpret_cast<const Vec*>(
                            w + (long)(r * R + s) * C + c);
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        float wj;
                        if constexpr (W_REGS) wj = wf[r * R + s][j];
                        else wj = E::get(wv, j);
                        acc[o][j] = fmaf(xf[s][j], wj, acc[o][j]);
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < R; ++s) raw[s] = nxt[s];
            __builtin_amdgcn_sched_barrier(0);
        }

#pragma unroll
        for (int o = 0; o < DW_TH; ++o) {
            const int oh = oh0 + o;
            if (oh >= OH) continue;
            Vec out;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float v = fmaf(acc[o][j], sc[j], bi[j]);
                if (act == ACT_HARDSWISH) {
                    v = hardswish_f(v);
                } else {
                    if (act != ACT_NONE) v = fmaxf(v, 0.0f);
                    if (act == ACT_RELU6) v = fminf(v, 6.0f);
                }
                E::set(out, j, v);
            }
            *reinterpret_cast<Vec*>(
                y + (((long)n * OH + oh) * OW + ow) * C + c) = out;
        }
    }
}

template <typename E>
void launch_dw(const void* x, const void* w, const float* scale,
               const float* bias, void* y, int NB, int H, int W, int C,
               int OH, int OW, int R, int stride, int pad, int act,
               hipStream_t s) {
    typedef typename E::T T;
    const int NS = (OH + dw_th(R) - 1) / dw_th(R);
    const long total = (long)NB * NS * OW * (C / E::V);
    if (total <= 0) return;
    long g = (total + DW_TPB - 1) / DW_TPB;
    // enough blocks for every CU at the kernel's occupancy; the rest of the
    // work is the grid-stride loop's
    const int grid = (int)(g < 4096 ? g : 4096);
    typedef void (*Kernel)(const T*, const T*, const float*, const float*,
                           T*, int, int, int, int, int, int, int, int);
    static const Kernel kernel[2][2] = {
        {dwconv_kernel<E, 3, 1>, dwconv_kernel<E, 3, 2>},
        {dwconv_kernel<E, 5, 1>, dwconv_kernel<E, 5, 2>}};
    hipLaunchKernelGGL(kernel[R == 5][stride == 2], dim3(grid),
                       dim3(DW_TPB), 0, s, (const T*)x, (const T*)w, scale,
                       bias, (T*)y, NB, H, W, C, OH, OW, pad, act);
}

}  // namespace

namespace defer_hip {

void launch_dwconv(const void* x, const void* w, const float* scale,
                   const float* bias, void* y, int NB, int H, int W, int C,
                   int OH, int OW, int R, int stride, int pad, int act,
                   hipStream_t s) {
    launch_dw<DwBf16>(x, w, scale, bias, y, NB, H, W, C, OH, OW, R, stride,
                      pad, act, s);
}

void launch_dwconv_f32(const float* x, const float* w, const float* scale,
                       const float* bias, float* y, int NB, int H, int W,
                       int C, int OH, int OW, int R, int stride, int pad,
                       int act, hipStream_t s) {
    launch_dw<DwF32>(x, w, scale, bias, y, NB, H, W, C, OH, OW, R, stride,
                     pad, act, s);
}

}  // namespace defer_hip
