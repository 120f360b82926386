// fp32 versions of the elementwise, concat, pooling and softmax kernels
// (the bf16 ones live in elementwise.hip / pool.hip). Memory-bound:
// loads/stores vectorized 4-wide (16 B/lane), grid-stride loops sized
// <= 2048 blocks. This path exists for accuracy: plain IEEE f32 adds and
// multiplies, the accurate expf, true division.
#include "common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ f32x4 ld4(const float* p) {
    return *reinterpret_cast<const f32x4*>(p);
}
__device__ __forceinline__ void st4(float* p, f32x4 v) {
    *reinterpret_cast<f32x4*>(p) = v;
}

// y = act(x * scale[c] + bias[c]); x [*, C] with C % 4 == 0
__global__ void bn_act_f32_kernel(const float* __restrict__ x,
                                  const float* __restrict__ scale,
                                  const float* __restrict__ bias,
                                  float* __restrict__ y, long total4, int c4,
                                  int act) {
    long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total4; i += stride) {
        int c = (int)(i % c4) * 4;
        f32x4 v = ld4(x + i * 4);
        f32x4 sc = ld4(scale + c), bi = ld4(bias + c), o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[j] = apply_act(v[j] * sc[j] + bi[j], act);
        st4(y + i * 4, o);
    }
}

__global__ void add_act_f32_kernel(const float* __restrict__ a,
                                   const float* __restrict__ b,
                                   float* __restrict__ y, long total4,
                                   int act) {
    long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total4; i += stride) {
        f32x4 va = ld4(a + i * 4), vb = ld4(b + i * 4), o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = apply_act(va[j] + vb[j], act);
        st4(y + i * 4, o);
    }
}

__global__ void relu_f32_kernel(const float* __restrict__ x,
                                float* __restrict__ y, long total4) {
    long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total4; i += stride) {
        f32x4 v = ld4(x + i * 4), o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaxf(v[j], 0.0f);
        st4(y + i * 4, o);
    }
}

__global__ void relu6_f32_kernel(const float* __restrict__ x,
                                 float* __restrict__ y, long total4) {
    long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total4; i += stride) {
        f32x4 v = ld4(x + i * 4), o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fminf(fmaxf(v[j], 0.0f), 6.0f);
        st4(y + i * 4, o);
    }
}

__global__ void hardswish_f32_kernel(const float* __restrict__ x,
                                     float* __restrict__ y, long total4) {
    long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long stride = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total4; i += stride) {
        f32x4 v = ld4(x + i * 4), o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = hardswish_f(v[j]);
        st4(y + i * 4, o);
    }
}

// Row softmax: one wave per row, arbitrary ncols, accurate expf.
__global__ void softmax_f32_kernel(const float* __restrict__ x,
                                   float* __restrict__ y, int rows,
                                   int cols) {
    int row = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    int lane = threadIdx.x % WAVE;
    if (row >= rows) return;
    const float* xr = x + (long)row * cols;
    float m = -INFINITY;
    for (int c = lane; c < cols; c += WAVE) m = fmaxf(m, xr[c]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        m = fmaxf(m, __shfl_xor(m, off));
    float s = 0.f;
    for (int c = lane; c < cols; c += WAVE) s += expf(xr[c] - m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    float* yr = y + (long)row * cols;
    for (int c = lane; c < cols; c += WAVE) yr[c] = expf(xr[c] - m) / s;
}

// Two-input NHWC channel concat; c1, c2 in float4 chunks.
__global__ void cat2_f32_kernel(const float* __restrict__ a,
                                const float* __restrict__ b,
                                float* __restrict__ y, long rows, int c1_4,
                                int c2_4) {
    const int ct4 = c1_4 + c2_4;
    long total = rows * ct4;
    long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long gstride = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total; i += gstride) {
        long r = i / ct4;
        int c4 = (int)(i % ct4);
        f32x4 v = (c4 < c1_4) ? ld4(a + (r * c1_4 + c4) * 4)
                              : ld4(b + (r * c2_4 + (c4 - c1_4)) * 4);
        st4(y + i * 4, v);
    }
}

// max / mean over the window's valid taps; one lane handles 4 channels
// of one output pixel. AVG divides by the valid-tap count
// (count_include_pad=False).
template <bool AVG>
__global__ void pool_f32_kernel(const float* __restrict__ x,
                                float* __restrict__ y, int N, int H, int W,
                                int C, int OH, int OW, int k, int stride,
                                int pad) {
    const int c4n = C / 4;
    long total = (long)N * OH * OW * c4n;
    long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long gstride = (long)gridDim.x * blockDim.x;
    for (long i = i0; i < total; i += gstride) {
        int c4 = (int)(i % c4n);
        long p = i / c4n;
        int ow = (int)(p % OW);
        long q = p / OW;
        int oh = (int)(q % OH);
        int n = (int)(q / OH);
        f32x4 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = AVG ? 0.f : -INFINITY;
        int cnt = 0;
        int ih0 = oh * stride - pad, iw0 = ow * stride - pad;
        for (int r = 0; r < k; ++r) {
            int ih = ih0 + r;
            if (ih < 0 || ih >= H) continue;
            for (int s = 0; s < k; ++s) {
                int iw = iw0 + s;
                if (iw < 0 || iw >= W) continue;
                f32x4 v = ld4(x + (((long)n * H + ih) * W + iw) * C + c4 * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[j] = AVG ? acc[j] + v[j] : fmaxf(acc[j], v[j]);
                ++cnt;
            }
        }
        if (AVG) {
            float d = cnt > 0 ? (float)cnt : 1.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = acc[j] / d;
        }
        st4(y + i * 4, acc);
    }
}

// [N, H, W, C] -> [N, C]; one workgroup per (n, c-block of 1024), each
// lane averages its own 4 channels over all H*W pixels in pixel order.
__global__ void gap_f32_kernel(const float* __restrict__ x,
                               float* __restrict__ y, int N, int HW, int C) {
    int cblk = (C + 1023) / 1024;
    int n = blockIdx.x / cblk;
    int cb = blockIdx.x % cblk;
    int c = cb * 1024 + threadIdx.x * 4;
    if (n >= N || c >= C) return;
    const float* xn = x + (long)n * HW * C + c;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < HW; ++p) acc = acc + ld4(xn + (long)p * C);
    float d = (float)HW;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = acc[j] / d;
    st4(y + (long)n * C + c, acc);
}

int grid1d(long work, int block) {
    long g = (work + block - 1) / block;
    return (int)(g < 2048 ? g : 2048);
}

}  // namespace

namespace defer_hip {

void launch_bn_act_f32(const float* x, const float* scale, const float* bias,
                       float* y, long total4, int c4, bool relu,
                       hipStream_t s) {
    hipLaunchKernelGGL(bn_act_f32_kernel, dim3(grid1d(total4, 256)),
                       dim3(256), 0, s, x, scale, bias, y, total4, c4,
                       relu ? ACT_RELU : ACT_NONE);
}

void launch_add_act_f32(const float* a, const float* b, float* y,
                        long total4, bool relu, hipStream_t s) {
    hipLaunchKernelGGL(add_act_f32_kernel, dim3(grid1d(total4, 256)),
                       dim3(256), 0, s, a, b, y, total4,
                       relu ? ACT_RELU : ACT_NONE);
}

void launch_relu_f32(const float* x, float* y, long total4, hipStream_t s) {
    hipLaunchKernelGGL(relu_f32_kernel, dim3(grid1d(total4, 256)), dim3(256),
                       0, s, x, y, total4);
}

void launch_relu6_f32(const float* x, float* y, long total4, hipStream_t s) {
    hipLaunchKernelGGL(relu6_f32_kernel, dim3(grid1d(total4, 256)),
                       dim3(256), 0, s, x, y, total4);
}

void launch_hardswish_f32(const float* x, float* y, long total4,
                          hipStream_t s) {
    hipLaunchKernelGGL(hardswish_f32_kernel, dim3(grid1d(total4, 256)),
                       dim3(256), 0, s, x, y, total4);
}

void launch_cat2_f32(const float* a, const float* b, float* y, long rows,
                     int c1, int c2, hipStream_t s) {
    long total = rows * ((c1 + c2) / 4);
    hipLaunchKernelGGL(cat2_f32_kernel, dim3(grid1d(total, 256)), dim3(256),
                       0, s, a, b, y, rows, c1 / 4, c2 / 4);
}

void launch_softmax_f32(const float* x, float* y, int rows, int cols,
                        hipStream_t s) {
    int wpb = 4;
    int blocks = (rows + wpb - 1) / wpb;
    hipLaunchKernelGGL(softmax_f32_kernel, dim3(blocks), dim3(wpb * 64), 0,
                       s, x, y, rows, cols);
}

void launch_maxpool_f32(const float* x, float* y, int NB, int H, int W,
                        int C, int OH, int OW, int k, int stride, int pad,
                        hipStream_t s) {
    long total = (long)NB * OH * OW * (C / 4);
    hipLaunchKernelGGL(pool_f32_kernel<false>, dim3(grid1d(total, 256)),
                       dim3(256), 0, s, x, y, NB, H, W, C, OH, OW, k, stride,
                       pad);
}

void launch_avgpool_f32(const float* x, float* y, int NB, int H, int W,
                        int C, int OH, int OW, int k, int stride, int pad,
                        hipStream_t s) {
    long total = (long)NB * OH * OW * (C / 4);
    hipLaunchKernelGGL(pool_f32_kernel<true>, dim3(grid1d(total, 256)),
                       dim3(256), 0, s, x, y, NB, H, W, C, OH, OW, k, stride,
                       pad);
}

void launch_gap_f32(const float* x, float* y, int NB, int HW, int C,
                    hipStream_t s) {
    int cblk = (C + 1023) / 1024;
    hipLaunchKernelGGL(gap_f32_kernel, dim3(NB * cblk), dim3(256), 0, s, x,
                       y, NB, HW, C);
}

}  // namespace defer_hip
