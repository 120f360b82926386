// Layout conversion between the user's NCHW tensors and the NHWC
// activations every kernel of this library works on, with an optional
// fp32 <-> bf16 conversion in the same pass.
//
// Per image both directions are one row-major matrix transpose,
// in[R][Q] -> out[Q][R]: to_nhwc has R = C, Q = H*W, to_nchw R = H*W,
// Q = C. Elements travel as raw bit patterns (u16 for bf16, u32 for
// fp32), so a same-dtype conversion is a pure move; fp32 -> bf16 rounds
// to nearest even in integer arithmetic (bit-identical to torch's
// c10::BFloat16 conversion, denormals and ties included; NaN becomes
// 0x7FC0), bf16 -> fp32 is a 16-bit shift.
//
// Two kernels:
//  * transpose_tile_kernel: a 64x64 tile staged through LDS as one dword
//    per element. Global reads run along Q and global writes along R,
//    16 bytes per lane where the row length is a multiple of the vector
//    width and the base is 16-byte aligned (checked per launch, per
//    side), one element per lane otherwise.
//  * small_c_kernel: C <= 8 (every model's input is C = 1 or 3), where a
//    64-wide tile would idle most lanes. Each thread owns one pixel: C
//    plane accesses (coalesced across the wave) on the NCHW side and C
//    adjacent elements on the NHWC side.
//
// LDS banking (ds_read_b32 / ds_write_b32: bank = dword address % 32,
// conflicts counted per 32-lane half): the tile's row stride is 65 dwords,
// 64 padded by one 4-byte access width. In the vector phases a 32-lane
// half covers V rows x 32/V vectors (V = 4 for fp32, 8 for bf16): for
// element j of its vector, lane (row rr, vector qv) touches dword
// 65*rr + V*qv + j, i.e. bank rr + V*qv + j with rr < V: 32 distinct
// banks. The store phase is the mirror image (65*(V*rv + j) + qq = bank
// V*rv + qq + j mod 32, qq < V). The scalar phases touch 32 consecutive
// dwords of a row, or one column over 32 consecutive rows (bank r + q).
//
// All offsets are 64-bit; blocks walk tiles with a grid stride, so no
// grid dimension depends on the tensor size.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int TILE = 64;
constexpr int LDS_STRIDE = TILE + 1;
constexpr int TPB = 256;
constexpr int SMALL_C_MAX = 8;

template <int BYTES> struct Elem;
template <> struct Elem<2> { typedef unsigned short type; };
template <> struct Elem<4> { typedef u32 type; };

// bit pattern of an IN_B-byte element -> bit pattern of an OUT_B-byte one
template <int IN_B, int OUT_B>
__device__ __forceinline__ u32 cvt_bits(u32 v) {
    if constexpr (IN_B == OUT_B) {
        return v;
    } else if constexpr (IN_B == 2) {
        return v << 16;                         // bf16 -> fp32, exact
    } else {
        if ((v & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;    // NaN
        return (v + 0x7fffu + ((v >> 16) & 1u)) >> 16;          // RNE
    }
}

// the V = 16 / BYTES elements of one 16-byte vector, element e
template <int BYTES>
__device__ __forceinline__ u32 vec_get(const u32x4& v, int e) {
    if constexpr (BYTES == 4) return v[e];
    else return (v[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
}

template <int IN_B, int OUT_B, bool VEC_IN, bool VEC_OUT>
__global__ __launch_bounds__(TPB) void transpose_tile_kernel(
    const void* __restrict__ in_, void* __restrict__ out_, long B, int R,
    int Q, long tiles_r, long tiles_q) {
    typedef typename Elem<IN_B>::type in_t;
    typedef typename Elem<OUT_B>::type out_t;
    __shared__ u32 tile[TILE * LDS_STRIDE];
    const in_t* in = (const in_t*)in_;
    out_t* out = (out_t*)out_;
    const int tid = threadIdx.x;
    const int wave = tid / WAVE, lane = tid % WAVE;
    const int half = lane / 32, l32 = lane % 32;
    const long per_image = tiles_r * tiles_q;
    const long total = B * per_image;
    const long image = (long)R * Q;

    for (long t = blockIdx.x; t < total; t += gridDim.x) {
        const long b = t / per_image;
        const long rem = t - b * per_image;
        const int r0 = (int)(rem / tiles_q) * TILE;
        const int q0 = (int)(rem % tiles_q) * TILE;
        const in_t* src = in + b * image;
        out_t* dst = out + b * image;

        if constexpr (VEC_IN) {
            constexpr int V = 16 / IN_B, HALF = TILE / V / 2;
            const int qv = half * HALF + l32 % HALF;
            const int rr = l32 / HALF;                  // 0 .. V-1
            for (int r = wave * V + rr; r < TILE; r += (TPB / WAVE) * V) {
                const int gr = r0 + r, gq = q0 + qv * V;
                if (gr < R && gq < Q) {                 // Q % V == 0
                    const u32x4 v = *reinterpret_cast<const u32x4*>(
                        src + (long)gr * Q + gq);
#pragma unroll
                    for (int j = 0; j < V; ++j)
                        tile[r * LDS_STRIDE + qv * V + j] =
                            cvt_bits<IN_B, OUT_B>(vec_get<IN_B>(v, j));
                }
            }
        } else {
            for (int i = tid; i < TILE * TILE; i += TPB) {
                const int r = i / TILE, q = i % TILE;
                const int gr = r0 + r, gq = q0 + q;
                if (gr < R && gq < Q)
                    tile[r * LDS_STRIDE + q] =
                        cvt_bits<IN_B, OUT_B>(src[(long)gr * Q + gq]);
            }
        }
        __syncthreads();

        if constexpr (VEC_OUT) {
            constexpr int V = 16 / OUT_B, HALF = TILE / V / 2;
            const int rv = half * HALF + l32 % HALF;
            const int qq = l32 / HALF;                  // 0 .. V-1
            for (int q = wave * V + qq; q < TILE; q += (TPB / WAVE) * V) {
                const int gq = q0 + q, gr = r0 + rv * V;
                if (gq < Q && gr < R) {                 // R % V == 0
                    u32 e[V];
#pragma unroll
                    for (int j = 0; j < V; ++j)
                        e[j] = tile[(rv * V + j) * LDS_STRIDE + q];
                    u32x4 v;
                    if constexpr (OUT_B == 4) {
                        v = u32x4{e[0], e[1], e[2], e[3]};
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            v[k] = (e[2 * k] & 0xffffu) | (e[2 * k + 1] << 16);
                    }
                    *reinterpret_cast<u32x4*>(dst + (long)gq * R + gr) = v;
                }
            }
        } else {
            for (int i = tid; i < TILE * TILE; i += TPB) {
                const int q = i / TILE, r = i % TILE;
                const int gq = q0 + q, gr = r0 + r;
                if (gq < Q && gr < R)
                    dst[(long)gq * R + gr] =
                        (out_t)tile[r * LDS_STRIDE + q];
            }
        }
        __syncthreads();        // the next tile overwrites the staging
    }
}

// C <= SMALL_C_MAX: thread = pixel. TO_NHWC reads C planes and writes C
// adjacent elements; the other direction reads C adjacent elements and
// writes C planes.
template <int IN_B, int OUT_B, bool TO_NHWC>
__global__ __launch_bounds__(TPB) void small_c_kernel(
    const void* __restrict__ in_, void* __restrict__ out_, long pixels,
    long HW, int C) {
    typedef typename Elem<IN_B>::type in_t;
    typedef typename Elem<OUT_B>::type out_t;
    const in_t* in = (const in_t*)in_;
    out_t* out = (out_t*)out_;
    const long stride = (long)gridDim.x * TPB;
    for (long p = (long)blockIdx.x * TPB + threadIdx.x; p < pixels;
         p += stride) {
        const long n = p / HW, hw = p - n * HW;
        const long planar = n * C * HW + hw;    // + c * HW
        const long packed = p * C;              // + c
        u32 v[SMALL_C_MAX];
#pragma unroll
        for (int c = 0; c < SMALL_C_MAX; ++c)
            if (c < C)
                v[c] = cvt_bits<IN_B, OUT_B>(
                    TO_NHWC ? in[planar + c * HW] : in[packed + c]);
#pragma unroll
        for (int c = 0; c < SMALL_C_MAX; ++c)
            if (c < C) {
                if (TO_NHWC) out[packed + c] = (out_t)v[c];
                else out[planar + c * HW] = (out_t)v[c];
            }
    }
}

int grid_for(long work_items, long per_block) {
    long g = (work_items + per_block - 1) / per_block;
    return (int)(g < 65536 ? g : 65536);
}

template <int IN_B, int OUT_B>
void launch_typed(const void* in, void* out, long B, int R, int Q,
                  bool to_nhwc, hipStream_t s) {
    const int C = to_nhwc ? R : Q;
    const long HW = to_nhwc ? Q : R;
    if (C <= SMALL_C_MAX) {
        const long pixels = B * HW;
        const int grid = grid_for(pixels, TPB);
        if (to_nhwc)
            hipLaunchKernelGGL((small_c_kernel<IN_B, OUT_B, true>),
                               dim3(grid), dim3(TPB), 0, s, in, out, pixels,
                               HW, C);
        else
            hipLaunchKernelGGL((small_c_kernel<IN_B, OUT_B, false>),
                               dim3(grid), dim3(TPB), 0, s, in, out, pixels,
                               HW, C);
        return;
    }
    const long tiles_r = (R + TILE - 1) / TILE, tiles_q = (Q + TILE - 1) / TILE;
    const int grid = grid_for(B * tiles_r * tiles_q, 1);
    // 16-byte accesses need every row to start on a 16-byte boundary
    const bool vin = Q % (16 / IN_B) == 0 && (uintptr_t)in % 16 == 0;
    const bool vout = R % (16 / OUT_B) == 0 && (uintptr_t)out % 16 == 0;
#define DEFER_LAYOUT_LAUNCH(VI, VO)                                          \
    hipLaunchKernelGGL((transpose_tile_kernel<IN_B, OUT_B, VI, VO>),         \
                       dim3(grid), dim3(TPB), 0, s, in, out, B, R, Q,        \
                       tiles_r, tiles_q)
    if (vin && vout) DEFER_LAYOUT_LAUNCH(true, true);
    else if (vin) DEFER_LAYOUT_LAUNCH(true, false);
    else if (vout) DEFER_LAYOUT_LAUNCH(false, true);
    else DEFER_LAYOUT_LAUNCH(false, false);
#undef DEFER_LAYOUT_LAUNCH
}

}  // namespace

namespace defer_hip {

void launch_layout(const void* x, void* y, long N, int C, long HW,
                   bool to_nhwc, bool bf16_in, bool bf16_out,
                   hipStream_t s) {
    if (N <= 0 || C <= 0 || HW <= 0) return;
    const int R = to_nhwc ? C : (int)HW, Q = to_nhwc ? (int)HW : C;
    if (bf16_in && bf16_out) launch_typed<2, 2>(x, y, N, R, Q, to_nhwc, s);
    else if (bf16_in) launch_typed<2, 4>(x, y, N, R, Q, to_nhwc, s);
    else if (bf16_out) launch_typed<4, 2>(x, y, N, R, Q, to_nhwc, s);
    else launch_typed<4, 4>(x, y, N, R, Q, to_nhwc, s);
}

}  // namespace defer_hip
