// Common device helpers for defer_amd gfx950 (CDNA4) kernels.
//
// All kernels in this library are written for MI355X only: wave64,
// MFMA bf16 (16x16x32), 160 KiB LDS per CU, NHWC activations.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define WAVE 64

typedef __bf16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned char u8;
typedef unsigned int u32;
typedef unsigned long long u64;
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf2f(bf16 v) { return (float)v; }
__device__ __forceinline__ bf16 f2bf(float v) { return (bf16)v; }

// Load 8 bf16 (16 B) as one vector
__device__ __forceinline__ bf16x8 load_bf16x8(const bf16* p) {
    return *reinterpret_cast<const bf16x8*>(p);
}
__device__ __forceinline__ void store_bf16x8(bf16* p, bf16x8 v) {
    *reinterpret_cast<bf16x8*>(p) = v;
}

__device__ __forceinline__ int cdiv(int a, int b) { return (a + b - 1) / b; }

#define MFMA_BF16_16x16x32(a, b, c) \
    __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

// activation codes
// (ACT_RELU6 is a runtime value of the depthwise and fp32 conv kernels and
// of the bindings; the bf16 conv templates take ACT_RELU with a bound for
// it, and ACT_NONE, ACT_RELU or ACT_HARDSWISH as their ACT)
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_RELU6 = 2, ACT_HARDSWISH = 3 };

// hardsigmoid(v) = min(max(v + 3, 0), 6) * (1/6), hardswish(v) = v * that,
// in this order everywhere (ops/reference.py too): 6 * c6 and 3 * c6 round
// to exactly 1 and 0.5, so hardswish returns v bit for bit for v >= 3 and 0
// for v <= -3. No division and no fma: there is no product feeding a sum.
__device__ __forceinline__ float hardsigmoid_f(float v) {
    return fminf(fmaxf(v + 3.0f, 0.0f), 6.0f) * (1.0f / 6.0f);
}
__device__ __forceinline__ float hardswish_f(float v) {
    return v * hardsigmoid_f(v);
}

__device__ __forceinline__ float apply_act(float v, int act) {
    return act == ACT_RELU ? fmaxf(v, 0.0f) : v;
}

// The bf16 conv epilogues: ACT_RELU clamps to [0, hi]. hi = +inf is the
// plain ReLU (min(v, +inf) == v, so the bits are those of apply_act) and
// hi = 6 is ReLU6, without a third template value per kernel. ACT_HARDSWISH
// is a template value of its own: as a runtime flag inside the ReLU
// instantiations it cost ResNet50 2.5 % (docs/OPTIMIZATION_LOG.md). act is a
// compile-time constant at every call, so the ReLU and no-activation
// instantiations are what they were.
__device__ __forceinline__ float apply_act_hi(float v, int act, float hi) {
    if (act == ACT_HARDSWISH) return hardswish_f(v);
    return act == ACT_RELU ? fminf(fmaxf(v, 0.0f), hi) : v;
}
