// What the torch entry points of every kernel family share (host only):
// argument checks, the process-wide buffers and the launch counters. The
// families are entry_*.cpp, one `bind_<family>(m)` each; bindings.cpp calls
// them. A new op's entry goes into its family's file and takes its checks
// from here.
#pragma once

// ATen and the Tensor casters of pybind11, not all of torch/extension.h:
// every family file pays for this include once
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <torch/csrc/utils/pybind.h>

#include <cstdint>
#include <functional>
#include <mutex>

#include "kernels.h"

namespace defer_bind {

using at::Tensor;

inline hipStream_t cur_stream() {
    return at::cuda::getCurrentHIPStream().stream();
}

inline const void* bptr(const Tensor& t) { return t.data_ptr(); }
inline void* bptr_mut(Tensor& t) { return t.data_ptr(); }
inline const float* f32ptr(const Tensor& t) { return t.data_ptr<float>(); }
inline bool aligned16(const Tensor& t) {
    return (uintptr_t)t.data_ptr() % 16 == 0;
}

// ---- dtype checks ----
// on the GPU, bf16, contiguous (alignment is not asked for)
void check_bf16(const Tensor& t, const char* name);
// on the GPU, fp32, contiguous, 16-byte aligned
void check_f32(const Tensor& t, const char* name);
// on the GPU, e4m3, contiguous, 16-byte aligned
void check_e4m3(const Tensor& t, const char* name);
// dtype dispatch of the entry points: true = the fp32 launchers, false =
// the bf16 ones; every other dtype raises
bool is_f32(const Tensor& t, const char* name);
// check_f32 or check_bf16 by `f32`; `aligned` asks 16 bytes of bf16 too
void check_as(const Tensor& t, const char* name, bool f32, bool aligned);
// an operand in either compute dtype: is_f32 + check_as, returns f32
bool check_dtype(const Tensor& t, const char* name, bool aligned = false);
// x and w share bf16 or fp32: check_dtype(x) + check_as(w), returns f32
bool check_pair(const Tensor& x, const Tensor& w, const char* wname,
                bool aligned);
// `value` (an op's numel or C, named by `what`) is a multiple of one 16-byte
// vector of the dtype: 4 fp32 or 8 bf16. Returns that count.
int check_vec(int64_t value, bool f32, const char* op, const char* what);
// x of the channel-vector ops: either dtype, contiguous, 16-byte aligned, C
// a positive multiple of one vector. Returns true for fp32.
bool check_channel_vec(const Tensor& x, const char* op);

// act is one of ACT_NONE .. ACT_HARDSWISH (kernels.h)
void check_act(int64_t act);

// The pooling geometry both dtypes accept, which is what F.max_pool2d
// accepts.
void check_pool(const Tensor& x, int64_t kernel, int64_t stride, int64_t pad,
                const char* op);

// ---- fp32[n] scale / bias / parameter vectors ----
// A present vector is fp32, contiguous, on x's device and of n values;
// `aligned` adds 16-byte alignment and `rank1` dim() == 1.
struct VecReq {
    bool aligned = false, rank1 = false;
};
const float* f32_vec(const Tensor& t, const Tensor& x, const char* op,
                     const char* name, int64_t n, VecReq req = {});
// The optional form. Absent means `absent`: null where the kernel takes a
// null pointer, ones_buf() or zeros_buf() where it does not, and then n is
// bound by that buffer's 8192 values.
const float* f32_vec(const c10::optional<Tensor>& t, const float* absent,
                     const Tensor& x, const char* op, const char* name,
                     int64_t n, VecReq req = {});

// ---- conv output geometry ----
struct ConvOut {
    int64_t OH, OW, M;      // M = NB * OH * OW
};
// (H + 2 pad - R) / stride + 1 and its refusals: a kernel larger than the
// padded input, M of 2^31 or more and, with `elems32` (kernels whose element
// offsets are 32-bit), x [NB, H, W, Cin] or out [M, Cout] of 2^31 or more
// elements.
ConvOut conv_out_geom(int64_t NB, int64_t H, int64_t W, int64_t Cin,
                      int64_t Cout, int64_t R, int64_t S, int64_t stride,
                      int64_t pad, bool elems32);

// ---- process-wide buffers (one each, whatever the translation unit) ----
// 16 B of zeros: the source of out-of-bounds global_load_lds lanes
const void* zero_buf();
// scale / bias must be non-null in the bf16 kernels (nullable per-element
// loads de-pipeline the epilogue): 8192 cached ones / zeros when absent
constexpr int64_t kCachedVec = 8192;
const float* ones_buf();
const float* zeros_buf();

// Prepared-weight cache (K-order repack, channel pad, fp32 bias): weights
// are constant in inference, so the one-time transform is keyed on
// (data_ptr, numel, variant). See entry_util.cpp.
Tensor cached_weight_prep(const Tensor& w, int64_t variant,
                          const std::function<Tensor()>& make);

// What a kernel with a launch policy did, for tests: its launches in this
// process and up to two named integers of the last one.
class LaunchStats {
  public:
    LaunchStats(const char* name0, const char* name1 = nullptr)
        : names_{name0, name1} {}
    void record(int64_t v0, int64_t v1 = 0);
    py::dict to_dict();     // {"launches", name0[, name1]}

  private:
    const char* names_[2];
    std::mutex mu_;
    int64_t launches_ = 0, v_[2] = {0, 0};
};

// bf16 max-pool entry (entry_pointwise.cpp); conv_bn_act_maxpool composes it
Tensor maxpool2d(Tensor x, int64_t kernel, int64_t stride, int64_t pad);

}  // namespace defer_bind

// one per family file, called by PYBIND11_MODULE in this order
void bind_conv(py::module_& m);
void bind_dwconv(py::module_& m);
void bind_pointwise(py::module_& m);
void bind_attention(py::module_& m);
void bind_fp8(py::module_& m);
void bind_codec(py::module_& m);
