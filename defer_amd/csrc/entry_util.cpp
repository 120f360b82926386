// The shared half of the torch bindings: see entry_util.h.
#include "entry_util.h"

#include <unordered_map>

namespace defer_bind {

void check_bf16(const Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

void check_f32(const Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.scalar_type() == at::kFloat, name,
                " must be fp32 like x (mixed dtypes)");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(aligned16(t), name, " must be 16-byte aligned");
}

void check_e4m3(const Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.scalar_type() == at::kFloat8_e4m3fn, name,
                " must be torch.float8_e4m3fn");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(aligned16(t), name, " must be 16-byte aligned");
}

bool is_f32(const Tensor& t, const char* name) {
    if (t.scalar_type() == at::kBFloat16) return false;
    TORCH_CHECK(t.scalar_type() == at::kFloat, name,
                " must be bf16 or fp32");
    return true;
}

void check_as(const Tensor& t, const char* name, bool f32, bool aligned) {
    if (f32) return check_f32(t, name);
    check_bf16(t, name);
    TORCH_CHECK(!aligned || aligned16(t), name, " must be 16-byte aligned");
}

bool check_dtype(const Tensor& t, const char* name, bool aligned) {
    const bool f32 = is_f32(t, name);
    check_as(t, name, f32, aligned);
    return f32;
}

bool check_pair(const Tensor& x, const Tensor& w, const char* wname,
                bool aligned) {
    const bool f32 = check_dtype(x, "x", aligned);
    check_as(w, wname, f32, aligned);
    return f32;
}

int check_vec(int64_t value, bool f32, const char* op, const char* what) {
    const int vec = f32 ? 4 : 8;
    TORCH_CHECK(value % vec == 0, f32 ? "fp32 " : "bf16 ", op, " needs ",
                what, " % ", vec, " == 0, got ", value);
    return vec;
}

bool check_channel_vec(const Tensor& x, const char* op) {
    const bool f32 = is_f32(x, "x");
    TORCH_CHECK(x.is_cuda(), op, ": x must be on GPU");
    TORCH_CHECK(x.is_contiguous(), op, ": x must be contiguous");
    TORCH_CHECK(aligned16(x), op, ": x must be 16-byte aligned");
    const int vec = f32 ? 4 : 8;
    const int64_t C = x.size(-1);
    TORCH_CHECK(C > 0 && C % vec == 0, op, ": ", f32 ? "fp32" : "bf16",
                " needs C % ", vec, " == 0 (16-byte channel vectors), got "
                "C = ", C);
    return f32;
}

void check_act(int64_t act) {
    TORCH_CHECK(act >= ACT_NONE && act <= ACT_HARDSWISH,
                "act must be 0 (none), 1 (relu), 2 (relu6) or 3 (hardswish), "
                "got ", act);
}

// a stride of 0 would divide by zero in the caller, and with
// pad > kernel / 2 a border window has no tap
void check_pool(const Tensor& x, int64_t kernel, int64_t stride, int64_t pad,
                const char* op) {
    TORCH_CHECK(x.dim() == 4, "x must be NHWC");
    TORCH_CHECK(kernel >= 1, op, ": kernel must be >= 1, got ", kernel);
    TORCH_CHECK(stride >= 1, op, ": stride must be >= 1, got ", stride);
    TORCH_CHECK(pad >= 0 && pad <= kernel / 2, op,
                ": pad must be in [0, kernel / 2], got pad ", pad,
                " for kernel ", kernel);
    TORCH_CHECK(x.size(1) + 2 * pad >= kernel &&
                x.size(2) + 2 * pad >= kernel, op, ": input ", x.size(1),
                "x", x.size(2), " with pad ", pad,
                " is smaller than the window ", kernel);
}

const float* f32_vec(const Tensor& t, const Tensor& x, const char* op,
                     const char* name, int64_t n, VecReq req) {
    TORCH_CHECK(t.device() == x.device() && t.scalar_type() == at::kFloat &&
                t.is_contiguous() && t.numel() == n &&
                (!req.rank1 || t.dim() == 1) &&
                (!req.aligned || aligned16(t)),
                op, ": ", name, " must be a contiguous",
                req.aligned ? ", 16-byte aligned" : "",
                req.rank1 ? " 1-D" : "", " fp32[C] on x's device with C = ",
                n);
    return t.data_ptr<float>();
}

const float* f32_vec(const c10::optional<Tensor>& t, const float* absent,
                     const Tensor& x, const char* op, const char* name,
                     int64_t n, VecReq req) {
    if (t) return f32_vec(*t, x, op, name, n, req);
    TORCH_CHECK(!absent || n <= kCachedVec, op, " without ", name,
                " takes at most C = ", kCachedVec, ", got ", n);
    return absent;
}

ConvOut conv_out_geom(int64_t NB, int64_t H, int64_t W, int64_t Cin,
                      int64_t Cout, int64_t R, int64_t S, int64_t stride,
                      int64_t pad, bool elems32) {
    TORCH_CHECK(H + 2 * pad >= R && W + 2 * pad >= S,
                "kernel larger than the padded input");
    ConvOut g;
    g.OH = (H + 2 * pad - R) / stride + 1;
    g.OW = (W + 2 * pad - S) / stride + 1;
    g.M = NB * g.OH * g.OW;
    TORCH_CHECK(g.M < (1LL << 31), "M too large");
    if (elems32) {
        TORCH_CHECK(NB * H * W * Cin < (1LL << 31),
                    "x has 2^31 or more elements");
        TORCH_CHECK(g.M * Cout < (1LL << 31),
                    "out has 2^31 or more elements");
    }
    return g;
}

const void* zero_buf() {
    static Tensor z = at::zeros(
        {16}, at::TensorOptions().dtype(at::kBFloat16).device(at::kCUDA));
    return bptr(z);
}

const float* ones_buf() {
    static Tensor t = at::ones(
        {kCachedVec}, at::TensorOptions().dtype(at::kFloat).device(at::kCUDA));
    return t.data_ptr<float>();
}
const float* zeros_buf() {
    static Tensor t = at::zeros(
        {kCachedVec}, at::TensorOptions().dtype(at::kFloat).device(at::kCUDA));
    return t.data_ptr<float>();
}

// The reference pays its weight prep once at dispatch too (node.py:34).
// The SOURCE tensor is pinned in the entry: the caching allocator would
// otherwise reuse a freed weight's pointer for a different model's
// same-shaped weights and the key would collide with stale data (observed
// as a flaky cross-test mismatch). Unbounded but tiny (one entry per
// prepared weight).
struct PrepEntry {
    Tensor src;       // pinning src keeps its pointer unique
    Tensor prepped;
    uint32_t version; // src._version at prep time: in-place mutation of
                      // the source weight (e.g. checkpoint reload into
                      // the same tensors) bumps it and invalidates the
                      // cached repack
};

Tensor cached_weight_prep(const Tensor& w, int64_t variant,
                          const std::function<Tensor()>& make) {
    static std::unordered_map<uint64_t, PrepEntry> cache;
    static std::mutex mu;
    uint64_t key = (uint64_t)(uintptr_t)w.data_ptr() * 31 +
                   (uint64_t)w.numel() * 7 + (uint64_t)variant;
    uint32_t ver = w.unsafeGetTensorImpl()->version_counter().current_version();
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find(key);
    if (it != cache.end() &&
        it->second.src.data_ptr() == w.data_ptr() &&
        it->second.src.numel() == w.numel() &&
        it->second.version == ver)
        return it->second.prepped;
    Tensor t = make();
    cache[key] = {w, t, ver};
    return t;
}

void LaunchStats::record(int64_t v0, int64_t v1) {
    std::lock_guard<std::mutex> g(mu_);
    ++launches_;
    v_[0] = v0;
    v_[1] = v1;
}

py::dict LaunchStats::to_dict() {
    std::lock_guard<std::mutex> g(mu_);
    py::dict d;
    d["launches"] = launches_;
    for (int i = 0; i < 2 && names_[i]; ++i) d[names_[i]] = v_[i];
    return d;
}

}  // namespace defer_bind
