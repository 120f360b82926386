// Torch bindings for the defer_amd gfx950 kernel library.
//
// Host-only TU: checks device/dtype/contiguity and calls the launchers in
// the .hip TUs on the current HIP stream, so ops compose with torch.cuda
// streams and hipGraph capture.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cmath>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <string>
#include <unordered_map>

#include "conv_plan.h"
#include "kernels.h"

namespace {

using at::Tensor;
using defer_hip::ConvParams;

hipStream_t cur_stream() {
    return at::cuda::getCurrentHIPStream().stream();
}

const void* bptr(const Tensor& t) { return t.data_ptr(); }
void* bptr_mut(Tensor& t) { return t.data_ptr(); }

void check_bf16(const Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// dtype dispatch for the op entry points: true = the fp32 launchers,
// false = the bf16 ones; every other dtype raises.
bool is_f32(const Tensor& t, const char* name) {
    if (t.scalar_type() == at::kBFloat16) return false;
    TORCH_CHECK(t.scalar_type() == at::kFloat, name,
                " must be bf16 or fp32");
    return true;
}

void check_f32(const Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
    TORCH_CHECK(t.scalar_type() == at::kFloat, name,
                " must be fp32 like x (mixed dtypes)");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0, name,
                " must be 16-byte aligned");
}

const float* f32ptr(const Tensor& t) { return t.data_ptr<float>(); }

// The pooling geometry both dtypes accept, which is what F.max_pool2d
// accepts: a stride of 0 would divide by zero below, and with
// pad > kernel / 2 a border window has no tap.
void check_pool(const Tensor& x, int64_t kernel, int64_t stride,
                int64_t pad, const char* op) {
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

// activation codes of the ops that know ReLU6 and hardswish (ACT_* of
// csrc/common.h); C++ callers that pass a bool get none / relu
enum { kActNone = 0, kActRelu = 1, kActRelu6 = 2, kActHardswish = 3 };

void check_act(int64_t act) {
    TORCH_CHECK(act >= kActNone && act <= kActHardswish,
                "act must be 0 (none), 1 (relu), 2 (relu6) or 3 (hardswish), "
                "got ", act);
}

// 16B zero source for OOB global_load_lds lanes, one per process
const void* zero_buf() {
    static Tensor z = at::zeros(
        {16}, at::TensorOptions().dtype(at::kBFloat16).device(at::kCUDA));
    return bptr(z);
}

// scale/bias must be non-null in the kernel (nullable per-element loads
// de-pipeline the epilogue); substitute cached ones/zeros when absent.
const float* ones_buf() {
    static Tensor t = at::ones(
        {8192}, at::TensorOptions().dtype(at::kFloat).device(at::kCUDA));
    return t.data_ptr<float>();
}
const float* zeros_buf() {
    static Tensor t = at::zeros(
        {8192}, at::TensorOptions().dtype(at::kFloat).device(at::kCUDA));
    return t.data_ptr<float>();
}

// Prepared-weight cache for the stem paths (K-order repack / channel
// pad). Weights are constant in inference, so the one-time transform is
// keyed on (data_ptr, numel, variant) — the reference pays its weight
// prep once at dispatch too (node.py:34). The SOURCE tensor is pinned
// in the entry: the caching allocator would otherwise reuse a freed
// weight's pointer for a different model's same-shaped weights and the
// key would collide with stale data (observed as a flaky cross-test
// mismatch). Unbounded but tiny (one entry per stem conv weight);
// in-place weight mutation is not detected (inference engine — the
// reference also ships weights exactly once, dispatcher.py:57).
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

const float* fptr_opt(const c10::optional<Tensor>& t, const char* name,
                      const float* fallback, int64_t n) {
    if (!t) {
        TORCH_CHECK(n <= 8192, "Cout too large for cached scale/bias");
        return fallback;
    }
    TORCH_CHECK(t->scalar_type() == at::kFloat, name, " must be fp32");
    TORCH_CHECK(t->is_contiguous(), name, " must be contiguous");
    return t->data_ptr<float>();
}

// ---- fp32 path ----

// A/B switch for the fp32 conv tile (mirrors DEFER_CONV_VARIANT): unset =
// the launcher's heuristic, "128x128" / "128x64" force one tile.
int conv_f32_tile() {
    static int tile = [] {
        const char* e = std::getenv("DEFER_CONV_F32_TILE");
        if (!e || !*e) return 0;
        std::string v(e);
        TORCH_CHECK(v == "128x128" || v == "128x64",
                    "DEFER_CONV_F32_TILE: expected unset, '128x128' or "
                    "'128x64'");
        return v == "128x128" ? 1 : 2;
    }();
    return tile;
}

// nullable fp32[n] scale/bias for the fp32 kernels (null = 1 / 0)
const float* f32_vec_opt(const c10::optional<Tensor>& t, const char* name,
                         int64_t n) {
    if (!t) return nullptr;
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat &&
                t->is_contiguous() && t->numel() == n &&
                (uintptr_t)t->data_ptr() % 16 == 0,
                name, " must be a contiguous GPU fp32[Cout]");
    return t->data_ptr<float>();
}

// shared tail of the fp32 conv / linear entry points; x is [.., Cin]
// with Cin % 4 == 0 here
void run_conv_f32(const Tensor& x, const Tensor& w, const float* scale,
                  const float* bias, const c10::optional<Tensor>& res,
                  Tensor& out, long M, int H, int W, int Cin, int OH, int OW,
                  int R, int S, int stride, int pad, int act) {
    int Cout = (int)out.size(-1);
    TORCH_CHECK(M < (1LL << 31), "M too large");
    TORCH_CHECK(x.numel() < (1LL << 31), "x has 2^31 or more elements");
    TORCH_CHECK(out.numel() < (1LL << 31), "out has 2^31 or more elements");
    if (res) {
        check_f32(*res, "res");
        TORCH_CHECK(res->numel() == out.numel(),
                    "res must match the output shape");
    }
    defer_hip::ConvF32Params p{};
    p.x = f32ptr(x);
    p.w = f32ptr(w);
    p.scale = scale;
    p.bias = bias;
    p.res = res ? f32ptr(*res) : nullptr;
    p.out = out.data_ptr<float>();
    p.M = (int)M; p.K = R * S * Cin; p.Cout = Cout;
    p.H = H; p.W = W; p.Cin = Cin;
    p.OH = OH; p.OW = OW; p.S = S; p.stride = stride; p.pad = pad;
    p.relu = act;
    bool gemm_mode = (R == 1 && S == 1 && stride == 1 && pad == 0);
    if (M > 0)
        defer_hip::launch_conv_f32(p, gemm_mode, conv_f32_tile(),
                                   cur_stream());
}

Tensor conv2d_bn_act_f32(const Tensor& x, const Tensor& w,
                         const c10::optional<Tensor>& scale,
                         const c10::optional<Tensor>& bias,
                         const c10::optional<Tensor>& res, int64_t stride,
                         int64_t pad, int act) {
    check_f32(x, "x");
    check_f32(w, "w");
    TORCH_CHECK(x.dim() == 4, "x must be NHWC");
    TORCH_CHECK(w.dim() == 4, "w must be OHWI");
    TORCH_CHECK(stride >= 1 && pad >= 0, "bad stride/pad");
    int NB = x.size(0), H = x.size(1), W = x.size(2), Cin = x.size(3);
    int Cout = w.size(0), R = w.size(1), S = w.size(2);
    TORCH_CHECK(w.size(3) == Cin, "w Cin mismatch");
    TORCH_CHECK(Cout % 4 == 0,
                "fp32 conv needs Cout % 4 == 0 (16-byte stores), got ",
                Cout);
    TORCH_CHECK(H + 2 * pad >= R && W + 2 * pad >= S,
                "kernel larger than the padded input");
    int OH = (int)((H + 2 * pad - R) / stride + 1);
    int OW = (int)((W + 2 * pad - S) / stride + 1);
    long M = (long)NB * OH * OW;
    const float* sc = f32_vec_opt(scale, "scale", Cout);
    const float* bi = f32_vec_opt(bias, "bias", Cout);
    auto out = at::empty({NB, OH, OW, Cout}, x.options());
    if (Cin % 4 != 0) {
        // odd-Cin stems: zero-pad channels to a multiple of 4 (weights
        // once, cached) so every K chunk is one aligned float4
        int C4 = (Cin + 3) / 4 * 4;
        hipStream_t s = cur_stream();
        auto xp = at::empty({NB, H, W, C4}, x.options());
        defer_hip::launch_pad_channels_f32(f32ptr(x), xp.data_ptr<float>(),
                                           (long)NB * H * W, Cin, C4, s);
        auto wp = cached_weight_prep(w, -4000 - C4, [&] {
            auto t = at::empty({Cout, R, S, C4}, w.options());
            defer_hip::launch_pad_channels_f32(
                f32ptr(w), t.data_ptr<float>(), (long)Cout * R * S, Cin, C4,
                s);
            return t;
        });
        run_conv_f32(xp, wp, sc, bi, res, out, M, H, W, C4, OH, OW, R, S,
                     (int)stride, (int)pad, act);
        return out;
    }
    run_conv_f32(x, w, sc, bi, res, out, M, H, W, Cin, OH, OW, R, S,
                 (int)stride, (int)pad, act);
    return out;
}

Tensor linear_f32(const Tensor& x, const Tensor& w,
                  const c10::optional<Tensor>& bias) {
    check_f32(x, "x");
    check_f32(w, "w");
    TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "linear wants 2-D");
    int M = x.size(0), K = x.size(1), N = w.size(0);
    TORCH_CHECK(w.size(1) == K, "K mismatch");
    TORCH_CHECK(K % 4 == 0, "fp32 linear needs K % 4 == 0, got ", K);
    TORCH_CHECK(N % 4 == 0, "fp32 linear needs N % 4 == 0, got ", N);
    auto out = at::empty({M, N}, x.options());
    run_conv_f32(x, w, nullptr, f32_vec_opt(bias, "bias", N), c10::nullopt,
                 out, M, 1, 1, K, 1, 1, 1, 1, 1, 0, kActNone);
    return out;
}

// What the weight-stationary 3x3 path did, for tests: how many times the
// kernel was launched in this process and the grid of the last launch.
struct ConvWsStats {
    std::mutex mu;
    int64_t launches = 0;
    int64_t blocks = 0, tiles_per_block = 0;
};
ConvWsStats& conv_ws_stats_ref() {
    static ConvWsStats st;
    return st;
}

py::dict conv_ws_stats() {
    auto& st = conv_ws_stats_ref();
    std::lock_guard<std::mutex> g(st.mu);
    py::dict d;
    d["launches"] = st.launches;
    d["blocks"] = st.blocks;
    d["tiles_per_block"] = st.tiles_per_block;
    return d;
}

// The one place that fills the ConvParams geometry (pointers stay null).
// gemm_mode collapses a 1x1/s1/p0 conv or a linear layer to
// out[M,N] = x[M,K] @ w[N,K]^T.
ConvParams conv_geom(long M, int K, int Cout, int NB, int H, int W, int Cin,
                     int OH, int OW, int R, int S, int stride, int pad,
                     bool gemm_mode) {
    ConvParams p{};
    p.M = (int)M; p.K = K; p.Cout = Cout;
    p.NB = NB; p.H = H; p.W = W; p.Cin = Cin;
    p.OH = OH; p.OW = OW; p.R = R; p.S = S;
    p.stride = stride; p.pad = pad;
    p.act_hi = INFINITY;            // plain ReLU; conv2d_bn_act sets ReLU6's
    if (gemm_mode) {
        p.NB = (int)M; p.H = 1; p.W = 1; p.Cin = K;
        p.OH = 1; p.OW = 1;
    }
    return p;
}

// Which way a bf16 conv goes and the geometry its kernel sees. Decided
// from the shapes alone: no allocation, no launch.
struct ConvPrep {
    enum Path { SWIN, STEM, PAD8, GENERAL } path = GENERAL;
    ConvParams p{};                 // geometry of the launch
    bool gemm_mode = false, stem_mode = false;
    int OH = 0, OW = 0;
    int C8 = 0;                     // SWIN, PAD8: padded channel count
    int Kpad = 0;                   // SWIN: padded K of the repacked weights
    int TR = 0, PH = 0, PW = 0;     // STEM (Keff is p.K)
};

ConvPrep prepare_conv(int NB, int H, int W, int Cin, int Cout, int R, int S,
                      int stride, int pad, bool has_res, char variant) {
    ConvPrep g;
    int OH = g.OH = (H + 2 * pad - R) / stride + 1;
    int OW = g.OW = (W + 2 * pad - S) / stride + 1;
    long M = (long)NB * OH * OW;
    TORCH_CHECK(M < (1LL << 31), "M too large");
    if (Cin % 8 == 0) {
        g.gemm_mode = (R == 1 && S == 1 && stride == 1 && pad == 0);
        g.p = conv_geom(M, R * S * Cin, Cout, NB, H, W, Cin, OH, OW, R, S,
                        stride, pad, g.gemm_mode);
        return g;
    }
    // small-Cin window path (VGG-style 3x3 stems): channel-pad to
    // 8, repack weights j-major (cached), stage each 8x16 output
    // tile's input window to LDS once — kills the ~9x input
    // re-reads of the channel-pad gather path (b1.c1 143 -> 91 us).
    // The 7x7/s2 ResNet stem stays on the spatial-prepad run-packed
    // path: its K is 168 vs the window kernel's zero-padded 448
    // (Cin 3 -> 8), and the 2.7x extra MFMA work measured slower.
    if (!has_res && R == S && R == 3 && (stride == 1 || stride == 2) &&
        Cout == 64) {
        ConvParams q = conv_geom(M, R * S * 8, Cout, NB, H, W, 8, OH, OW,
                                 R, S, stride, pad, false);
        if (defer_hip::plan_swin(q, variant).grid_x) {
            g.path = ConvPrep::SWIN;
            g.p = q;
            g.C8 = 8;
            g.Kpad = (R * R * 8 + 63) / 64 * 64;
            return g;
        }
    }
    if ((stride * Cin) % 2 == 0) {
        // STEM path (ResNet 7x7/s2, Cin=3): spatially pre-pad the
        // raw input and gather K as (r, run)-major where a run is
        // TR = ceil(S*Cin/8)*8 CONTIGUOUS bf16 of one padded input
        // row (S*Cin real + a few next-pixel values that multiply
        // zero weights). K drops from R*S*pad8(Cin) (392) to R*TR
        // (168) and the gather needs no validity math at all.
        int TR = (S * Cin + 7) / 8 * 8;
        int Keff = R * TR;
        int nk = (Keff + 63) / 64;
        int rmax = (nk * 64 - 1) / TR;          // last k row touched
        int PW = std::max(W + 2 * pad,
                          (OW - 1) * stride + (TR + Cin - 1) / Cin);
        int PH = std::max(H + 2 * pad, (OH - 1) * stride + rmax + 1);
        if (((long)PW * Cin) % 2) PW += 1;      // 4-B chunk alignment
        g.path = ConvPrep::STEM;
        g.stem_mode = true;
        g.TR = TR; g.PH = PH; g.PW = PW;
        // S carries the run length TR
        g.p = conv_geom(M, Keff, Cout, NB, PH, PW, Cin, OH, OW, R, TR,
                        stride, 0, false);
        return g;
    }
    // odd stride*Cin (e.g. 3x3/s1 VGG stem): zero-pad channels to 8
    // and take the regular implicit-GEMM path.
    g.path = ConvPrep::PAD8;
    g.C8 = (Cin + 7) / 8 * 8;
    g.p = conv_geom(M, R * S * g.C8, Cout, NB, H, W, g.C8, OH, OW, R, S,
                    stride, pad, false);
    return g;
}

// The kernel plan of a prepared conv. Only the general path may take the
// weight-stationary kernel.
defer_hip::ConvPlan plan_prepared(const ConvPrep& g, int64_t mode,
                                  int64_t max_blocks, char variant) {
    if (g.path == ConvPrep::SWIN) return defer_hip::plan_swin(g.p, variant);
    return defer_hip::plan_conv(
        g.p, g.gemm_mode, g.stem_mode,
        g.path == ConvPrep::GENERAL ? (int)mode : 2, (int)max_blocks,
        variant);
}

// What conv2d_bn_act (4-D shapes) or linear (2-D shapes) would launch for
// these shapes: the path, the prepared geometry, the plan and the kernel's
// template arguments. Runs prepare_conv and the plan and nothing else, so
// it needs no GPU. variant: a DEFER_CONV_VARIANT value, None = the latched
// environment value.
py::dict conv_plan(std::vector<int64_t> xs, std::vector<int64_t> ws,
                   int64_t stride, int64_t pad, bool has_res, int64_t mode,
                   int64_t max_blocks, c10::optional<std::string> variant) {
    using namespace pybind11::literals;
    TORCH_CHECK(mode >= 0 && mode <= 2, "mode must be 0, 1 or 2");
    TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0");
    const char v = variant ? (variant->empty() ? '\0' : (*variant)[0])
                           : defer_hip::conv_variant();
    ConvPrep g;
    const bool is_linear = xs.size() == 2 && ws.size() == 2;
    if (is_linear) {
        TORCH_CHECK(ws[1] == xs[1], "K mismatch");
        g.gemm_mode = true;
        g.p = conv_geom(xs[0], (int)xs[1], (int)ws[0], 0, 0, 0, 0, 0, 0, 1,
                        1, 1, 0, true);
        mode = 2;
    } else {
        TORCH_CHECK(xs.size() == 4, "x must be NHWC");
        TORCH_CHECK(ws.size() == 4, "w must be OHWI");
        TORCH_CHECK(ws[3] == xs[3], "w Cin mismatch");
        g = prepare_conv((int)xs[0], (int)xs[1], (int)xs[2], (int)xs[3],
                         (int)ws[0], (int)ws[1], (int)ws[2], (int)stride,
                         (int)pad, has_res, v);
    }
    static const char* paths[] = {"swin", "stem", "pad8", "general"};
    static const char* families[] = {"igemm", "win", "ws", "swin"};
    const auto pl = plan_prepared(g, mode, max_blocks, v);
    return py::dict(
        "path"_a = is_linear ? "linear" : paths[g.path], "M"_a = g.p.M,
        "K"_a = g.p.K, "Cin"_a = g.p.Cin, "C8"_a = g.C8, "Kpad"_a = g.Kpad,
        "TR"_a = g.TR, "PH"_a = g.PH, "PW"_a = g.PW,
        "family"_a = families[pl.family], "amode"_a = pl.amode,
        "bp"_a = (bool)pl.bp, "BM"_a = pl.BM, "BN"_a = pl.BN,
        "DA"_a = pl.DA, "DB"_a = pl.DB, "WPS"_a = pl.WPS, "TH"_a = pl.TH,
        "full_sync"_a = pl.full_sync, "grid_x"_a = pl.grid_x,
        "grid_y"_a = pl.grid_y, "blocks"_a = pl.blocks,
        "tiles_per_block"_a = pl.tiles_per_block,
        "template_args"_a = defer_hip::conv_kernel_args(pl, has_res));
}

// mode selects between the weight-stationary kernel (conv_ws.hip) and the
// launch_conv_igemm paths for the 3x3/s1/p1 64->64 bf16 class: 0 = the
// measured policy, 1 = the new kernel wherever it covers the shape, 2 =
// never. Shapes it does not cover run launch_conv_igemm under every mode.
// max_blocks caps that kernel's grid (0 = policy). act: kActNone, kActRelu,
// kActRelu6 or kActHardswish. ReLU6 runs the ReLU instantiation of whichever
// kernel the plan names, with the upper bound 6 in ConvParams::act_hi;
// hardswish has instantiations of its own (the third row of the launchers'
// kernel tables). Every dtype applies the activation in fp32 before the one
// rounding.
Tensor conv2d_bn_act(Tensor x, Tensor w, c10::optional<Tensor> scale,
                     c10::optional<Tensor> bias, c10::optional<Tensor> res,
                     int64_t stride, int64_t pad, int64_t act,
                     int64_t mode = 0, int64_t max_blocks = 0) {
    TORCH_CHECK(mode >= 0 && mode <= 2, "mode must be 0, 1 or 2");
    TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0");
    check_act(act);
    if (is_f32(x, "x"))
        return conv2d_bn_act_f32(x, w, scale, bias, res, stride, pad,
                                 (int)act);
    // the launchers' instantiation: 0 none, 1 relu (and relu6), 2 hardswish
    const int kact = act == kActNone ? 0 : act == kActHardswish ? 2 : 1;
    check_bf16(x, "x");
    check_bf16(w, "w");
    TORCH_CHECK(x.dim() == 4, "x must be NHWC");
    TORCH_CHECK(w.dim() == 4, "w must be OHWI");
    int NB = x.size(0), H = x.size(1), W = x.size(2), Cin = x.size(3);
    int Cout = w.size(0), R = w.size(1), S = w.size(2);
    TORCH_CHECK(w.size(3) == Cin, "w Cin mismatch");
    const char variant = defer_hip::conv_variant();
    const ConvPrep g = prepare_conv(NB, H, W, Cin, Cout, R, S, (int)stride,
                                    (int)pad, (bool)res, variant);
    auto out = at::empty({NB, g.OH, g.OW, Cout}, x.options());
    if (res) check_bf16(*res, "res");
    hipStream_t s = cur_stream();

    ConvParams p = g.p;
    p.scale = fptr_opt(scale, "scale", ones_buf(), Cout);
    p.bias = fptr_opt(bias, "bias", zeros_buf(), Cout);
    p.res = res ? bptr(*res) : nullptr;
    p.out = bptr_mut(out);
    p.zbuf = zero_buf();
    if (act == kActRelu6) p.act_hi = 6.0f;

    Tensor xp = x, wp = w;
    if (g.path == ConvPrep::SWIN) {
        xp = at::empty({NB, H, W, 8}, x.options());
        defer_hip::launch_pad_channels(bptr(x), bptr_mut(xp),
                                       (long)NB * H * W, Cin, 8, s);
        wp = cached_weight_prep(w, 1000 + g.Kpad, [&] {
            auto t = at::empty({Cout, g.Kpad}, w.options());
            defer_hip::launch_swin_repack_w(bptr(w), bptr_mut(t), Cout, R,
                                            Cin, g.Kpad, s);
            return t;
        });
    } else if (g.path == ConvPrep::STEM) {
        xp = at::empty({NB, g.PH, g.PW, Cin}, x.options());
        defer_hip::launch_pad2d(bptr(x), bptr_mut(xp), NB, H, W, Cin, g.PH,
                                g.PW, (int)pad, (int)pad, s);
        wp = cached_weight_prep(w, g.TR, [&] {
            auto t = at::empty({Cout, p.K}, w.options());
            defer_hip::launch_stem_repack_w(bptr(w), bptr_mut(t), Cout, R,
                                            S, Cin, g.TR, s);
            return t;
        });
    } else if (g.path == ConvPrep::PAD8) {
        xp = at::empty({NB, H, W, g.C8}, x.options());
        defer_hip::launch_pad_channels(bptr(x), bptr_mut(xp),
                                       (long)NB * H * W, Cin, g.C8, s);
        wp = cached_weight_prep(w, -g.C8, [&] {
            auto t = at::empty({Cout, R, S, g.C8}, w.options());
            defer_hip::launch_pad_channels(bptr(w), bptr_mut(t),
                                           (long)Cout * R * S, Cin, g.C8,
                                           s);
            return t;
        });
    }
    p.x = bptr(xp);
    p.w = bptr(wp);
    const auto plan = plan_prepared(g, mode, max_blocks, variant);
    if (plan.family == defer_hip::ConvPlan::WS) {
        auto used = defer_hip::launch_conv_ws(p, kact, (bool)res,
                                              (int)max_blocks, s);
        auto& st = conv_ws_stats_ref();
        std::lock_guard<std::mutex> g2(st.mu);
        ++st.launches;
        st.blocks = used.blocks;
        st.tiles_per_block = used.tiles_per_block;
        return out;
    }
    defer_hip::launch_conv_igemm(p, plan, kact, (bool)res, s);
    return out;
}

Tensor linear(Tensor x, Tensor w, c10::optional<Tensor> bias) {
    if (is_f32(x, "x")) return linear_f32(x, w, bias);
    check_bf16(x, "x");
    check_bf16(w, "w");
    TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "linear wants 2-D");
    int M = x.size(0), K = x.size(1), N = w.size(0);
    TORCH_CHECK(w.size(1) == K, "K mismatch");
    TORCH_CHECK(K % 8 == 0, "K must be a multiple of 8");
    auto out = at::empty({M, N}, x.options());
    c10::optional<Tensor> bias_f;
    if (bias)
        bias_f = cached_weight_prep(*bias, -1, [&] {
            return bias->to(at::kFloat).contiguous();
        });
    ConvParams p = conv_geom(M, K, N, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, true);
    p.x = bptr(x); p.w = bptr(w);
    p.scale = fptr_opt(c10::nullopt, "scale", ones_buf(), N);
    p.bias = fptr_opt(bias_f, "bias", zeros_buf(), N);
    p.res = nullptr; p.out = bptr_mut(out); p.zbuf = zero_buf();
    const auto plan = defer_hip::plan_conv(p, true, false, 2, 0,
                                           defer_hip::conv_variant());
    defer_hip::launch_conv_igemm(p, plan, false, false, cur_stream());
    return out;
}

Tensor conv1x1_prebn(Tensor x, Tensor w, Tensor scale, Tensor bias,
                     c10::optional<Tensor> out_scale,
                     c10::optional<Tensor> out_bias) {
    // x [N,H,W,Cin] bf16, w [Cout,1,1,Cin] bf16, scale/bias fp32[Cin]:
    // out = relu(x*scale+bias) @ w — one pass over x instead of the
    // bn_act tensor round-trip (DenseNet's dominant cost)
    check_bf16(x, "x");
    check_bf16(w, "w");
    TORCH_CHECK(x.dim() == 4 && w.dim() == 4 && w.size(1) == 1
                && w.size(2) == 1, "conv1x1_prebn wants NHWC x, 1x1 w");
    int NB = x.size(0), H = x.size(1), W = x.size(2), Cin = x.size(3);
    int Cout = w.size(0);
    TORCH_CHECK(w.size(3) == Cin && Cin % 8 == 0, "Cin mismatch");
    TORCH_CHECK(scale.scalar_type() == at::kFloat && scale.is_contiguous()
                && scale.numel() == Cin, "scale must be fp32[Cin]");
    TORCH_CHECK(bias.scalar_type() == at::kFloat && bias.is_contiguous()
                && bias.numel() == Cin, "bias must be fp32[Cin]");
    long M = (long)NB * H * W;
    TORCH_CHECK(M < (1LL << 31), "M too large");
    auto out = at::empty({NB, H, W, Cout}, x.options());
    const float* os = nullptr;
    const float* ob = nullptr;
    if (out_scale) {
        TORCH_CHECK(out_bias, "out_scale needs out_bias");
        TORCH_CHECK(out_scale->scalar_type() == at::kFloat
                    && out_scale->is_contiguous()
                    && out_scale->numel() == Cout
                    && out_bias->scalar_type() == at::kFloat
                    && out_bias->is_contiguous()
                    && out_bias->numel() == Cout,
                    "out affine must be fp32[Cout]");
        os = out_scale->data_ptr<float>();
        ob = out_bias->data_ptr<float>();
    }
    defer_hip::launch_gemm_prebn(bptr(x), bptr(w),
                                 scale.data_ptr<float>(),
                                 bias.data_ptr<float>(), os, ob,
                                 zero_buf(), bptr_mut(out), (int)M, Cin,
                                 Cout, cur_stream());
    return out;
}

// What the chain kernel did, for tests: launches in this process, and the
// grid and the tile height of the last one.
struct ChainStats {
    std::mutex mu;
    int64_t launches = 0;
    int64_t blocks = 0;
    int64_t bm = 0;
};
ChainStats& chain_stats_ref() {
    static ChainStats st;
    return st;
}

py::dict conv1x1_chain_stats() {
    auto& st = chain_stats_ref();
    std::lock_guard<std::mutex> g(st.mu);
    py::dict d;
    d["launches"] = st.launches;
    d["blocks"] = st.blocks;
    d["bm"] = st.bm;
    return d;
}

std::tuple<Tensor, Tensor> conv1x1_chain(
    Tensor x, Tensor w3, c10::optional<Tensor> s3, c10::optional<Tensor> b3,
    Tensor res, bool relu3, Tensor w1, c10::optional<Tensor> s1,
    c10::optional<Tensor> b1, bool relu1, int64_t mode,
    int64_t max_blocks, int64_t bm) {
    // y = act3(conv1x1(x, w3)*s3+b3 + res); a2 = act1(conv1x1(y, w1)*s1+b1)
    // mode 0: fused kernel where the launcher's measured policy says so;
    // 1: fused wherever an instantiation exists; 2: always two launches.
    // bm: rows of a fused tile, 0 = the launcher's measured policy, 64, or
    // 128 where the class has that form (else 64).
    check_bf16(x, "x");
    check_bf16(w3, "w3");
    check_bf16(w1, "w1");
    check_bf16(res, "res");
    TORCH_CHECK(x.dim() == 4 && w3.dim() == 4 && w1.dim() == 4 &&
                w3.size(1) == 1 && w3.size(2) == 1 && w1.size(1) == 1 &&
                w1.size(2) == 1, "conv1x1_chain wants NHWC x, 1x1 weights");
    TORCH_CHECK(mode >= 0 && mode <= 2, "mode must be 0, 1 or 2");
    TORCH_CHECK(bm == 0 || bm == 64 || bm == 128, "bm must be 0, 64 or 128");
    int NB = x.size(0), H = x.size(1), W = x.size(2), K1 = x.size(3);
    int N1 = w3.size(0), N2 = w1.size(0);
    TORCH_CHECK(w3.size(3) == K1 && w1.size(3) == N1, "channel mismatch");
    TORCH_CHECK(res.dim() == 4 && res.size(0) == NB && res.size(1) == H &&
                res.size(2) == W && res.size(3) == N1,
                "res must match the expand output");
    TORCH_CHECK((!s3 || s3->numel() == N1) && (!b3 || b3->numel() == N1) &&
                (!s1 || s1->numel() == N2) && (!b1 || b1->numel() == N2),
                "scale/bias length must equal the conv's Cout");
    long M = (long)NB * H * W;
    TORCH_CHECK(M < (1LL << 31), "M too large");
    if (mode != 2 && K1 % 64 == 0 && N1 % 64 == 0 && N2 % 64 == 0) {
        auto y = at::empty({NB, H, W, N1}, x.options());
        auto a2 = at::empty({NB, H, W, N2}, x.options());
        defer_hip::ChainLaunch l = defer_hip::launch_conv1x1_chain(
            bptr(x), bptr(w3), fptr_opt(s3, "s3", ones_buf(), N1),
            fptr_opt(b3, "b3", zeros_buf(), N1), bptr(res), bptr_mut(y),
            relu3, bptr(w1), fptr_opt(s1, "s1", ones_buf(), N2),
            fptr_opt(b1, "b1", zeros_buf(), N2), bptr_mut(a2), relu1, (int)M,
            K1, N1, N2, mode == 1, (int)max_blocks, (int)bm, cur_stream());
        if (l.blocks > 0) {
            auto& st = chain_stats_ref();
            std::lock_guard<std::mutex> g(st.mu);
            ++st.launches;
            st.blocks = l.blocks;
            st.bm = l.bm;
            return {y, a2};
        }
    }
    auto y = conv2d_bn_act(x, w3, s3, b3, res, 1, 0, relu3);
    auto a2 = conv2d_bn_act(y, w1, s1, b1, c10::nullopt, 1, 0, relu1);
    return {y, a2};
}

// What the projected-residual chain kernel did, for tests: launches in
// this process and the grid of the last one.
struct ChainProjStats {
    std::mutex mu;
    int64_t launches = 0;
    int64_t blocks = 0;
};
ChainProjStats& chain_proj_stats_ref() {
    static ChainProjStats st;
    return st;
}

py::dict chain_proj_stats() {
    auto& st = chain_proj_stats_ref();
    std::lock_guard<std::mutex> g(st.mu);
    py::dict d;
    d["launches"] = st.launches;
    d["blocks"] = st.blocks;
    return d;
}

// conv1x1_chain whose residual is bf16(conv1x1(xp, wp)*sp+bp), made inside
// the kernel. mode 0: where the launcher's measured policy says so; 1:
// wherever the kernel serves the shape. Returns nothing when no kernel was
// launched: the caller then composes the projection conv and conv1x1_chain.
c10::optional<std::tuple<Tensor, Tensor>> conv1x1_chain_proj(
    Tensor x, Tensor w3, c10::optional<Tensor> s3, c10::optional<Tensor> b3,
    Tensor xp, Tensor wp, c10::optional<Tensor> sp, c10::optional<Tensor> bp,
    bool relu3, Tensor w1, c10::optional<Tensor> s1,
    c10::optional<Tensor> b1, bool relu1, int64_t mode,
    int64_t max_blocks) {
    check_bf16(x, "x");
    check_bf16(w3, "w3");
    check_bf16(xp, "xp");
    check_bf16(wp, "wp");
    check_bf16(w1, "w1");
    TORCH_CHECK(x.dim() == 4 && xp.dim() == 4 && w3.dim() == 4 &&
                wp.dim() == 4 && w1.dim() == 4 && w3.size(1) == 1 &&
                w3.size(2) == 1 && wp.size(1) == 1 && wp.size(2) == 1 &&
                w1.size(1) == 1 && w1.size(2) == 1,
                "conv1x1_chain_proj wants NHWC x and xp, 1x1 weights");
    TORCH_CHECK(mode >= 0 && mode <= 1, "mode must be 0 or 1");
    TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0");
    int NB = x.size(0), H = x.size(1), W = x.size(2), K1 = x.size(3);
    int KP = xp.size(3);
    int N1 = w3.size(0), N2 = w1.size(0);
    TORCH_CHECK(w3.size(3) == K1 && w1.size(3) == N1 && wp.size(0) == N1 &&
                wp.size(3) == KP, "channel mismatch");
    TORCH_CHECK(xp.size(0) == NB && xp.size(1) == H && xp.size(2) == W,
                "xp must cover the pixels of x");
    TORCH_CHECK((!s3 || s3->numel() == N1) && (!b3 || b3->numel() == N1) &&
                (!sp || sp->numel() == N1) && (!bp || bp->numel() == N1) &&
                (!s1 || s1->numel() == N2) && (!b1 || b1->numel() == N2),
                "scale/bias length must equal the conv's Cout");
    long M = (long)NB * H * W;
    TORCH_CHECK(M < (1LL << 31), "M too large");
    if (K1 != 64 || KP != 64 || N2 != 64 || N1 % 64 != 0 || M == 0)
        return c10::nullopt;
    auto y = at::empty({NB, H, W, N1}, x.options());
    auto a2 = at::empty({NB, H, W, N2}, x.options());
    int blocks = defer_hip::launch_conv1x1_chain_proj(
        bptr(x), bptr(w3), fptr_opt(s3, "s3", ones_buf(), N1),
        fptr_opt(b3, "b3", zeros_buf(), N1), bptr(xp), bptr(wp),
        fptr_opt(sp, "sp", ones_buf(), N1),
        fptr_opt(bp, "bp", zeros_buf(), N1), bptr_mut(y), relu3, bptr(w1),
        fptr_opt(s1, "s1", ones_buf(), N2),
        fptr_opt(b1, "b1", zeros_buf(), N2), bptr_mut(a2), relu1, (int)M,
        K1, KP, N1, N2, mode == 1, (int)max_blocks, cur_stream());
    if (blocks == 0) return c10::nullopt;
    auto& st = chain_proj_stats_ref();
    std::lock_guard<std::mutex> g(st.mu);
    ++st.launches;
    st.blocks = blocks;
    return std::make_tuple(y, a2);
}

Tensor bn_act(Tensor x, Tensor scale, Tensor bias, bool relu) {
    if (is_f32(x, "x")) {
        check_f32(x, "x");
        int C = x.size(-1);
        TORCH_CHECK(C % 4 == 0, "fp32 bn_act needs C % 4 == 0, got ", C);
        TORCH_CHECK(scale.is_cuda() && bias.is_cuda() &&
                    scale.numel() == C && bias.numel() == C,
                    "scale/bias must be GPU tensors of length C");
        auto out = at::empty_like(x);
        auto sf = scale.to(at::kFloat).contiguous();
        auto bf = bias.to(at::kFloat).contiguous();
        defer_hip::launch_bn_act_f32(f32ptr(x), f32ptr(sf), f32ptr(bf),
                                     out.data_ptr<float>(), x.numel() / 4,
                                     C / 4, relu, cur_stream());
        return out;
    }
    check_bf16(x, "x");
    int C = x.size(-1);
    TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
    TORCH_CHECK(scale.is_cuda() && bias.is_cuda() &&
                scale.numel() == C && bias.numel() == C,
                "scale/bias must be GPU tensors of length C");
    auto out = at::empty_like(x);
    auto sf = scale.to(at::kFloat).contiguous();
    auto bf = bias.to(at::kFloat).contiguous();
    defer_hip::launch_bn_act(bptr(x), sf.data_ptr<float>(),
                             bf.data_ptr<float>(), bptr_mut(out),
                             x.numel() / 8, C / 8, relu, cur_stream());
    return out;
}

Tensor add_act(Tensor a, Tensor b, bool relu) {
    if (is_f32(a, "a")) {
        check_f32(a, "a");
        check_f32(b, "b");
        TORCH_CHECK(a.sizes() == b.sizes(), "shape mismatch");
        TORCH_CHECK(a.numel() % 4 == 0,
                    "fp32 add_act needs numel % 4 == 0");
        auto out = at::empty_like(a);
        defer_hip::launch_add_act_f32(f32ptr(a), f32ptr(b),
                                      out.data_ptr<float>(), a.numel() / 4,
                                      relu, cur_stream());
        return out;
    }
    check_bf16(a, "a");
    check_bf16(b, "b");
    TORCH_CHECK(a.sizes() == b.sizes(), "shape mismatch");
    TORCH_CHECK(a.numel() % 8 == 0, "numel must be a multiple of 8");
    auto out = at::empty_like(a);
    defer_hip::launch_add_act(bptr(a), bptr(b), bptr_mut(out),
                              a.numel() / 8, relu, cur_stream());
    return out;
}

Tensor relu(Tensor x) {
    if (is_f32(x, "x")) {
        check_f32(x, "x");
        TORCH_CHECK(x.numel() % 4 == 0, "fp32 relu needs numel % 4 == 0");
        auto out = at::empty_like(x);
        defer_hip::launch_relu_f32(f32ptr(x), out.data_ptr<float>(),
                                   x.numel() / 4, cur_stream());
        return out;
    }
    check_bf16(x, "x");
    TORCH_CHECK(x.numel() % 8 == 0, "numel must be a multiple of 8");
    auto out = at::empty_like(x);
    defer_hip::launch_relu(bptr(x), bptr_mut(out), x.numel() / 8,
                           cur_stream());
    return out;
}

Tensor relu6(Tensor x) {
    if (is_f32(x, "x")) {
        check_f32(x, "x");
        TORCH_CHECK(x.numel() % 4 == 0, "fp32 relu6 needs numel % 4 == 0");
        auto out = at::empty_like(x);
        defer_hip::launch_relu6_f32(f32ptr(x), out.data_ptr<float>(),
                                    x.numel() / 4, cur_stream());
        return out;
    }
    check_bf16(x, "x");
    TORCH_CHECK(x.numel() % 8 == 0, "numel must be a multiple of 8");
    auto out = at::empty_like(x);
    defer_hip::launch_relu6(bptr(x), bptr_mut(out), x.numel() / 8,
                            cur_stream());
    return out;
}

Tensor hardswish(Tensor x) {
    if (is_f32(x, "x")) {
        check_f32(x, "x");
        TORCH_CHECK(x.numel() % 4 == 0,
                    "fp32 hardswish needs numel % 4 == 0");
        auto out = at::empty_like(x);
        defer_hip::launch_hardswish_f32(f32ptr(x), out.data_ptr<float>(),
                                        x.numel() / 4, cur_stream());
        return out;
    }
    check_bf16(x, "x");
    TORCH_CHECK(x.numel() % 8 == 0, "numel must be a multiple of 8");
    auto out = at::empty_like(x);
    defer_hip::launch_hardswish(bptr(x), bptr_mut(out), x.numel() / 8,
                                cur_stream());
    return out;
}

// fp32 bias of one FC of squeeze_excite: absent = null (the kernel adds
// nothing); present = fp32[n] on x's device, whatever the compute dtype
const float* se_bias(const c10::optional<Tensor>& t, const char* name,
                     int64_t n, const Tensor& x) {
    if (!t) return nullptr;
    TORCH_CHECK(t->device() == x.device() &&
                t->scalar_type() == at::kFloat && t->is_contiguous() &&
                t->dim() == 1 && t->numel() == n,
                "squeeze_excite: ", name, " must be a contiguous fp32[", n,
                "] on x's device");
    return t->data_ptr<float>();
}

// The gate of squeeze-excite (csrc/se.hip), fp32 [N, C]:
// g = hardsigmoid(w2 @ act(w1 @ mean_hw(x) + b1) + b2), all in fp32. One
// launch on the current stream, no host sync. act: kActNone or kActRelu.
// The kernel's LDS holds the C means and the Cr hidden values in fp32.
Tensor se_gate(Tensor x, Tensor w1, c10::optional<Tensor> b1, Tensor w2,
               c10::optional<Tensor> b2, int64_t act) {
    TORCH_CHECK(act == kActNone || act == kActRelu,
                "squeeze_excite: act must be 0 (none) or 1 (relu), got ",
                act);
    const bool f32 = is_f32(x, "x");
    for (const Tensor* t : {&x, &w1, &w2}) {
        const char* name = t == &x ? "x" : t == &w1 ? "w1" : "w2";
        if (f32) check_f32(*t, name);
        else check_bf16(*t, name);
        TORCH_CHECK((uintptr_t)t->data_ptr() % 16 == 0, name,
                    " must be 16-byte aligned");
    }
    TORCH_CHECK(w1.device() == x.device() && w2.device() == x.device(),
                "squeeze_excite: w1 and w2 must be on x's device");
    TORCH_CHECK(x.dim() == 4, "squeeze_excite: x must be NHWC, got ",
                x.dim(), "-D");
    int64_t NB = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
    const int vec = f32 ? 4 : 8;
    TORCH_CHECK(C > 0 && C % vec == 0, "squeeze_excite: ",
                f32 ? "fp32" : "bf16", " needs C % ", vec, " == 0, got ", C);
    TORCH_CHECK(w1.dim() == 2 && w1.size(1) == C && w1.size(0) >= 1,
                "squeeze_excite: w1 must be [Cr, C] with C = ", C);
    const int64_t Cr = w1.size(0);
    TORCH_CHECK(w2.dim() == 2 && w2.size(0) == C && w2.size(1) == Cr,
                "squeeze_excite: w2 must be [C, Cr] = [", C, ", ", Cr, "]");
    const float* bp1 = se_bias(b1, "b1", Cr, x);
    const float* bp2 = se_bias(b2, "b2", C, x);
    TORCH_CHECK(H * W > 0, "squeeze_excite: empty spatial extent");
    TORCH_CHECK(H * W < (1LL << 30) && NB < (1LL << 31),
                "squeeze_excite: H * W of 2^30 or a batch of 2^31 or more");
    TORCH_CHECK(C + Cr <= defer_hip::SE_MAX_LDS_FLOATS,
                "squeeze_excite: C + Cr must be at most ",
                defer_hip::SE_MAX_LDS_FLOATS, ", got ", C + Cr);
    auto g = at::empty({NB, C}, x.options().dtype(at::kFloat));
    if (NB == 0) return g;
    defer_hip::launch_se_gate(x.data_ptr(), w1.data_ptr(), bp1,
                              w2.data_ptr(), bp2, g.data_ptr<float>(),
                              (int)NB, (int)(H * W), (int)C, (int)Cr,
                              (int)act, f32, cur_stream());
    return g;
}

// y[n, h, w, c] = round(x[n, h, w, c] * g[n, c]): the scale pass of
// squeeze-excite. x NHWC bf16 or fp32, g fp32 [N, C].
Tensor channel_scale(Tensor x, Tensor g) {
    const bool f32 = is_f32(x, "x");
    if (f32) check_f32(x, "x");
    else check_bf16(x, "x");
    check_f32(g, "g");
    TORCH_CHECK(g.device() == x.device(),
                "channel_scale: g must be on x's device");
    TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0,
                "x must be 16-byte aligned");
    TORCH_CHECK(x.dim() == 4, "channel_scale: x must be NHWC");
    int64_t NB = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
    const int vec = f32 ? 4 : 8;
    TORCH_CHECK(C > 0 && C % vec == 0, "channel_scale: ",
                f32 ? "fp32" : "bf16", " needs C % ", vec, " == 0, got ", C);
    TORCH_CHECK(g.dim() == 2 && g.size(0) == NB && g.size(1) == C,
                "channel_scale: g must be [N, C] = [", NB, ", ", C, "]");
    auto y = at::empty_like(x);
    if (y.numel() == 0) return y;
    defer_hip::launch_channel_scale(x.data_ptr(), g.data_ptr<float>(),
                                    y.data_ptr(), NB, HW, (int)C, f32,
                                    cur_stream());
    return y;
}

// Squeeze-excite: y = x * se_gate(x, ...). Two launches, both
// deterministic; g comes from torch's allocator, so the pair can be
// captured into a hipGraph.
Tensor squeeze_excite(Tensor x, Tensor w1, c10::optional<Tensor> b1,
                      Tensor w2, c10::optional<Tensor> b2, int64_t act) {
    return channel_scale(x, se_gate(x, w1, b1, w2, b2, act));
}

// fp32[C] scale / bias of the depthwise conv; absent = the cached ones /
// zeros, which bound C
const float* dw_vec_opt(const c10::optional<Tensor>& t, const char* name,
                        const float* fallback, int64_t C) {
    if (!t) {
        TORCH_CHECK(C <= 8192, "dwconv2d_bn_act without ", name,
                    " takes at most C = 8192, got ", C);
        return fallback;
    }
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat &&
                t->is_contiguous() && t->numel() == C,
                name, " must be a contiguous GPU fp32[C]");
    return t->data_ptr<float>();
}

// Depthwise conv + folded BN + activation (csrc/dwconv.hip): x NHWC, w
// [R, S, C], both bf16 or both fp32. Everything the kernels do not serve
// is refused here; there is no other path.
Tensor dwconv2d_bn_act(Tensor x, Tensor w, c10::optional<Tensor> scale,
                       c10::optional<Tensor> bias, int64_t stride,
                       int64_t pad, int64_t act) {
    check_act(act);
    const bool f32 = is_f32(x, "x");
    if (f32) {
        check_f32(x, "x");
        check_f32(w, "w");
    } else {
        check_bf16(x, "x");
        check_bf16(w, "w");
        TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 &&
                    (uintptr_t)w.data_ptr() % 16 == 0,
                    "x and w must be 16-byte aligned");
    }
    TORCH_CHECK(x.dim() == 4, "x must be NHWC");
    TORCH_CHECK(w.dim() == 3, "w must be [R, S, C]");
    int64_t NB = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
    int64_t R = w.size(0), S = w.size(1);
    TORCH_CHECK(w.size(2) == C, "w has ", w.size(2), " channels, x has ", C);
    TORCH_CHECK(R == S && (R == 3 || R == 5),
                "depthwise conv needs a 3x3 or 5x5 kernel, got ", R, "x", S);
    TORCH_CHECK(stride == 1 || stride == 2,
                "depthwise conv needs stride 1 or 2, got ", stride);
    TORCH_CHECK(pad >= 0 && pad <= R / 2,
                "depthwise conv needs 0 <= padding <= R / 2, got ", pad);
    const int vec = f32 ? 4 : 8;
    TORCH_CHECK(C > 0 && C % vec == 0, f32 ? "fp32" : "bf16",
                " depthwise conv needs C % ", vec, " == 0, got ", C);
    TORCH_CHECK(H + 2 * pad >= R && W + 2 * pad >= S,
                "kernel larger than the padded input");
    TORCH_CHECK(x.numel() < (1LL << 31), "x has 2^31 or more elements");
    int64_t OH = (H + 2 * pad - R) / stride + 1;
    int64_t OW = (W + 2 * pad - S) / stride + 1;
    TORCH_CHECK(NB * OH * OW * C < (1LL << 31),
                "out has 2^31 or more elements");
    const float* sc = dw_vec_opt(scale, "scale", ones_buf(), C);
    const float* bi = dw_vec_opt(bias, "bias", zeros_buf(), C);
    auto out = at::empty({NB, OH, OW, C}, x.options());
    if (out.numel() == 0) return out;
    if (f32)
        defer_hip::launch_dwconv_f32(f32ptr(x), f32ptr(w), sc, bi,
                                     out.data_ptr<float>(), (int)NB, (int)H,
                                     (int)W, (int)C, (int)OH, (int)OW,
                                     (int)R, (int)stride, (int)pad,
                                     (int)act, cur_stream());
    else
        defer_hip::launch_dwconv(bptr(x), bptr(w), sc, bi, bptr_mut(out),
                                 (int)NB, (int)H, (int)W, (int)C, (int)OH,
                                 (int)OW, (int)R, (int)stride, (int)pad,
                                 (int)act, cur_stream());
    return out;
}

Tensor softmax(Tensor x) {
    if (is_f32(x, "x")) {
        check_f32(x, "x");
        TORCH_CHECK(x.dim() >= 1 && x.numel() > 0, "softmax of nothing");
        int cols = x.size(-1);
        long rows = x.numel() / cols;
        auto out = at::empty_like(x);
        defer_hip::launch_softmax_f32(f32ptr(x), out.data_ptr<float>(),
                                      (int)rows, cols, cur_stream());
        return out;
    }
    check_bf16(x, "x");
    TORCH_CHECK(x.dim() >= 1 && x.numel() > 0, "softmax of nothing");
    int cols = x.size(-1);
    long rows = x.numel() / cols;
    auto out = at::empty_like(x);
    defer_hip::launch_softmax(bptr(x), bptr_mut(out), (int)rows, cols,
                              cur_stream());
    return out;
}

Tensor maxpool2d(Tensor x, int64_t kernel, int64_t stride, int64_t pad) {
    if (is_f32(x, "x")) {
        check_f32(x, "x");
        check_pool(x, kernel, stride, pad, "maxpool2d");
        int NB = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
        TORCH_CHECK(C % 4 == 0, "fp32 maxpool2d needs C % 4 == 0, got ", C);
        int OH = (int)((H + 2 * pad - kernel) / stride + 1);
        int OW = (int)((W + 2 * pad - kernel) / stride + 1);
        auto out = at::empty({NB, OH, OW, C}, x.options());
        defer_hip::launch_maxpool_f32(f32ptr(x), out.data_ptr<float>(), NB, H,
                                 W, C, OH, OW, (int)kernel, (int)stride,
                                 (int)pad, cur_stream());
        return out;
    }
    check_bf16(x, "x");
    check_pool(x, kernel, stride, pad, "maxpool2d");
    int NB = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
    TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
    int OH = (int)((H + 2 * pad - kernel) / stride + 1);
    int OW = (int)((W + 2 * pad - kernel) / stride + 1);
    auto out = at::empty({NB, OH, OW, C}, x.options());
    defer_hip::launch_maxpool(bptr(x), bptr_mut(out), NB, H, W, C, OH, OW,
                              (int)kernel, (int)stride, (int)pad,
                              cur_stream());
    return out;
}

// What the fused stem path did, for tests: how many times the kernel was
// launched in this process and the band split of the last launch.
struct StemPoolStats {
    std::mutex mu;
    int64_t launches = 0;
    int64_t bands = 0, rows_per_band = 0;
};
StemPoolStats& stem_pool_stats_ref() {
    static StemPoolStats st;
    return st;
}

py::dict stem_pool_stats() {
    auto& st = stem_pool_stats_ref();
    std::lock_guard<std::mutex> g(st.mu);
    py::dict d;
    d["launches"] = st.launches;
    d["bands"] = st.bands;
    d["rows_per_band"] = st.rows_per_band;
    return d;
}

Tensor conv_bn_act_maxpool(Tensor x, Tensor w, c10::optional<Tensor> scale,
                           c10::optional<Tensor> bias, int64_t stride,
                           int64_t pad, bool relu, int64_t pool_kernel,
                           int64_t pool_stride, int64_t pool_pad,
                           int64_t mode, int64_t max_blocks) {
    // maxpool(act(conv(x, w)*scale + bias)). mode 0: fused kernel where
    // the policy says so; 1: fused wherever the kernel covers the shape;
    // 2: always two launches. bf16 only (ops composes the fp32 path).
    check_bf16(x, "x");
    check_bf16(w, "w");
    TORCH_CHECK(x.dim() == 4, "x must be NHWC");
    TORCH_CHECK(w.dim() == 4, "w must be OHWI");
    TORCH_CHECK(mode >= 0 && mode <= 2, "mode must be 0, 1 or 2");
    TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0");
    int NB = x.size(0), H = x.size(1), W = x.size(2), Cin = x.size(3);
    int Cout = w.size(0), R = w.size(1), S = w.size(2);
    TORCH_CHECK(w.size(3) == Cin, "w Cin mismatch");
    TORCH_CHECK((!scale || scale->numel() == Cout) &&
                (!bias || bias->numel() == Cout),
                "scale/bias length must equal Cout");
    int OH = (int)((H + 2 * pad - R) / stride + 1);
    int OW = (int)((W + 2 * pad - S) / stride + 1);
    // policy: the fused kernel won the A/B at batch 256, 64, 8 and 1
    // (docs/OPTIMIZATION_LOG.md), so mode 0 takes it wherever it is legal
    // and is the same as mode 1 today
    if (mode != 2 && NB > 0 && OH > 0 && OW > 0 &&
        (long)NB * OH * OW < (1LL << 31) &&
        defer_hip::stem_pool_supported(Cin, Cout, R, S, (int)stride,
                                       (int)pad, relu, (int)pool_kernel,
                                       (int)pool_stride, (int)pool_pad,
                                       OH, OW)) {
        hipStream_t s = cur_stream();
        // same repacked weights as the STEM path of conv2d_bn_act
        // (TR = 24, K = 168); the kernel pads the raw input itself
        const int TR = 24, Keff = R * TR;
        auto wp = cached_weight_prep(w, TR, [&] {
            auto t = at::empty({Cout, Keff}, w.options());
            defer_hip::launch_stem_repack_w(bptr(w), bptr_mut(t), Cout, R,
                                            S, Cin, TR, s);
            return t;
        });
        int POH = (OH + 2 - 3) / 2 + 1, POW = (OW + 2 - 3) / 2 + 1;
        auto out = at::empty({NB, POH, POW, Cout}, x.options());
        defer_hip::StemPoolParams q{};
        q.x = bptr(x);
        q.wp = bptr(wp);
        q.scale = fptr_opt(scale, "scale", ones_buf(), Cout);
        q.bias = fptr_opt(bias, "bias", zeros_buf(), Cout);
        q.out = bptr_mut(out);
        q.NB = NB; q.H = H; q.W = W;
        q.OH = OH; q.OW = OW; q.POH = POH; q.POW = POW;
        auto used = defer_hip::launch_stem_pool(q, (int)max_blocks, s);
        {
            auto& st = stem_pool_stats_ref();
            std::lock_guard<std::mutex> g(st.mu);
            ++st.launches;
            st.bands = used.bands;
            st.rows_per_band = used.rpb;
        }
        return out;
    }
    auto y = conv2d_bn_act(x, w, scale, bias, c10::nullopt, stride, pad,
                           relu);
    return maxpool2d(y, pool_kernel, pool_stride, pool_pad);
}

Tensor avgpool2d(Tensor x, int64_t kernel, int64_t stride, int64_t pad) {
    if (is_f32(x, "x")) {
        check_f32(x, "x");
        check_pool(x, kernel, stride, pad, "avgpool2d");
        int NB = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
        TORCH_CHECK(C % 4 == 0, "fp32 avgpool2d needs C % 4 == 0, got ", C);
        int OH = (int)((H + 2 * pad - kernel) / stride + 1);
        int OW = (int)((W + 2 * pad - kernel) / stride + 1);
        auto out = at::empty({NB, OH, OW, C}, x.options());
        defer_hip::launch_avgpool_f32(f32ptr(x), out.data_ptr<float>(), NB, H,
                                 W, C, OH, OW, (int)kernel, (int)stride,
                                 (int)pad, cur_stream());
        return out;
    }
    check_bf16(x, "x");
    check_pool(x, kernel, stride, pad, "avgpool2d");
    int NB = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
    TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
    int OH = (int)((H + 2 * pad - kernel) / stride + 1);
    int OW = (int)((W + 2 * pad - kernel) / stride + 1);
    auto out = at::empty({NB, OH, OW, C}, x.options());
    defer_hip::launch_avgpool(bptr(x), bptr_mut(out), NB, H, W, C, OH,
                              OW, (int)kernel, (int)stride, (int)pad,
                              cur_stream());
    return out;
}

// Concat along the LAST (channel) dim of NHWC tensors: pure data
// movement, one strided device-to-device hipMemcpy2DAsync per input
// (row = one pixel's channels) — no torch compute kernels in the path
// (DenseNet's dense blocks are concat-heavy).
Tensor concat_lastdim(std::vector<Tensor> xs) {
    TORCH_CHECK(!xs.empty(), "concat of nothing");
    auto base = xs[0].sizes().vec();
    int nd = (int)base.size();
    long rows = 1;
    for (int i = 0; i + 1 < nd; ++i) rows *= base[i];
    long ctot = 0;
    const bool f32 = is_f32(xs[0], "concat input");
    for (auto& t : xs) {
        if (f32) check_f32(t, "concat input");
        else check_bf16(t, "concat input");
        TORCH_CHECK((int)t.sizes().size() == nd, "rank mismatch");
        for (int i = 0; i + 1 < nd; ++i)
            TORCH_CHECK(t.size(i) == base[i], "leading-dim mismatch");
        ctot += t.size(nd - 1);
    }
    base[nd - 1] = ctot;
    auto out = at::empty(base, xs[0].options());
    hipStream_t s = cur_stream();
    if (f32) {
        if (xs.size() == 2 && xs[0].size(nd - 1) % 4 == 0 &&
            xs[1].size(nd - 1) % 4 == 0) {
            defer_hip::launch_cat2_f32(f32ptr(xs[0]), f32ptr(xs[1]),
                                       out.data_ptr<float>(), rows,
                                       (int)xs[0].size(nd - 1),
                                       (int)xs[1].size(nd - 1), s);
            return out;
        }
        long coff = 0;
        for (auto& t : xs) {
            long cj = t.size(nd - 1);
            hipMemcpy2DAsync((char*)bptr_mut(out) + coff * 4, ctot * 4,
                             bptr(t), cj * 4, cj * 4, rows,
                             hipMemcpyDeviceToDevice, s);
            coff += cj;
        }
        return out;
    }
    if (xs.size() == 2 && xs[0].size(nd - 1) % 8 == 0 &&
        xs[1].size(nd - 1) % 8 == 0) {
        // the DenseNet shape class: one vectorized kernel beats the
        // per-input small-pitch 2D copies (measured)
        defer_hip::launch_cat2(bptr(xs[0]), bptr(xs[1]), bptr_mut(out),
                               rows, (int)xs[0].size(nd - 1),
                               (int)xs[1].size(nd - 1), s);
        return out;
    }
    long coff = 0;
    for (auto& t : xs) {
        long cj = t.size(nd - 1);
        hipMemcpy2DAsync((char*)bptr_mut(out) + coff * 2, ctot * 2,
                         bptr(t), cj * 2, cj * 2, rows,
                         hipMemcpyDeviceToDevice, s);
        coff += cj;
    }
    return out;
}

Tensor global_avg_pool(Tensor x) {
    if (is_f32(x, "x")) {
        check_f32(x, "x");
        TORCH_CHECK(x.dim() == 4, "x must be NHWC");
        int NB = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
        TORCH_CHECK(C % 4 == 0,
                    "fp32 global_avg_pool needs C % 4 == 0, got ", C);
        TORCH_CHECK(HW > 0, "empty spatial extent");
        auto out = at::empty({NB, C}, x.options());
        defer_hip::launch_gap_f32(f32ptr(x), out.data_ptr<float>(), NB, HW,
                                  C, cur_stream());
        return out;
    }
    check_bf16(x, "x");
    TORCH_CHECK(x.dim() == 4, "x must be NHWC");
    int NB = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
    TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
    TORCH_CHECK(HW > 0, "empty spatial extent");
    auto out = at::empty({NB, C}, x.options());
    defer_hip::launch_gap(bptr(x), bptr_mut(out), NB, HW, C, cur_stream());
    return out;
}

// NCHW -> NHWC (to_nhwc) or back, converting between fp32 and bf16 on the
// way when bf16_out differs from x's dtype. `out`, when given, is the
// contiguous destination of the right shape and dtype (lets a caller own
// the buffer); otherwise a fresh at::empty tensor. One launch on the
// current stream, no sync, so it can be captured into a hipGraph.
Tensor layout_convert(Tensor x, bool to_nhwc, bool bf16_out,
                      c10::optional<Tensor> out) {
    TORCH_CHECK(x.is_cuda(), "x must be on GPU");
    const bool bf16_in = !is_f32(x, "x");
    TORCH_CHECK(x.dim() == 4, "x must be 4-D (",
                to_nhwc ? "NCHW" : "NHWC", "), got ", x.dim(), "-D");
    TORCH_CHECK(x.is_contiguous(), "x must be contiguous");
    TORCH_CHECK(x.numel() < (1LL << 31), "x has 2^31 or more elements");
    int64_t N = x.size(0), C, H, W;
    if (to_nhwc) { C = x.size(1); H = x.size(2); W = x.size(3); }
    else { H = x.size(1); W = x.size(2); C = x.size(3); }
    std::vector<int64_t> shape =
        to_nhwc ? std::vector<int64_t>{N, H, W, C}
                : std::vector<int64_t>{N, C, H, W};
    auto dt = bf16_out ? at::kBFloat16 : at::kFloat;
    Tensor y;
    if (out) {
        TORCH_CHECK(out->is_cuda() && out->is_contiguous() &&
                    out->scalar_type() == dt && out->sizes().vec() == shape,
                    "out must be a contiguous GPU tensor of the converted "
                    "shape and dtype");
        y = *out;
    } else {
        y = at::empty(shape, x.options().dtype(dt));
    }
    defer_hip::launch_layout(bptr(x), bptr_mut(y), N, (int)C, H * W, to_nhwc,
                             bf16_in, bf16_out, cur_stream());
    return y;
}

std::tuple<int64_t, int64_t, int64_t> field_shape(const Tensor& t) {
    auto sz = t.sizes();
    int nd = sz.size();
    if (nd == 1) return {1, 1, sz[0]};
    if (nd == 2) return {1, sz[0], sz[1]};
    int64_t d0 = 1;
    for (int i = 0; i + 2 < nd; ++i) d0 *= sz[i];
    return {d0, sz[nd - 2], sz[nd - 1]};
}

Tensor zfp_encode(Tensor x, int64_t rate, c10::optional<Tensor> out,
                  int64_t phases = 3) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be GPU contig");
    bool bf16 = x.scalar_type() == at::kBFloat16;
    TORCH_CHECK(bf16 || x.scalar_type() == at::kFloat, "bf16/f32 only");
    auto [d0, d1, d2] = field_shape(x);
    long nb = ((d0 + 3) / 4) * ((d1 + 3) / 4) * ((d2 + 3) / 4);
    long bytes = nb * rate * 8;
    Tensor o;
    if (out) {
        TORCH_CHECK(out->numel() == bytes && out->is_contiguous()
                    && out->scalar_type() == at::kByte, "bad out buffer");
        o = *out;
    } else {
        o = at::empty({bytes},
                      x.options().dtype(at::kByte));
    }
    defer_hip::launch_zfp_encode(bptr(x), bptr_mut(o), bf16, (int)d0,
                                 (int)d1, (int)d2, (int)rate,
                                 cur_stream(), (int)phases);
    return o;
}

Tensor zfp_decode(Tensor wire, std::vector<int64_t> shape, int64_t rate,
                  bool bf16_out) {
    TORCH_CHECK(wire.is_cuda() && wire.is_contiguous()
                && wire.scalar_type() == at::kByte, "bad wire");
    auto o = at::empty(shape, wire.options().dtype(
                                  bf16_out ? at::kBFloat16 : at::kFloat));
    auto [d0, d1, d2] = field_shape(o);
    defer_hip::launch_zfp_decode(bptr(wire), bptr_mut(o), bf16_out,
                                 (int)d0, (int)d1, (int)d2, (int)rate,
                                 cur_stream());
    return o;
}

// fp8 e4m3fn wire: one fused HIP path (init + atomic amax + cast, the
// scale never visits the host) replacing the torch fallback's ~5
// dispatches. Wire layout matches comm.Codec exactly.
void fp8_encode(Tensor x, Tensor out) {
    check_bf16(x, "x");
    long n = x.numel();
    TORCH_CHECK(out.is_cuda() && out.is_contiguous()
                && out.scalar_type() == at::kByte
                && out.numel() == n + 4, "bad fp8 wire buffer");
    defer_hip::launch_fp8_encode(bptr(x), n, bptr_mut(out),
                                 cur_stream());
}

Tensor fp8_decode(Tensor wire, std::vector<int64_t> shape) {
    TORCH_CHECK(wire.is_cuda() && wire.is_contiguous()
                && wire.scalar_type() == at::kByte, "bad wire");
    auto y = at::empty(shape, wire.options().dtype(at::kBFloat16));
    TORCH_CHECK(y.numel() + 4 == wire.numel(), "wire/shape mismatch");
    defer_hip::launch_fp8_decode(bptr(wire), y.numel(), bptr_mut(y),
                                 cur_stream());
    return y;
}

Tensor lz4_compress(Tensor x) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous()
                && x.scalar_type() == at::kByte, "x must be GPU u8 contig");
    long n = x.numel();
    TORCH_CHECK(n > 0, "empty input");
    auto scratch = at::empty({defer_hip::lz4_scratch_bytes(n)},
                             x.options());
    auto o = at::empty({defer_hip::lz4_max_compressed(n)}, x.options());
    defer_hip::launch_lz4_compress(bptr(x), n, bptr_mut(scratch),
                                   bptr_mut(o), cur_stream());
    // total compressed size = header word [2 + nblocks] (syncs the stream;
    // the hop needs the byte count on the host to post the send anyway)
    long nb = (n + 4095) / 4096;
    auto hdr_cpu = o.narrow(0, 4 * (2 + nb), 4).to(at::kCPU);
    uint32_t total;
    std::memcpy(&total, hdr_cpu.data_ptr(), 4);
    return o.narrow(0, 0, 4 * (2 + nb + 1) + (long)total);
}

// Fully async zfp+lz4 hop encode: compress `x` (u8, the ZFP wire) into
// the caller's preallocated worst-case `out` ring slot and write the
// total wire byte count into `len_out` (device int64) — no host sync.
// The hop sends `len_out` as the size message straight from the device
// and reads the host copy one item later (comm.VarP2PRing), keeping the
// sender's host loop ahead of the device (the round-1 version's
// per-item .to(kCPU) sync serialized the pipeline).
void lz4_compress_into(Tensor x, Tensor scratch, Tensor out,
                       Tensor len_out) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous()
                && x.scalar_type() == at::kByte, "x must be GPU u8 contig");
    long n = x.numel();
    TORCH_CHECK(n > 0, "empty input");
    TORCH_CHECK(scratch.numel() >= defer_hip::lz4_scratch_bytes(n)
                && scratch.is_cuda(), "scratch too small");
    TORCH_CHECK(out.numel() >= defer_hip::lz4_max_compressed(n)
                && out.is_cuda() && out.scalar_type() == at::kByte,
                "out too small");
    TORCH_CHECK(len_out.is_cuda() && len_out.numel() == 1
                && len_out.scalar_type() == at::kLong, "bad len_out");
    hipStream_t s = cur_stream();
    defer_hip::launch_lz4_compress(bptr(x), n, bptr_mut(scratch),
                                   bptr_mut(out), s);
    defer_hip::launch_lz4_wire_len(bptr(out), n, bptr_mut(len_out), s);
}

Tensor lz4_decompress(Tensor comp, int64_t raw_len) {
    TORCH_CHECK(comp.is_cuda() && comp.is_contiguous()
                && comp.scalar_type() == at::kByte, "bad comp buffer");
    TORCH_CHECK(raw_len > 0, "raw_len must be positive");
    auto o = at::empty({raw_len}, comp.options());
    defer_hip::launch_lz4_decompress(bptr(comp), bptr_mut(o), raw_len,
                                     cur_stream());
    return o;
}

// ---- lossless wire (csrc/pack.hip, spec in ops/pack_ref.py) ----
static int pack_elem_bits(const Tensor& x) {
    TORCH_CHECK(x.scalar_type() == at::kBFloat16
                || x.scalar_type() == at::kFloat,
                "lossless wire packs bf16 or fp32, got ", x.scalar_type());
    return x.scalar_type() == at::kBFloat16 ? 16 : 32;
}

static void pack_check_numel(long n, int bits) {
    TORCH_CHECK(n > 0, "empty input");
    // chunk_off[] holds u32 word offsets into the payload
    TORCH_CHECK(defer_hip::pack_wire_bytes_max(n, bits) / 4 < (1ll << 32),
                "tensor too large for the lossless wire's u32 offsets");
}

// Fully async lossless hop encode: pack `x` into the caller's worst-case
// `out` ring slot and write the exact wire byte count into `len_out`
// (device int64) — the same contract as lz4_compress_into. Bytes of
// `out` past the wire are left untouched.
void pack_encode_into(Tensor x, Tensor scratch, Tensor out,
                      Tensor len_out) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be GPU contig");
    int bits = pack_elem_bits(x);
    long n = x.numel();
    pack_check_numel(n, bits);
    TORCH_CHECK(scratch.is_cuda() && scratch.is_contiguous()
                && scratch.scalar_type() == at::kByte
                && scratch.numel() >= defer_hip::pack_scratch_bytes(n, bits)
                && (uintptr_t)scratch.data_ptr() % 4 == 0,
                "scratch too small or misaligned");
    TORCH_CHECK(out.is_cuda() && out.is_contiguous()
                && out.scalar_type() == at::kByte
                && out.numel() >= defer_hip::pack_wire_bytes_max(n, bits)
                && (uintptr_t)out.data_ptr() % 4 == 0,
                "out too small or misaligned");
    TORCH_CHECK(len_out.is_cuda() && len_out.numel() == 1
                && len_out.scalar_type() == at::kLong, "bad len_out");
    defer_hip::launch_pack_encode(bptr(x), n, bits == 16,
                                  bptr_mut(scratch), bptr_mut(out),
                                  bptr_mut(len_out), cur_stream());
}

// convenience form: exact-size wire (syncs the stream to read the size)
Tensor pack_encode(Tensor x) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be GPU contig");
    int bits = pack_elem_bits(x);
    long n = x.numel();
    pack_check_numel(n, bits);
    auto bopt = x.options().dtype(at::kByte);
    auto scratch = at::empty({defer_hip::pack_scratch_bytes(n, bits)}, bopt);
    auto o = at::empty({defer_hip::pack_wire_bytes_max(n, bits)}, bopt);
    auto len = at::empty({1}, x.options().dtype(at::kLong));
    defer_hip::launch_pack_encode(bptr(x), n, bits == 16,
                                  bptr_mut(scratch), bptr_mut(o),
                                  bptr_mut(len), cur_stream());
    long total = len.item<int64_t>();
    return o.narrow(0, 0, total);
}

Tensor pack_decode(Tensor wire, std::vector<int64_t> shape, bool bf16_out) {
    TORCH_CHECK(wire.is_cuda() && wire.is_contiguous()
                && wire.scalar_type() == at::kByte
                && (uintptr_t)wire.data_ptr() % 4 == 0, "bad wire");
    auto y = at::empty(shape, wire.options().dtype(
                                  bf16_out ? at::kBFloat16 : at::kFloat));
    long n = y.numel();
    pack_check_numel(n, bf16_out ? 16 : 32);
    TORCH_CHECK(wire.numel() >= defer_hip::pack_table_bytes(n),
                "wire shorter than its tables for this shape");
    defer_hip::launch_pack_decode(bptr(wire), wire.numel(), bptr_mut(y), n,
                                  bf16_out, cur_stream());
    return y;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("conv2d_bn_act", &conv2d_bn_act, py::arg("x"), py::arg("w"),
          py::arg("scale"), py::arg("bias"), py::arg("res"),
          py::arg("stride"), py::arg("pad"), py::arg("act"),
          py::arg("mode") = 0, py::arg("max_blocks") = 0);
    m.def("dwconv2d_bn_act", &dwconv2d_bn_act, py::arg("x"), py::arg("w"),
          py::arg("scale"), py::arg("bias"), py::arg("stride"),
          py::arg("pad"), py::arg("act"));
    m.def("conv_ws_stats", &conv_ws_stats);
    m.def("conv_plan", &conv_plan, py::arg("x_shape"), py::arg("w_shape"),
          py::arg("stride"), py::arg("pad"), py::arg("has_res"),
          py::arg("mode") = 0, py::arg("max_blocks") = 0,
          py::arg("variant") = py::none());
    m.def("conv_table_rows", &defer_hip::conv_table_rows);
    m.def("linear", &linear);
    m.def("bn_act", &bn_act);
    m.def("conv1x1_prebn", &conv1x1_prebn, py::arg("x"),
          py::arg("w"), py::arg("scale"), py::arg("bias"),
          py::arg("out_scale") = py::none(),
          py::arg("out_bias") = py::none());
    m.def("conv1x1_chain", &conv1x1_chain, py::arg("x"), py::arg("w3"),
          py::arg("s3"), py::arg("b3"), py::arg("res"), py::arg("relu3"),
          py::arg("w1"), py::arg("s1"), py::arg("b1"), py::arg("relu1"),
          py::arg("mode") = 0, py::arg("max_blocks") = 0, py::arg("bm") = 0);
    m.def("conv1x1_chain_stats", &conv1x1_chain_stats);
    m.def("conv1x1_chain_proj", &conv1x1_chain_proj, py::arg("x"),
          py::arg("w3"), py::arg("s3"), py::arg("b3"), py::arg("xp"),
          py::arg("wp"), py::arg("sp"), py::arg("bp"), py::arg("relu3"),
          py::arg("w1"), py::arg("s1"), py::arg("b1"), py::arg("relu1"),
          py::arg("mode") = 0, py::arg("max_blocks") = 0);
    m.def("chain_proj_stats", &chain_proj_stats);
    m.def("conv_bn_act_maxpool", &conv_bn_act_maxpool, py::arg("x"),
          py::arg("w"), py::arg("scale"), py::arg("bias"),
          py::arg("stride"), py::arg("pad"), py::arg("relu"),
          py::arg("pool_kernel"), py::arg("pool_stride"),
          py::arg("pool_pad"), py::arg("mode") = 0,
          py::arg("max_blocks") = 0);
    m.def("stem_pool_stats", &stem_pool_stats);
    m.def("add_act", &add_act);
    m.def("relu", &relu);
    m.def("relu6", &relu6);
    m.def("hardswish", &hardswish);
    m.def("squeeze_excite", &squeeze_excite, py::arg("x"), py::arg("w1"),
          py::arg("b1"), py::arg("w2"), py::arg("b2"), py::arg("act"));
    m.def("se_gate", &se_gate, py::arg("x"), py::arg("w1"), py::arg("b1"),
          py::arg("w2"), py::arg("b2"), py::arg("act"));
    m.def("channel_scale", &channel_scale);
    m.def("softmax", &softmax);
    m.def("maxpool2d", &maxpool2d);
    m.def("avgpool2d", &avgpool2d);
    m.def("concat_lastdim", &concat_lastdim);
    m.def("global_avg_pool", &global_avg_pool);
    m.def("layout_convert", &layout_convert, py::arg("x"),
          py::arg("to_nhwc"), py::arg("bf16_out"),
          py::arg("out") = py::none());
    m.def("zfp_encode", &zfp_encode, py::arg("x"), py::arg("rate"),
          py::arg("out") = py::none(), py::arg("phases") = 3);
    m.def("zfp_decode", &zfp_decode);
    m.def("fp8_encode", &fp8_encode);
    m.def("fp8_decode", &fp8_decode);
    m.def("lz4_compress", &lz4_compress);
    m.def("lz4_compress_into", &lz4_compress_into);
    m.def("lz4_scratch_bytes",
          [](int64_t n) { return defer_hip::lz4_scratch_bytes(n); });
    m.def("lz4_decompress", &lz4_decompress);
    m.def("pack_scratch_bytes", [](int64_t n, int64_t bits) {
        return defer_hip::pack_scratch_bytes(n, (int)bits);
    });
    m.def("pack_wire_bytes_max", [](int64_t n, int64_t bits) {
        return defer_hip::pack_wire_bytes_max(n, (int)bits);
    });
    m.def("pack_encode_into", &pack_encode_into);
    m.def("pack_encode", &pack_encode);
    m.def("pack_decode", &pack_decode);
}
