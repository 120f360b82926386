// Torch entry points of the dense conv family: the fp32 and bf16 conv and
// linear, the fused 1x1 chains and the fused stem, with the plan queries and
// the launch counters the tests read.
#include <cmath>
#include <cstdlib>
#include <string>

#include "entry_util.h"
#include "conv_plan.h"

namespace {

using namespace defer_bind;
using defer_hip::ConvParams;

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
    const ConvOut g = conv_out_geom(NB, H, W, Cin, Cout, R, S, stride, pad,
                                    true);
    const int OH = (int)g.OH, OW = (int)g.OW;
    const float* sc = f32_vec(scale, nullptr, x, "conv2d_bn_act", "scale",
                              Cout, {true, false});
    const float* bi = f32_vec(bias, nullptr, x, "conv2d_bn_act", "bias",
                              Cout, {true, false});
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
        run_conv_f32(xp, wp, sc, bi, res, out, g.M, H, W, C4, OH, OW, R, S,
                     (int)stride, (int)pad, act);
        return out;
    }
    run_conv_f32(x, w, sc, bi, res, out, g.M, H, W, Cin, OH, OW, R, S,
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
    const float* bi = f32_vec(bias, nullptr, x, "linear", "bias", N,
                              {true, false});
    auto out = at::empty({M, N}, x.options());
    run_conv_f32(x, w, nullptr, bi, c10::nullopt, out, M, 1, 1, K, 1, 1, 1,
                 1, 1, 0, ACT_NONE);
    return out;
}

// ---- bf16 path ----

// What the kernels with a launch policy did, for tests: launches in this
// process and the grid (and tile split) of the last one.
LaunchStats ws_stats{"blocks", "tiles_per_block"};      // conv_ws.hip
LaunchStats chain_stats{"blocks", "bm"};                // chain.hip
LaunchStats chain_proj_stats{"blocks"};                 // chain.hip, projected
LaunchStats stem_pool_stats{"bands", "rows_per_band"};  // stem_pool.hip

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
    // the bf16 kernels' element offsets are 64-bit: only M is bounded
    const ConvOut o = conv_out_geom(NB, H, W, Cin, Cout, R, S, stride, pad,
                                    false);
    int OH = g.OH = (int)o.OH;
    int OW = g.OW = (int)o.OW;
    long M = o.M;
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
// max_blocks caps that kernel's grid (0 = policy). act: ACT_NONE, ACT_RELU,
// ACT_RELU6 or ACT_HARDSWISH. ReLU6 runs the ReLU instantiation of whichever
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
    const int kact = act == ACT_NONE ? 0 : act == ACT_HARDSWISH ? 2 : 1;
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
    ConvParams p = g.p;
    p.scale = f32_vec(scale, ones_buf(), x, "conv2d_bn_act", "scale", Cout);
    p.bias = f32_vec(bias, zeros_buf(), x, "conv2d_bn_act", "bias", Cout);
    auto out = at::empty({NB, g.OH, g.OW, Cout}, x.options());
    if (res) check_bf16(*res, "res");
    hipStream_t s = cur_stream();

    p.res = res ? bptr(*res) : nullptr;
    p.out = bptr_mut(out);
    p.zbuf = zero_buf();
    if (act == ACT_RELU6) p.act_hi = 6.0f;

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
        ws_stats.record(used.blocks, used.tiles_per_block);
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
    p.scale = f32_vec(c10::nullopt, ones_buf(), x, "linear", "scale", N);
    p.bias = f32_vec(bias_f, zeros_buf(), x, "linear", "bias", N);
    p.res = nullptr; p.out = bptr_mut(out); p.zbuf = zero_buf();
    const auto plan = defer_hip::plan_conv(p, true, false, 2, 0,
                                           defer_hip::conv_variant());
    defer_hip::launch_conv_igemm(p, plan, false, false, cur_stream());
    return out;
}

// gelu(x[M, K] @ w[N, K]^T + bias): linear with the GELU epilogue. bf16: the
// GEMM-mode plan of linear, run on its ACT_GELU instantiation; fp32: the
// runtime act of conv_f32_kernel. The shape rules are linear's.
Tensor linear_gelu(Tensor x, Tensor w, c10::optional<Tensor> bias) {
    TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "linear_gelu wants 2-D");
    const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
    TORCH_CHECK(w.size(1) == K, "K mismatch");
    TORCH_CHECK(M < (1LL << 31), "M too large");
    auto out = at::empty({M, N}, x.options());
    c10::optional<Tensor> bias_f;
    if (bias) {
        TORCH_CHECK(bias->is_cuda() && bias->numel() == N,
                    "linear_gelu: bias must be a GPU tensor of Cout = ", N,
                    " values");
        bias_f = bias->scalar_type() == at::kFloat && bias->is_contiguous()
                     ? *bias
                     : cached_weight_prep(*bias, -1, [&] {
                           return bias->to(at::kFloat).contiguous();
                       });
    }
    if (is_f32(x, "x")) {
        check_f32(x, "x");
        check_f32(w, "w");
        TORCH_CHECK(K % 4 == 0, "fp32 linear_gelu needs K % 4 == 0, got ", K);
        TORCH_CHECK(N % 4 == 0, "fp32 linear_gelu needs N % 4 == 0, got ", N);
        run_conv_f32(x, w, nullptr,
                     f32_vec(bias_f, nullptr, x, "linear_gelu", "bias", N,
                             {true, false}),
                     c10::nullopt, out, M, 1, 1, (int)K, 1, 1, 1, 1, 1, 0,
                     ACT_GELU);
        return out;
    }
    check_bf16(x, "x");
    check_bf16(w, "w");
    TORCH_CHECK(K % 8 == 0, "K must be a multiple of 8");
    if (M == 0) return out;
    ConvParams p = conv_geom(M, (int)K, (int)N, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0,
                             true);
    p.x = bptr(x); p.w = bptr(w);
    p.scale = f32_vec(c10::nullopt, ones_buf(), x, "linear_gelu", "scale", N);
    p.bias = f32_vec(bias_f, zeros_buf(), x, "linear_gelu", "bias", N);
    p.res = nullptr; p.out = bptr_mut(out); p.zbuf = zero_buf();
    const auto plan = defer_hip::plan_conv(p, true, false, 2, 0,
                                           defer_hip::conv_variant());
    defer_hip::launch_gemm_gelu(p, plan, cur_stream());
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
    const float* ps = f32_vec(scale, x, "conv1x1_prebn", "scale", Cin);
    const float* pb = f32_vec(bias, x, "conv1x1_prebn", "bias", Cin);
    long M = (long)NB * H * W;
    TORCH_CHECK(M < (1LL << 31), "M too large");
    TORCH_CHECK(!out_scale || out_bias, "out_scale needs out_bias");
    const float* os = nullptr;
    const float* ob = nullptr;
    if (out_scale) {
        os = f32_vec(*out_scale, x, "conv1x1_prebn", "out_scale", Cout);
        ob = f32_vec(*out_bias, x, "conv1x1_prebn", "out_bias", Cout);
    }
    auto out = at::empty({NB, H, W, Cout}, x.options());
    defer_hip::launch_gemm_prebn(bptr(x), bptr(w), ps, pb, os, ob,
                                 zero_buf(), bptr_mut(out), (int)M, Cin,
                                 Cout, cur_stream());
    return out;
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
    const char* op = "conv1x1_chain";
    const float* ps3 = f32_vec(s3, ones_buf(), x, op, "s3", N1);
    const float* pb3 = f32_vec(b3, zeros_buf(), x, op, "b3", N1);
    const float* ps1 = f32_vec(s1, ones_buf(), x, op, "s1", N2);
    const float* pb1 = f32_vec(b1, zeros_buf(), x, op, "b1", N2);
    long M = (long)NB * H * W;
    TORCH_CHECK(M < (1LL << 31), "M too large");
    if (mode != 2 && K1 % 64 == 0 && N1 % 64 == 0 && N2 % 64 == 0) {
        auto y = at::empty({NB, H, W, N1}, x.options());
        auto a2 = at::empty({NB, H, W, N2}, x.options());
        defer_hip::ChainLaunch l = defer_hip::launch_conv1x1_chain(
            bptr(x), bptr(w3), ps3, pb3, bptr(res), bptr_mut(y), relu3,
            bptr(w1), ps1, pb1, bptr_mut(a2), relu1, (int)M, K1, N1, N2,
            mode == 1, (int)max_blocks, (int)bm, cur_stream());
        if (l.blocks > 0) {
            chain_stats.record(l.blocks, l.bm);
            return {y, a2};
        }
    }
    auto y = conv2d_bn_act(x, w3, s3, b3, res, 1, 0, relu3);
    auto a2 = conv2d_bn_act(y, w1, s1, b1, c10::nullopt, 1, 0, relu1);
    return {y, a2};
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
    const char* op = "conv1x1_chain_proj";
    const float* ps3 = f32_vec(s3, ones_buf(), x, op, "s3", N1);
    const float* pb3 = f32_vec(b3, zeros_buf(), x, op, "b3", N1);
    const float* psp = f32_vec(sp, ones_buf(), x, op, "sp", N1);
    const float* pbp = f32_vec(bp, zeros_buf(), x, op, "bp", N1);
    const float* ps1 = f32_vec(s1, ones_buf(), x, op, "s1", N2);
    const float* pb1 = f32_vec(b1, zeros_buf(), x, op, "b1", N2);
    long M = (long)NB * H * W;
    TORCH_CHECK(M < (1LL << 31), "M too large");
    if (K1 != 64 || KP != 64 || N2 != 64 || N1 % 64 != 0 || M == 0)
        return c10::nullopt;
    auto y = at::empty({NB, H, W, N1}, x.options());
    auto a2 = at::empty({NB, H, W, N2}, x.options());
    int blocks = defer_hip::launch_conv1x1_chain_proj(
        bptr(x), bptr(w3), ps3, pb3, bptr(xp), bptr(wp), psp, pbp,
        bptr_mut(y), relu3, bptr(w1), ps1, pb1, bptr_mut(a2), relu1, (int)M,
        K1, KP, N1, N2, mode == 1, (int)max_blocks, cur_stream());
    if (blocks == 0) return c10::nullopt;
    chain_proj_stats.record(blocks);
    return std::make_tuple(y, a2);
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
    const char* op = "conv_bn_act_maxpool";
    const float* sc = f32_vec(scale, ones_buf(), x, op, "scale", Cout);
    const float* bi = f32_vec(bias, zeros_buf(), x, op, "bias", Cout);
    // a gate of the fused path, not a refusal: the composed path below has
    // conv2d_bn_act's rules
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
        q.scale = sc;
        q.bias = bi;
        q.out = bptr_mut(out);
        q.NB = NB; q.H = H; q.W = W;
        q.OH = OH; q.OW = OW; q.POH = POH; q.POW = POW;
        auto used = defer_hip::launch_stem_pool(q, (int)max_blocks, s);
        stem_pool_stats.record(used.bands, used.rpb);
        return out;
    }
    auto y = conv2d_bn_act(x, w, scale, bias, c10::nullopt, stride, pad,
                           relu);
    return maxpool2d(y, pool_kernel, pool_stride, pool_pad);
}

}  // namespace

void bind_conv(py::module_& m) {
    m.def("conv2d_bn_act", &conv2d_bn_act, py::arg("x"), py::arg("w"),
          py::arg("scale"), py::arg("bias"), py::arg("res"),
          py::arg("stride"), py::arg("pad"), py::arg("act"),
          py::arg("mode") = 0, py::arg("max_blocks") = 0);
    m.def("conv_plan", &conv_plan, py::arg("x_shape"), py::arg("w_shape"),
          py::arg("stride"), py::arg("pad"), py::arg("has_res"),
          py::arg("mode") = 0, py::arg("max_blocks") = 0,
          py::arg("variant") = py::none());
    m.def("conv_table_rows", &defer_hip::conv_table_rows);
    m.def("conv_ws_stats", [] { return ws_stats.to_dict(); });
    m.def("linear", &linear);
    m.def("linear_gelu", &linear_gelu, py::arg("x"), py::arg("w"),
          py::arg("bias"));
    m.def("conv1x1_prebn", &conv1x1_prebn, py::arg("x"),
          py::arg("w"), py::arg("scale"), py::arg("bias"),
          py::arg("out_scale") = py::none(),
          py::arg("out_bias") = py::none());
    m.def("conv1x1_chain", &conv1x1_chain, py::arg("x"), py::arg("w3"),
          py::arg("s3"), py::arg("b3"), py::arg("res"), py::arg("relu3"),
          py::arg("w1"), py::arg("s1"), py::arg("b1"), py::arg("relu1"),
          py::arg("mode") = 0, py::arg("max_blocks") = 0, py::arg("bm") = 0);
    m.def("conv1x1_chain_stats", [] { return chain_stats.to_dict(); });
    m.def("conv1x1_chain_proj", &conv1x1_chain_proj, py::arg("x"),
          py::arg("w3"), py::arg("s3"), py::arg("b3"), py::arg("xp"),
          py::arg("wp"), py::arg("sp"), py::arg("bp"), py::arg("relu3"),
          py::arg("w1"), py::arg("s1"), py::arg("b1"), py::arg("relu1"),
          py::arg("mode") = 0, py::arg("max_blocks") = 0);
    m.def("chain_proj_stats", [] { return chain_proj_stats.to_dict(); });
    m.def("conv_bn_act_maxpool", &conv_bn_act_maxpool, py::arg("x"),
          py::arg("w"), py::arg("scale"), py::arg("bias"),
          py::arg("stride"), py::arg("pad"), py::arg("relu"),
          py::arg("pool_kernel"), py::arg("pool_stride"),
          py::arg("pool_pad"), py::arg("mode") = 0,
          py::arg("max_blocks") = 0);
    m.def("stem_pool_stats", [] { return stem_pool_stats.to_dict(); });
}

