// Torch entry points of the fp8 (OCP e4m3) conv path (conv_fp8.hip).
#include <cmath>

#include "entry_util.h"

namespace {

using namespace defer_bind;

// e4m3(clamp(x * inv_scale, -448, 448)), round to nearest even; x bf16 or
// fp32 with numel % 16 == 0
Tensor quantize_fp8(Tensor x, double inv_scale, int64_t max_blocks) {
    const bool f32 = check_dtype(x, "x", true);
    TORCH_CHECK(x.numel() % 16 == 0, "quantize_fp8 needs numel % 16 == 0, "
                "got ", x.numel());
    auto out = at::empty(x.sizes(), x.options().dtype(at::kFloat8_e4m3fn));
    if (out.numel() == 0) return out;
    defer_hip::launch_quantize_fp8(bptr(x), out.data_ptr(), x.numel(), f32,
                                   (float)inv_scale, (int)max_blocks,
                                   cur_stream());
    return out;
}

struct Fp8Geom { int64_t NB, H, W, Cin, Cout, R, S, OH, OW, M, K; };

// the geometry conv_fp8_kernel serves; everything else is refused
Fp8Geom fp8_geom(at::IntArrayRef xs, at::IntArrayRef ws, int64_t stride,
                 int64_t pad) {
    TORCH_CHECK(xs.size() == 4, "x must be NHWC");
    TORCH_CHECK(ws.size() == 4, "w must be OHWI");
    Fp8Geom g{xs[0], xs[1], xs[2], xs[3], ws[0], ws[1], ws[2]};
    TORCH_CHECK(ws[3] == g.Cin, "w has ", ws[3], " input channels, x ",
                g.Cin);
    TORCH_CHECK(g.Cin > 0 && g.Cin % 16 == 0 && g.Cout > 0 &&
                g.Cout % 16 == 0,
                "fp8 conv needs Cin % 16 == 0 and Cout % 16 == 0, got ",
                g.Cin, " and ", g.Cout);
    TORCH_CHECK(g.R == g.S && g.R >= 1, "fp8 conv needs a square kernel, "
                "got ", g.R, "x", g.S);
    TORCH_CHECK(stride == 1 || stride == 2,
                "fp8 conv needs stride 1 or 2, got ", stride);
    TORCH_CHECK(pad >= 0 && pad <= g.R / 2,
                "fp8 conv needs 0 <= padding <= R / 2, got ", pad);
    const ConvOut o = conv_out_geom(g.NB, g.H, g.W, g.Cin, g.Cout, g.R, g.S,
                                    stride, pad, true);
    g.OH = o.OH;
    g.OW = o.OW;
    g.M = o.M;
    g.K = g.R * g.S * g.Cin;
    TORCH_CHECK(g.Cout * g.K < (1LL << 31), "w has 2^31 or more elements");
    return g;
}

py::dict fp8_plan_dict(const defer_hip::ConvFp8Plan& pl) {
    py::dict d;
    d["tile"] = pl.bm == 128 ? "large" : "small";
    d["bm"] = pl.bm;
    d["bn"] = pl.bn;
    d["m_tiles"] = pl.ntm;
    d["n_tiles"] = pl.ntn;
    d["k_tiles"] = pl.ktiles;
    d["mfma"] = pl.narrow ? "bf16" : "fp8";
    d["grid"] = pl.grid;
    d["lds_bytes"] = pl.lds_bytes;
    return d;
}

py::dict conv_fp8_plan(std::vector<int64_t> xs, std::vector<int64_t> ws,
                       int64_t stride, int64_t pad, int64_t max_blocks) {
    const Fp8Geom g = fp8_geom(xs, ws, stride, pad);
    return fp8_plan_dict(defer_hip::plan_conv_fp8(
        g.M, (int)g.Cout, (int)g.K, (int)max_blocks));
}

Tensor conv2d_bn_act_fp8(Tensor x, Tensor w, Tensor scale, Tensor bias,
                         c10::optional<Tensor> res, int64_t stride,
                         int64_t pad, int64_t act, double res_scale,
                         c10::optional<double> out_inv_scale,
                         int64_t max_blocks) {
    const char* op = "conv2d_bn_act_fp8";
    TORCH_CHECK(act >= ACT_NONE && act <= ACT_RELU6,
                "fp8 conv act must be 0 (none), 1 (relu) or 2 (relu6), got ",
                act);
    check_e4m3(x, "x");
    check_e4m3(w, "w");
    const Fp8Geom g = fp8_geom(x.sizes(), w.sizes(), stride, pad);
    defer_hip::ConvFp8Params p{};
    p.x = (const unsigned char*)x.data_ptr();
    p.w = (const unsigned char*)w.data_ptr();
    p.scale = f32_vec(scale, x, op, "scale", g.Cout, {true, false});
    p.bias = f32_vec(bias, x, op, "bias", g.Cout, {true, false});
    if (res) {
        check_e4m3(*res, "residual");
        TORCH_CHECK(res->dim() == 4 && res->size(0) == g.NB &&
                    res->size(1) == g.OH && res->size(2) == g.OW &&
                    res->size(3) == g.Cout,
                    "residual must have the output's shape");
        p.res = (const unsigned char*)res->data_ptr();
    }
    auto out = at::empty(
        {g.NB, g.OH, g.OW, g.Cout},
        x.options().dtype(out_inv_scale ? at::kFloat8_e4m3fn
                                        : at::kBFloat16));
    if (out.numel() == 0) return out;
    p.out = out.data_ptr();
    p.zbuf = zero_buf();
    p.M = (int)g.M; p.K = (int)g.K; p.Cout = (int)g.Cout;
    p.Cin = (int)g.Cin; p.S = (int)g.S;
    if (g.R == 1 && stride == 1) {      // GEMM mode: one row of M pixels
        p.H = 1; p.W = (int)g.M; p.OH = 1; p.OW = (int)g.M;
        p.stride = 1; p.pad = 0;
    } else {
        p.H = (int)g.H; p.W = (int)g.W; p.OH = (int)g.OH; p.OW = (int)g.OW;
        p.stride = (int)stride; p.pad = (int)pad;
    }
    p.act_lo = act == ACT_NONE ? -INFINITY : 0.0f;
    p.act_hi = act == ACT_RELU6 ? 6.0f : INFINITY;
    p.res_scale = (float)res_scale;
    p.out_fp8 = out_inv_scale ? 1 : 0;
    p.out_inv_scale = out_inv_scale ? (float)*out_inv_scale : 1.0f;
    defer_hip::launch_conv_fp8(p, (int)max_blocks, cur_stream());
    return out;
}

}  // namespace

void bind_fp8(py::module_& m) {
    m.def("quantize_fp8", &quantize_fp8, py::arg("x"), py::arg("inv_scale"),
          py::arg("max_blocks") = 0);
    m.def("conv2d_bn_act_fp8", &conv2d_bn_act_fp8, py::arg("x"), py::arg("w"),
          py::arg("scale"), py::arg("bias"), py::arg("residual"),
          py::arg("stride"), py::arg("pad"), py::arg("act"),
          py::arg("res_scale"), py::arg("out_inv_scale"),
          py::arg("max_blocks") = 0);
    m.def("conv_fp8_plan", &conv_fp8_plan, py::arg("x_shape"),
          py::arg("w_shape"), py::arg("stride"), py::arg("pad"),
          py::arg("max_blocks") = 0);
}
