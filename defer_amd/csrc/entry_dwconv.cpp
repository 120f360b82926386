// Torch entry points of the depthwise and grouped convs (dwconv.hip,
// dwconv7.hip, gconv.hip). Everything the kernels do not serve is refused
// here; there is no other path.
#include "entry_util.h"

namespace {

using namespace defer_bind;

// Depthwise conv + folded BN + activation: x NHWC, w [R, S, C], both bf16 or
// both fp32.
Tensor dwconv2d_bn_act(Tensor x, Tensor w, c10::optional<Tensor> scale,
                       c10::optional<Tensor> bias, int64_t stride,
                       int64_t pad, int64_t act) {
    const char* op = "dwconv2d_bn_act";
    check_act(act);
    const bool f32 = check_pair(x, w, "w", true);
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
    const ConvOut g = conv_out_geom(NB, H, W, C, C, R, S, stride, pad, true);
    const float* sc = f32_vec(scale, ones_buf(), x, op, "scale", C);
    const float* bi = f32_vec(bias, zeros_buf(), x, op, "bias", C);
    auto out = at::empty({NB, g.OH, g.OW, C}, x.options());
    if (out.numel() == 0) return out;
    if (f32)
        defer_hip::launch_dwconv_f32(f32ptr(x), f32ptr(w), sc, bi,
                                     out.data_ptr<float>(), (int)NB, (int)H,
                                     (int)W, (int)C, (int)g.OH, (int)g.OW,
                                     (int)R, (int)stride, (int)pad,
                                     (int)act, cur_stream());
    else
        defer_hip::launch_dwconv(bptr(x), bptr(w), sc, bi, bptr_mut(out),
                                 (int)NB, (int)H, (int)W, (int)C, (int)g.OH,
                                 (int)g.OW, (int)R, (int)stride, (int)pad,
                                 (int)act, cur_stream());
    return out;
}

// 7x7 depthwise conv, stride 1, padding 3, + bias: x NHWC, w [7, 7, C], both
// bf16 or both fp32. max_blocks caps the grid along the tiles (0 = policy).
Tensor dwconv7x7(Tensor x, Tensor w, c10::optional<Tensor> bias,
                 int64_t max_blocks) {
    TORCH_CHECK(x.dim() == 4, "dwconv7x7: x must be NHWC");
    TORCH_CHECK(w.dim() == 3, "dwconv7x7: w must be [7, 7, C]");
    const bool f32 = check_channel_vec(x, "dwconv7x7");
    TORCH_CHECK(w.is_cuda() && w.scalar_type() == x.scalar_type() &&
                w.is_contiguous() && aligned16(w),
                "dwconv7x7: w must be a contiguous GPU tensor of x's dtype "
                "(mixed dtypes)");
    int64_t NB = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
    TORCH_CHECK(w.size(0) == 7 && w.size(1) == 7 && w.size(2) == C,
                "dwconv7x7: w must be [7, 7, C] with C = ", C);
    TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0");
    TORCH_CHECK(H * W * C < (1LL << 31),
                "dwconv7x7: an image has 2^31 or more elements");
    const float* bi = f32_vec(bias, zeros_buf(), x, "dwconv7x7", "bias", C,
                              {false, true});
    auto out = at::empty_like(x);
    if (out.numel() == 0) return out;
    defer_hip::launch_dwconv7(bptr(x), bptr(w), bi, bptr_mut(out), (int)NB,
                              (int)H, (int)W, (int)C, f32, (int)max_blocks,
                              cur_stream());
    return out;
}

// What dwconv7x7 launches for an NHWC shape: the tile policy of dw7_geom.
// Needs no GPU.
py::dict dwconv7x7_plan(std::vector<int64_t> xs, bool f32) {
    using namespace pybind11::literals;
    TORCH_CHECK(xs.size() == 4, "x must be NHWC");
    const auto g = defer_hip::dw7_geom((int)xs[0], (int)xs[1], (int)xs[2],
                                       (int)xs[3], f32 ? 4 : 8);
    return py::dict("TH"_a = g.TH, "TW"_a = g.TW, "nth"_a = g.nth,
                    "ntw"_a = g.ntw, "CBV"_a = g.CBV, "PV"_a = g.PV,
                    "ncb"_a = g.ncb, "lds_bytes"_a = g.lds_bytes,
                    "tiles"_a = g.tiles);
}

// Grouped 3x3 conv + folded BN + activation: x NHWC, w [C, 3, 3, Cg] with
// Cg = C / groups, both bf16 or both fp32.
Tensor gconv2d_bn_act(Tensor x, Tensor w, c10::optional<Tensor> scale,
                      c10::optional<Tensor> bias, int64_t stride,
                      int64_t pad, int64_t act) {
    const char* op = "gconv2d_bn_act";
    check_act(act);
    const bool f32 = check_pair(x, w, "w", true);
    TORCH_CHECK(x.dim() == 4, "x must be NHWC");
    TORCH_CHECK(w.dim() == 4, "w must be [C, 3, 3, Cg]");
    int64_t NB = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
    int64_t R = w.size(1), S = w.size(2), Cg = w.size(3);
    TORCH_CHECK(w.size(0) == C, "grouped conv needs Cout == Cin, got w with ",
                w.size(0), " output channels for x with ", C);
    TORCH_CHECK(R == 3 && S == 3, "grouped conv needs a 3x3 kernel, got ", R,
                "x", S);
    TORCH_CHECK(Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32,
                "grouped conv needs 4, 8, 16 or 32 channels per group, got ",
                Cg);
    TORCH_CHECK(C > 0 && C % 16 == 0 && C % Cg == 0,
                "grouped conv needs C % 16 == 0 and C % Cg == 0, got C = ",
                C, " with Cg = ", Cg);
    TORCH_CHECK(stride == 1 || stride == 2,
                "grouped conv needs stride 1 or 2, got ", stride);
    TORCH_CHECK(pad == 0 || pad == 1,
                "grouped conv needs padding 0 or 1, got ", pad);
    const ConvOut g = conv_out_geom(NB, H, W, C, C, 3, 3, stride, pad, true);
    TORCH_CHECK(C <= 64 * 65535, "grouped conv takes at most C = ",
                64 * 65535, ", got ", C);
    const float* sc = f32_vec(scale, ones_buf(), x, op, "scale", C);
    const float* bi = f32_vec(bias, zeros_buf(), x, op, "bias", C);
    auto out = at::empty({NB, g.OH, g.OW, C}, x.options());
    if (out.numel() == 0) return out;
    if (f32)
        defer_hip::launch_gconv_f32(f32ptr(x), f32ptr(w), sc, bi,
                                    out.data_ptr<float>(), (int)NB, (int)H,
                                    (int)W, (int)C, (int)g.OH, (int)g.OW,
                                    (int)Cg, (int)stride, (int)pad, (int)act,
                                    cur_stream());
    else
        defer_hip::launch_gconv(bptr(x), bptr(w), sc, bi, zero_buf(),
                                bptr_mut(out), (int)NB, (int)H, (int)W,
                                (int)C, (int)g.OH, (int)g.OW, (int)Cg,
                                (int)stride, (int)pad, (int)act,
                                cur_stream());
    return out;
}

}  // namespace

void bind_dwconv(py::module_& m) {
    m.def("dwconv2d_bn_act", &dwconv2d_bn_act, py::arg("x"), py::arg("w"),
          py::arg("scale"), py::arg("bias"), py::arg("stride"),
          py::arg("pad"), py::arg("act"));
    m.def("dwconv7x7", &dwconv7x7, py::arg("x"), py::arg("w"),
          py::arg("bias"), py::arg("max_blocks") = 0);
    m.def("dwconv7x7_plan", &dwconv7x7_plan, py::arg("x_shape"),
          py::arg("f32") = false);
    m.def("gconv2d_bn_act", &gconv2d_bn_act, py::arg("x"), py::arg("w"),
          py::arg("scale"), py::arg("bias"), py::arg("stride"),
          py::arg("pad"), py::arg("act"));
}
