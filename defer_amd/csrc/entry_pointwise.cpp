// Torch entry points of the pointwise, pooling and normalisation ops
// (elementwise.hip, ops_f32.hip, pool.hip, se.hip, layernorm.hip,
// layout.hip). Each op serves bf16 and fp32 through one body: the checks are
// shared, the launcher is picked by the dtype.
#include "entry_util.h"

namespace {

using namespace defer_bind;

Tensor bn_act(Tensor x, Tensor scale, Tensor bias, bool relu) {
    const bool f32 = check_dtype(x, "x");
    int C = x.size(-1);
    const int vec = check_vec(C, f32, "bn_act", "C");
    TORCH_CHECK(scale.is_cuda() && bias.is_cuda() &&
                scale.numel() == C && bias.numel() == C,
                "scale/bias must be GPU tensors of length C");
    auto out = at::empty_like(x);
    auto sf = scale.to(at::kFloat).contiguous();
    auto bf = bias.to(at::kFloat).contiguous();
    if (f32)
        defer_hip::launch_bn_act_f32(f32ptr(x), f32ptr(sf), f32ptr(bf),
                                     out.data_ptr<float>(), x.numel() / vec,
                                     C / vec, relu, cur_stream());
    else
        defer_hip::launch_bn_act(bptr(x), f32ptr(sf), f32ptr(bf),
                                 bptr_mut(out), x.numel() / vec, C / vec,
                                 relu, cur_stream());
    return out;
}

Tensor add_act(Tensor a, Tensor b, bool relu) {
    const bool f32 = check_dtype(a, "a");
    check_as(b, "b", f32, false);
    TORCH_CHECK(a.sizes() == b.sizes(), "shape mismatch");
    const int vec = check_vec(a.numel(), f32, "add_act", "numel");
    auto out = at::empty_like(a);
    if (f32)
        defer_hip::launch_add_act_f32(f32ptr(a), f32ptr(b),
                                      out.data_ptr<float>(), a.numel() / vec,
                                      relu, cur_stream());
    else
        defer_hip::launch_add_act(bptr(a), bptr(b), bptr_mut(out),
                                  a.numel() / vec, relu, cur_stream());
    return out;
}

// relu, relu6 and hardswish: one body, the launcher pair differs
using UnaryBf16 = void (*)(const void*, void*, long, hipStream_t);
using UnaryF32 = void (*)(const float*, float*, long, hipStream_t);

Tensor unary(const Tensor& x, const char* op, UnaryBf16 bf16, UnaryF32 fp32) {
    const bool f32 = check_dtype(x, "x");
    const int vec = check_vec(x.numel(), f32, op, "numel");
    auto out = at::empty_like(x);
    if (f32)
        fp32(f32ptr(x), out.data_ptr<float>(), x.numel() / vec, cur_stream());
    else
        bf16(bptr(x), bptr_mut(out), x.numel() / vec, cur_stream());
    return out;
}

Tensor relu(Tensor x) {
    return unary(x, "relu", defer_hip::launch_relu,
                 defer_hip::launch_relu_f32);
}
Tensor relu6(Tensor x) {
    return unary(x, "relu6", defer_hip::launch_relu6,
                 defer_hip::launch_relu6_f32);
}
Tensor hardswish(Tensor x) {
    return unary(x, "hardswish", defer_hip::launch_hardswish,
                 defer_hip::launch_hardswish_f32);
}

// The gate of squeeze-excite (csrc/se.hip), fp32 [N, C]:
// g = hardsigmoid(w2 @ act(w1 @ mean_hw(x) + b1) + b2), all in fp32. One
// launch on the current stream, no host sync. act: ACT_NONE or ACT_RELU.
// The kernel's LDS holds the C means and the Cr hidden values in fp32.
Tensor se_gate(Tensor x, Tensor w1, c10::optional<Tensor> b1, Tensor w2,
               c10::optional<Tensor> b2, int64_t act) {
    TORCH_CHECK(act == ACT_NONE || act == ACT_RELU,
                "squeeze_excite: act must be 0 (none) or 1 (relu), got ",
                act);
    const bool f32 = check_pair(x, w1, "w1", true);
    check_as(w2, "w2", f32, true);
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
    // absent = null: the kernel adds nothing
    const float* bp1 = f32_vec(b1, nullptr, x, "squeeze_excite", "b1", Cr,
                               {false, true});
    const float* bp2 = f32_vec(b2, nullptr, x, "squeeze_excite", "b2", C,
                               {false, true});
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
    const bool f32 = check_dtype(x, "x", true);
    check_f32(g, "g");
    TORCH_CHECK(g.device() == x.device(),
                "channel_scale: g must be on x's device");
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

Tensor softmax(Tensor x) {
    const bool f32 = check_dtype(x, "x");
    TORCH_CHECK(x.dim() >= 1 && x.numel() > 0, "softmax of nothing");
    int cols = x.size(-1);
    long rows = x.numel() / cols;
    auto out = at::empty_like(x);
    if (f32)
        defer_hip::launch_softmax_f32(f32ptr(x), out.data_ptr<float>(),
                                      (int)rows, cols, cur_stream());
    else
        defer_hip::launch_softmax(bptr(x), bptr_mut(out), (int)rows, cols,
                                  cur_stream());
    return out;
}

// maxpool2d and avgpool2d: one body, the launcher pair differs
using PoolBf16 = void (*)(const void*, void*, int, int, int, int, int, int,
                          int, int, int, hipStream_t);
using PoolF32 = void (*)(const float*, float*, int, int, int, int, int, int,
                         int, int, int, hipStream_t);

Tensor pool2d(const Tensor& x, int64_t kernel, int64_t stride, int64_t pad,
              const char* op, PoolBf16 bf16, PoolF32 fp32) {
    const bool f32 = check_dtype(x, "x");
    check_pool(x, kernel, stride, pad, op);
    int NB = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
    check_vec(C, f32, op, "C");
    int OH = (int)((H + 2 * pad - kernel) / stride + 1);
    int OW = (int)((W + 2 * pad - kernel) / stride + 1);
    auto out = at::empty({NB, OH, OW, C}, x.options());
    if (f32)
        fp32(f32ptr(x), out.data_ptr<float>(), NB, H, W, C, OH, OW,
             (int)kernel, (int)stride, (int)pad, cur_stream());
    else
        bf16(bptr(x), bptr_mut(out), NB, H, W, C, OH, OW, (int)kernel,
             (int)stride, (int)pad, cur_stream());
    return out;
}

Tensor avgpool2d(Tensor x, int64_t kernel, int64_t stride, int64_t pad) {
    return pool2d(x, kernel, stride, pad, "avgpool2d",
                  defer_hip::launch_avgpool, defer_hip::launch_avgpool_f32);
}

Tensor global_avg_pool(Tensor x) {
    const bool f32 = check_dtype(x, "x");
    TORCH_CHECK(x.dim() == 4, "x must be NHWC");
    int NB = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
    check_vec(C, f32, "global_avg_pool", "C");
    TORCH_CHECK(HW > 0, "empty spatial extent");
    auto out = at::empty({NB, C}, x.options());
    if (f32)
        defer_hip::launch_gap_f32(f32ptr(x), out.data_ptr<float>(), NB, HW,
                                  C, cur_stream());
    else
        defer_hip::launch_gap(bptr(x), bptr_mut(out), NB, HW, C,
                              cur_stream());
    return out;
}

// Concat along the LAST (channel) dim of NHWC tensors: pure data
// movement. Two inputs whose channels are whole 16-byte vectors (the
// DenseNet shape class) take one vectorized kernel, which beats the
// per-input small-pitch 2D copies (measured); everything else is one
// strided device-to-device hipMemcpy2DAsync per input (row = one pixel's
// channels). No torch compute kernels in the path.
Tensor concat_lastdim(std::vector<Tensor> xs) {
    TORCH_CHECK(!xs.empty(), "concat of nothing");
    auto base = xs[0].sizes().vec();
    int nd = (int)base.size();
    long rows = 1;
    for (int i = 0; i + 1 < nd; ++i) rows *= base[i];
    long ctot = 0;
    const bool f32 = is_f32(xs[0], "concat input");
    for (auto& t : xs) {
        check_as(t, "concat input", f32, false);
        TORCH_CHECK((int)t.sizes().size() == nd, "rank mismatch");
        for (int i = 0; i + 1 < nd; ++i)
            TORCH_CHECK(t.size(i) == base[i], "leading-dim mismatch");
        ctot += t.size(nd - 1);
    }
    base[nd - 1] = ctot;
    auto out = at::empty(base, xs[0].options());
    hipStream_t s = cur_stream();
    const int vec = f32 ? 4 : 8;
    if (xs.size() == 2 && xs[0].size(nd - 1) % vec == 0 &&
        xs[1].size(nd - 1) % vec == 0) {
        const int c0 = (int)xs[0].size(nd - 1), c1 = (int)xs[1].size(nd - 1);
        if (f32)
            defer_hip::launch_cat2_f32(f32ptr(xs[0]), f32ptr(xs[1]),
                                       out.data_ptr<float>(), rows, c0, c1,
                                       s);
        else
            defer_hip::launch_cat2(bptr(xs[0]), bptr(xs[1]), bptr_mut(out),
                                   rows, c0, c1, s);
        return out;
    }
    const long esz = f32 ? 4 : 2;
    long coff = 0;
    for (auto& t : xs) {
        long cj = t.size(nd - 1);
        hipMemcpy2DAsync((char*)bptr_mut(out) + coff * esz, ctot * esz,
                         bptr(t), cj * esz, cj * esz, rows,
                         hipMemcpyDeviceToDevice, s);
        coff += cj;
    }
    return out;
}

// LayerNorm over the last dim (csrc/layernorm.hip): x of rank >= 2, weight
// and bias fp32[C]. max_blocks caps the grid (0 = policy).
Tensor layernorm_channels(Tensor x, Tensor weight, Tensor bias, double eps,
                          int64_t max_blocks) {
    const char* op = "layernorm_channels";
    TORCH_CHECK(x.dim() >= 2, "layernorm_channels: x must have rank >= 2");
    const bool f32 = check_channel_vec(x, op);
    const int64_t C = x.size(-1);
    TORCH_CHECK(C <= defer_hip::LAYERNORM_MAX_C,
                "layernorm_channels: needs C <= ", defer_hip::LAYERNORM_MAX_C,
                ", got C = ", C);
    TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0");
    const float* wt = f32_vec(weight, x, op, "weight", C, {false, true});
    const float* bi = f32_vec(bias, x, op, "bias", C, {false, true});
    auto out = at::empty_like(x);
    if (out.numel() == 0) return out;
    defer_hip::launch_layernorm(bptr(x), wt, bi, bptr_mut(out),
                                x.numel() / C, (int)C, (float)eps, f32,
                                (int)max_blocks, cur_stream());
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

}  // namespace

Tensor defer_bind::maxpool2d(Tensor x, int64_t kernel, int64_t stride,
                             int64_t pad) {
    return pool2d(x, kernel, stride, pad, "maxpool2d",
                  defer_hip::launch_maxpool, defer_hip::launch_maxpool_f32);
}

void bind_pointwise(py::module_& m) {
    m.def("bn_act", &bn_act);
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
    m.def("maxpool2d", &defer_bind::maxpool2d);
    m.def("avgpool2d", &avgpool2d);
    m.def("concat_lastdim", &concat_lastdim);
    m.def("global_avg_pool", &global_avg_pool);
    m.def("layernorm_channels", &layernorm_channels, py::arg("x"),
          py::arg("weight"), py::arg("bias"), py::arg("eps"),
          py::arg("max_blocks") = 0);
    m.def("layernorm_plan", [](int64_t C, bool f32) {
        const auto pl = defer_hip::layernorm_plan((int)C, f32 ? 4 : 8);
        return std::make_pair(pl.G, pl.VPL);
    }, py::arg("C"), py::arg("f32") = false);
    m.def("layout_convert", &layout_convert, py::arg("x"),
          py::arg("to_nhwc"), py::arg("bf16_out"),
          py::arg("out") = py::none());
}
