// Torch entry points of the transformer ops: fused and shifted-window
// attention (attention.hip, window_attention.hip) with their plan queries,
// and the token shuffles around them (elementwise.hip, ops_f32.hip).
#include "entry_util.h"

namespace {

using namespace defer_bind;

// Fused multi-head attention: qkv [..., T, 3 * C] with the last dim laid out
// [3][heads][64], out [..., T, C].
Tensor attention(Tensor qkv, int64_t heads) {
    TORCH_CHECK(qkv.is_cuda(), "attention: qkv must be on GPU");
    TORCH_CHECK(qkv.scalar_type() == at::kBFloat16 ||
                qkv.scalar_type() == at::kFloat,
                "attention: qkv must be bf16 or fp32, got ",
                qkv.scalar_type());
    TORCH_CHECK(qkv.dim() >= 3,
                "attention: qkv must be [..., T, 3 * C] with rank >= 3, got ",
                qkv.dim(), "-D");
    TORCH_CHECK(qkv.is_contiguous(), "attention: qkv must be contiguous");
    TORCH_CHECK(aligned16(qkv), "attention: qkv must be 16-byte aligned");
    const int64_t C3 = qkv.size(-1), T = qkv.size(-2);
    TORCH_CHECK(heads >= 1 && C3 > 0 && C3 % (3 * heads) == 0,
                "attention: the last dim must be 3 * heads * D, got ", C3,
                " for heads = ", heads);
    TORCH_CHECK(C3 / (3 * heads) == 64,
                "attention: needs D == 64 (head dim), got D = ",
                C3 / (3 * heads));
    TORCH_CHECK(T >= 1, "attention: needs T >= 1, got T = ", T);
    TORCH_CHECK(qkv.numel() < (1LL << 31),
                "attention: qkv has 2^31 or more elements");
    auto shape = qkv.sizes().vec();
    shape.back() = C3 / 3;
    auto out = at::empty(shape, qkv.options());
    if (out.numel() == 0) return out;
    defer_hip::launch_attention(bptr(qkv), bptr_mut(out),
                                (int)(qkv.numel() / (T * C3)), (int)T,
                                (int)heads,
                                qkv.scalar_type() == at::kFloat,
                                cur_stream());
    return out;
}

// The bf16 attention kernel's work split for T tokens. Needs no GPU.
py::dict attention_plan(int64_t T) {
    using namespace pybind11::literals;
    TORCH_CHECK(T >= 1 && T < (1LL << 31), "attention: needs T >= 1");
    const auto a = defer_hip::attention_geom((int)T);
    return py::dict("groups"_a = a.G, "groups_per_wave"_a = a.NQ,
                    "blocks"_a = a.nblk, "groups_per_block"_a = a.gpb,
                    "lds_bytes"_a = a.lds_bytes);
}

// Shifted-window attention: qkv NHWC [N, H, W, 3 * C] with the last dim laid
// out [3][heads][32], table [(2w - 1)^2, heads] in qkv's dtype, out [N, H, W,
// C].
Tensor window_attention(Tensor qkv, Tensor table, int64_t heads,
                        int64_t window, int64_t shift) {
    TORCH_CHECK(qkv.is_cuda(), "window_attention: qkv must be on GPU");
    TORCH_CHECK(qkv.scalar_type() == at::kBFloat16 ||
                qkv.scalar_type() == at::kFloat,
                "window_attention: qkv must be bf16 or fp32, got ",
                qkv.scalar_type());
    TORCH_CHECK(qkv.dim() == 4,
                "window_attention: qkv must be NHWC (4-D), got ", qkv.dim(),
                "-D");
    TORCH_CHECK(qkv.is_contiguous(),
                "window_attention: qkv must be contiguous");
    TORCH_CHECK(aligned16(qkv),
                "window_attention: qkv must be 16-byte aligned");
    const int64_t N = qkv.size(0), H = qkv.size(1), W = qkv.size(2),
                  C3 = qkv.size(3);
    TORCH_CHECK(heads >= 1 && C3 == 3 * heads * 32,
                "window_attention: the last dim must be 3 * heads * 32, got ",
                C3, " for heads = ", heads);
    TORCH_CHECK(window >= 2 && window * window <= 64,
                "window_attention: needs 2 <= window and window^2 <= 64, got "
                "window = ", window);
    TORCH_CHECK(H > 0 && W > 0 && H % window == 0 && W % window == 0,
                "window_attention: window must divide H and W, got ", H, "x",
                W, " for window = ", window);
    TORCH_CHECK(shift >= 0 && shift < window,
                "window_attention: needs 0 <= shift < window, got shift = ",
                shift);
    const int64_t nb = (2 * window - 1) * (2 * window - 1);
    TORCH_CHECK(table.is_cuda() && table.scalar_type() == qkv.scalar_type() &&
                table.is_contiguous() && table.dim() == 2 &&
                table.size(0) == nb && table.size(1) == heads,
                "window_attention: bias_table must be a contiguous GPU "
                "[(2*window - 1)^2, heads] = [", nb, ", ", heads,
                "] of qkv's dtype (mixed dtypes)");
    TORCH_CHECK(qkv.numel() < (1LL << 31),
                "window_attention: qkv has 2^31 or more elements");
    auto out = at::empty({N, H, W, C3 / 3}, qkv.options());
    if (out.numel() == 0) return out;
    defer_hip::launch_window_attention(
        bptr(qkv), bptr(table), bptr_mut(out), (int)N, (int)H, (int)W,
        (int)heads, (int)window, (int)shift, qkv.scalar_type() == at::kFloat,
        cur_stream());
    return out;
}

// The bf16 window attention kernel's work split. Needs no GPU.
py::dict window_attention_plan(int64_t N, int64_t H, int64_t W, int64_t heads,
                               int64_t window) {
    using namespace pybind11::literals;
    TORCH_CHECK(N >= 0 && heads >= 1 && window >= 2 && window * window <= 64 &&
                H > 0 && W > 0 && H % window == 0 && W % window == 0 &&
                N * H * W * heads * 96 < (1LL << 31),
                "window_attention: no kernel for this shape");
    const auto g = defer_hip::window_attention_geom((int)N, (int)H, (int)W,
                                                    (int)heads, (int)window);
    return py::dict("tokens"_a = g.T, "groups"_a = g.groups,
                    "windows"_a = g.windows, "pairs"_a = g.pairs,
                    "blocks"_a = g.blocks, "idle_waves"_a = g.idle_waves,
                    "lds_bytes"_a = g.lds_bytes);
}

// Swin's patch merging gather: NHWC [N, H, W, C] -> [N, H/2, W/2, 4C], the
// four pixels of a 2x2 patch in torchvision's order. A copy.
Tensor patch_merge(Tensor x) {
    TORCH_CHECK(x.dim() == 4, "patch_merge: x must be NHWC");
    const bool f32 = check_channel_vec(x, "patch_merge");
    const int64_t N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
    TORCH_CHECK(H % 2 == 0 && W % 2 == 0,
                "patch_merge: H and W must be even, got ", H, "x", W);
    TORCH_CHECK(H < (1LL << 31) && W < (1LL << 31),
                "patch_merge: H and W must be below 2^31");
    auto out = at::empty({N, H / 2, W / 2, 4 * C}, x.options());
    if (out.numel() == 0) return out;
    if (f32)
        defer_hip::launch_patch_merge_f32(f32ptr(x), out.data_ptr<float>(), N,
                                          (int)H, (int)W, (int)C,
                                          cur_stream());
    else
        defer_hip::launch_patch_merge(bptr(x), bptr_mut(out), N, (int)H,
                                      (int)W, (int)C, cur_stream());
    return out;
}

// y[n, 0, 0] = cls + pos[0], y[n, 0, 1 + t] = x[n, t] + pos[1 + t]: x NHWC,
// cls fp32 [C], pos [1 + H*W, C] in x's dtype, y [N, 1, 1 + H*W, C].
Tensor embed_tokens(Tensor x, Tensor cls, Tensor pos) {
    TORCH_CHECK(x.dim() == 4, "embed_tokens: x must be NHWC");
    const bool f32 = check_channel_vec(x, "embed_tokens");
    const int64_t N = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
    const float* cl = f32_vec(cls, x, "embed_tokens", "cls", C,
                              {false, true});
    TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == x.scalar_type() &&
                pos.is_contiguous() && aligned16(pos) &&
                pos.dim() == 2 && pos.size(0) == HW + 1 && pos.size(1) == C,
                "embed_tokens: pos must be a contiguous GPU [1 + H*W, C] of "
                "x's dtype (mixed dtypes) with 1 + H*W = ", HW + 1,
                " and C = ", C);
    auto out = at::empty({N, 1, HW + 1, C}, x.options());
    if (out.numel() == 0) return out;
    if (f32)
        defer_hip::launch_embed_tokens_f32(f32ptr(x), cl, f32ptr(pos),
                                           out.data_ptr<float>(), N, HW,
                                           (int)C, cur_stream());
    else
        defer_hip::launch_embed_tokens(bptr(x), cl, bptr(pos), bptr_mut(out),
                                       N, HW, (int)C, cur_stream());
    return out;
}

// [N, 1, T, C] -> [N, C], token 0 of every image: one strided device copy
// (a memcpy node when a hipGraph is being captured), no compute kernel.
Tensor class_token(Tensor x) {
    TORCH_CHECK(x.is_cuda(), "class_token: x must be on GPU");
    is_f32(x, "class_token: x");
    TORCH_CHECK(x.dim() == 4 && x.size(1) == 1 && x.size(2) >= 1,
                "class_token: x must be [N, 1, T, C] with T >= 1");
    TORCH_CHECK(x.is_contiguous(), "class_token: x must be contiguous");
    const int64_t N = x.size(0), T = x.size(2), C = x.size(3);
    auto out = at::empty({N, C}, x.options());
    if (out.numel() == 0) return out;
    const size_t row = (size_t)C * x.element_size();
    hipMemcpy2DAsync(bptr_mut(out), row, bptr(x), (size_t)T * row, row,
                     (size_t)N, hipMemcpyDeviceToDevice, cur_stream());
    return out;
}

}  // namespace

void bind_attention(py::module_& m) {
    m.def("attention", &attention, py::arg("qkv"), py::arg("heads"));
    m.def("attention_plan", &attention_plan, py::arg("T"));
    m.def("window_attention", &window_attention, py::arg("qkv"),
          py::arg("bias_table"), py::arg("heads"), py::arg("window"),
          py::arg("shift"));
    m.def("window_attention_plan", &window_attention_plan, py::arg("N"),
          py::arg("H"), py::arg("W"), py::arg("heads"), py::arg("window"));
    m.def("patch_merge", &patch_merge, py::arg("x"));
    m.def("embed_tokens", &embed_tokens, py::arg("x"), py::arg("cls"),
          py::arg("pos"));
    m.def("class_token", &class_token);
}
