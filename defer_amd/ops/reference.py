"""Pure-PyTorch fp32 reference implementations of every defer_amd op.

These are the ground truth that the HIP kernels are tested against
(numerics tests compare each gfx950 kernel to these at fp32), and the CPU
execution path for the plumbing config (BASELINE.json config 1 — the
reference's test/local_infer.py analogue).

All tensor ops use NHWC layout (the layout the HIP kernels use — NHWC makes
the implicit-GEMM K dimension (r, s, c) contiguous per (r, s) slice).
Weights for conv are [R, S, Cin, Cout] ("RSCK"); dense weights are
[Cin, Cout].
"""

from typing import Optional

import torch
import torch.nn.functional as F


# 1/6 rounded to fp32, the constant of the kernels (csrc/common.h)
_C6 = float(torch.tensor(1.0, dtype=torch.float32) / 6.0)


def _hardsigmoid_f32(v: torch.Tensor) -> torch.Tensor:
    """min(max(v + 3, 0), 6) * c6 of an fp32 tensor, in the kernels' order:
    6 * c6 and 3 * c6 round to exactly 1 and 0.5."""
    return torch.clamp(v + 3.0, 0.0, 6.0) * _C6


def _hardswish_f32(v: torch.Tensor) -> torch.Tensor:
    """v * hardsigmoid(v): v bit for bit for v >= 3, 0 for v <= -3. No
    division and no fma, unlike torch's own x * relu6(x + 3) / 6."""
    return v * _hardsigmoid_f32(v)


def apply_act(y: torch.Tensor, act: str,
              known=("none", "relu", "relu6", "hardswish")):
    """The activation `act` of the fp32 tensor `y`; a name outside `known`
    raises."""
    if act not in known:
        raise ValueError(f"act={act!r}: expected one of {list(known)}")
    if act == "relu":
        return torch.relu(y)
    if act == "relu6":
        return torch.clamp(y, 0.0, 6.0)
    if act == "hardswish":
        return _hardswish_f32(y)
    return y


_RELU_ONLY = ("none", "relu")


def conv2d_bn_act(
    x: torch.Tensor,            # [N, H, W, C]   activation
    w: torch.Tensor,            # [K, R, S, C]   weights (OHWI)
    scale: Optional[torch.Tensor],  # [K] folded BN scale (None -> 1)
    bias: Optional[torch.Tensor],   # [K] folded BN shift / conv bias
    stride: int = 1,
    padding: int = 0,
    act: str = "none",          # "none" | "relu" | "relu6" | "hardswish"
    residual: Optional[torch.Tensor] = None,  # [N, OH, OW, K] added pre-act
) -> torch.Tensor:
    """Fused conv + (folded) batchnorm + residual-add + activation.

    Mirrors what the reference gets from Keras Conv2D + BatchNormalization +
    Add + ReLU layers executed inside model.predict (node.py:106)."""
    xf = x.permute(0, 3, 1, 2).float()                 # NHWC -> NCHW
    wf = w.permute(0, 3, 1, 2).float()                 # OHWI -> OIHW
    y = F.conv2d(xf, wf, bias=None, stride=stride, padding=padding)
    if scale is not None:
        y = y * scale.float().view(1, -1, 1, 1)
    if bias is not None:
        y = y + bias.float().view(1, -1, 1, 1)
    y = y.permute(0, 2, 3, 1)                          # NCHW -> NHWC
    if residual is not None:
        y = y + residual.float()
    return apply_act(y, act).to(x.dtype)


def quantize_fp8(x, inv_scale):
    """e4m3(clamp(x * inv_scale, -448, 448)), round to nearest even. The
    clamp is the saturation: torch's cast alone gives NaN above 464."""
    return (x.float() * inv_scale).clamp(-448.0, 448.0).to(
        torch.float8_e4m3fn)


def conv2d_bn_act_fp8(x_q, w_q, scale, bias, stride, padding, act,
                      residual_q=None, res_scale=1.0, out_inv_scale=None):
    """The arithmetic of csrc/conv_fp8.hip in fp32 torch: dequantise the
    e4m3 bytes, conv, v = act(acc * scale + bias + res_scale * residual),
    then e4m3(clamp(v * out_inv_scale, +-448)) or, with out_inv_scale None,
    one bf16 rounding of v."""
    xf = x_q.float().permute(0, 3, 1, 2)
    wf = w_q.float().permute(0, 3, 1, 2)
    y = F.conv2d(xf, wf, bias=None, stride=stride, padding=padding)
    y = y * scale.float().view(1, -1, 1, 1) + bias.float().view(1, -1, 1, 1)
    y = y.permute(0, 2, 3, 1)
    if residual_q is not None:
        y = y + res_scale * residual_q.float()
    y = apply_act(y, act, known=("none", "relu", "relu6"))
    if out_inv_scale is None:
        return y.to(torch.bfloat16)
    return quantize_fp8(y, out_inv_scale)


def dwconv2d_bn_act(x, w, scale=None, bias=None, stride=1, padding=1,
                    act="none"):
    """Depthwise conv + (folded) batchnorm + activation: x [N, H, W, C],
    w [R, S, C], one filter per channel (F.conv2d with groups = C).

    y[n, oh, ow, c] = act(scale[c] * sum_{r,s} x[n, oh*stride - pad + r,
                          ow*stride - pad + s, c] * w[r, s, c] + bias[c])"""
    c = x.shape[-1]
    xf = x.permute(0, 3, 1, 2).float()                 # NHWC -> NCHW
    wf = w.permute(2, 0, 1).unsqueeze(1).float()       # RSC -> [C, 1, R, S]
    y = F.conv2d(xf, wf, bias=None, stride=stride, padding=padding, groups=c)
    if scale is not None:
        y = y * scale.float().view(1, -1, 1, 1)
    if bias is not None:
        y = y + bias.float().view(1, -1, 1, 1)
    return apply_act(y.permute(0, 2, 3, 1), act).to(x.dtype)


def gconv2d_bn_act(x, w, scale=None, bias=None, stride=1, padding=1,
                   act="none"):
    """Grouped conv + (folded) batchnorm + activation: x [N, H, W, C],
    w [K, R, S, Cg] with groups = C // Cg (F.conv2d with groups=); output
    channel k reads the input channels of group k // (K // groups)."""
    groups = x.shape[-1] // w.shape[-1]
    xf = x.permute(0, 3, 1, 2).float()                 # NHWC -> NCHW
    wf = w.permute(0, 3, 1, 2).float()                 # OHWI -> OIHW
    y = F.conv2d(xf, wf, bias=None, stride=stride, padding=padding,
                 groups=groups)
    if scale is not None:
        y = y * scale.float().view(1, -1, 1, 1)
    if bias is not None:
        y = y + bias.float().view(1, -1, 1, 1)
    return apply_act(y.permute(0, 2, 3, 1), act).to(x.dtype)


def dwconv7x7(x, w, bias=None):
    """7x7 depthwise conv, stride 1, padding 3: x [N, H, W, C], w [7, 7, C],
    bias fp32 [C] or None; no scale and no activation.

    y[n, oh, ow, c] = sum_{r,s} x[n, oh-3+r, ow-3+s, c] * w[r, s, c] + bias[c]"""
    c = x.shape[-1]
    xf = x.permute(0, 3, 1, 2).float()                 # NHWC -> NCHW
    wf = w.permute(2, 0, 1).unsqueeze(1).float()       # RSC -> [C, 1, R, S]
    y = F.conv2d(xf, wf, bias=None, stride=1, padding=3, groups=c)
    if bias is not None:
        y = y + bias.float().view(1, -1, 1, 1)
    return y.permute(0, 2, 3, 1).contiguous().to(x.dtype)


def layernorm_channels(x, weight, bias, eps=1e-6):
    """LayerNorm over the last dim, per leading index, in fp32 with the
    biased variance taken from the differences to the mean (two passes):

    y[..., c] = (x[..., c] - mean) / sqrt(var + eps) * weight[c] + bias[c]"""
    xf = x.float()
    d = xf - xf.mean(dim=-1, keepdim=True)
    var = (d * d).mean(dim=-1, keepdim=True)
    y = d * (1.0 / torch.sqrt(var + eps)) * weight.float() + bias.float()
    return y.to(x.dtype)


def _gelu_f32(v: torch.Tensor) -> torch.Tensor:
    """The exact (erf) GELU of an fp32 tensor, in the kernels' order."""
    return 0.5 * v * (1.0 + torch.erf(v * 0.70710678))


def linear_gelu(x, w, bias=None):
    """gelu(x @ w^T + bias): x [..., Cin], w [Cout, Cin]; the exact GELU in
    fp32 before the one rounding."""
    y = x.float() @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    return _gelu_f32(y).to(x.dtype)


def attention(qkv, heads):
    """Multi-head attention on a fused qkv [..., T, 3 * C] whose last dim is
    laid out [3][heads][D]: out[..., t, h*D + d] = sum_j P[h, t, j] *
    v[j, h, d] with P = softmax_j(q . k * D^-0.5). All of it in fp32, P
    included, one rounding to qkv's dtype."""
    t, c3 = qkv.shape[-2], qkv.shape[-1]
    d = c3 // (3 * heads)
    q, k, v = (qkv.float().reshape(-1, t, 3, heads, d)
               .permute(2, 0, 3, 1, 4))                 # each [N, heads, T, D]
    p = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1)
    out = (p @ v).permute(0, 2, 1, 3).reshape(*qkv.shape[:-1], c3 // 3)
    return out.to(qkv.dtype)


def _window_regions(size, window, shift):
    """The region 0, 1 or 2 of every shifted row (or column) of a map."""
    r = torch.arange(size)
    return (r >= size - window).long() + (r >= size - shift).long()


def window_attention(qkv, bias_table, heads, window, shift=0):
    """Swin's shifted-window attention on an NHWC qkv [N, H, W, 3 * C] whose
    last dim is [3][heads][32], as the plain composition: roll by -shift,
    partition into windows, q k^T * 32^-0.5 plus the index-gathered
    relative-position bias plus the -100 mask of the shifted regions,
    softmax, P v, reverse partition, roll back. All of it in fp32, P
    included, one rounding to qkv's dtype. This is the specification of
    ops.window_attention."""
    n, hh, ww, c3 = qkv.shape
    w, s, t, c = window, shift, window * window, c3 // 3
    d = c // heads
    x = torch.roll(qkv.float(), (-s, -s), (1, 2))
    x = (x.reshape(n, hh // w, w, ww // w, w, 3, heads, d)
         .permute(5, 0, 1, 3, 6, 2, 4, 7)
         .reshape(3, n, hh // w, ww // w, heads, t, d))
    q, k, v = x[0], x[1], x[2]                  # [N, nh, nw, heads, T, D]
    score = q @ k.transpose(-1, -2) * d ** -0.5
    ij = torch.stack(torch.meshgrid(torch.arange(w), torch.arange(w),
                                    indexing="ij")).reshape(2, t)
    rel = ij[:, :, None] - ij[:, None, :] + w - 1           # [2, T, T]
    index = rel[0] * (2 * w - 1) + rel[1]
    bias = bias_table.float()[index.reshape(-1)].reshape(t, t, heads)
    score = score + bias.permute(2, 0, 1).to(score.device)
    if s > 0:
        reg = (_window_regions(hh, w, s)[:, None] * 3
               + _window_regions(ww, w, s)[None, :])        # [H, W]
        reg = (reg.reshape(hh // w, w, ww // w, w).permute(0, 2, 1, 3)
               .reshape(hh // w, ww // w, t))
        apart = reg[:, :, :, None] != reg[:, :, None, :]    # [nh, nw, T, T]
        mask = torch.zeros(apart.shape).masked_fill(apart, -100.0)
        score = score + mask[:, :, None].to(score.device)
    out = torch.softmax(score, dim=-1) @ v                  # [N, nh, nw, h, T, D]
    out = (out.reshape(n, hh // w, ww // w, heads, w, w, d)
           .permute(0, 1, 4, 2, 5, 3, 6).reshape(n, hh, ww, c))
    return torch.roll(out, (s, s), (1, 2)).to(qkv.dtype)


def patch_merge(x):
    """NHWC [N, H, W, C] -> [N, H/2, W/2, 4C]: (even row, even col), (odd,
    even), (even, odd), (odd, odd) of every 2x2 patch, torchvision's order."""
    return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2],
                      x[:, 1::2, 1::2]], dim=-1).contiguous()


def embed_tokens(x, cls, pos):
    """NHWC x -> tokens [N, 1, 1 + H*W, C]: the class token cls (fp32 [C])
    in front of the H*W patch tokens, plus pos [1 + H*W, C]; fp32 sums, one
    rounding."""
    n, c = x.shape[0], x.shape[-1]
    tok = torch.cat([cls.float().expand(n, 1, c),
                     x.float().reshape(n, -1, c)], dim=1) + pos.float()
    return tok.unsqueeze(1).to(x.dtype)


def class_token(x):
    """[N, 1, T, C] -> [N, C]: token 0 of every image."""
    return x[:, 0, 0, :].contiguous()


def batchnorm_apply(x, scale, bias, act="none"):
    """Standalone inference batchnorm (y = x*scale + bias), NHWC.

    scale/bias are the folded gamma/sqrt(var+eps), beta - mean*scale."""
    y = x.float() * scale.float() + bias.float()
    return apply_act(y, act, _RELU_ONLY).to(x.dtype)


def add_act(a, b, act="relu"):
    """Residual add + activation (the reference's `add_N` layers +
    following ReLU — ResNet50 skip connections, test/test.py:18)."""
    y = a.float() + b.float()
    return apply_act(y, act, _RELU_ONLY).to(a.dtype)


def relu(x):
    return torch.relu(x)


def relu6(x):
    return torch.clamp(x, 0.0, 6.0)


def hardswish(x):
    """x * (min(max(x + 3, 0), 6) * c6) in fp32, one rounding to x's dtype."""
    return _hardswish_f32(x.float()).to(x.dtype)


def squeeze_excite(x, w1, b1, w2, b2, act="relu", gate="hardsigmoid"):
    """Squeeze-excite, x [N, H, W, C], w1 [Cr, C], w2 [C, Cr], biases [Cr]
    and [C] or None:

        s = mean over H, W of x          [N, C]
        z = act(w1 @ s + b1)             [N, Cr]
        g = gate(w2 @ z + b2)            [N, C]
        y = x * g

    s, z and g are fp32 and never rounded to x's dtype; y is rounded once."""
    if gate != "hardsigmoid":
        raise ValueError(f"gate={gate!r}: expected one of ['hardsigmoid']")
    xf = x.float()
    s = xf.mean(dim=(1, 2))
    z = s @ w1.float().t()
    if b1 is not None:
        z = z + b1.float()
    z = apply_act(z, act, _RELU_ONLY)
    v = z @ w2.float().t()
    if b2 is not None:
        v = v + b2.float()
    g = _hardsigmoid_f32(v)
    return (xf * g[:, None, None, :]).to(x.dtype)


def maxpool2d(x, kernel=3, stride=2, padding=1):
    """Max pooling, NHWC (ResNet50 stem)."""
    xf = x.permute(0, 3, 1, 2).float()
    y = F.max_pool2d(xf, kernel_size=kernel, stride=stride, padding=padding)
    return y.permute(0, 2, 3, 1).to(x.dtype)


def avgpool2d(x, kernel=2, stride=2, padding=0):
    """Average pooling, NHWC, valid taps only (count_include_pad=False;
    DenseNet transition layers)."""
    xf = x.permute(0, 3, 1, 2).float()
    y = F.avg_pool2d(xf, kernel_size=kernel, stride=stride,
                     padding=padding, count_include_pad=False)
    return y.permute(0, 2, 3, 1).to(x.dtype)


def concat_channels(xs):
    """Concat NHWC tensors on the channel dim (DenseNet)."""
    return torch.cat(list(xs), dim=-1)


def global_avg_pool(x):
    """[N, H, W, C] -> [N, C] (ResNet50 head)."""
    return x.float().mean(dim=(1, 2)).to(x.dtype)


def linear(x, w, bias=None):
    """[N, Cin] @ [Cout, Cin]^T + bias (classifier head)."""
    y = x.float() @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    return y.to(x.dtype)


def to_nhwc(x, dtype):
    """[N, C, H, W] -> [N, H, W, C] in `dtype` (fp32 -> bf16 rounds to
    nearest even, bf16 -> fp32 is exact)."""
    return x.permute(0, 2, 3, 1).contiguous().to(dtype)


def to_nchw(x, dtype):
    """[N, H, W, C] -> [N, C, H, W] in `dtype`; the inverse of to_nhwc."""
    return x.permute(0, 3, 1, 2).contiguous().to(dtype)


def softmax(x):
    """Row softmax over the last dim (classifier head)."""
    return F.softmax(x.float(), dim=-1).to(x.dtype)
