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
