"""defer_amd.ops — functional op API with gfx950 HIP backend.

On a GPU device every op dispatches to the hand-written CDNA4 kernels in
`defer_amd/csrc` (built in-tree as `defer_amd._hip_ops`). If a tensor is on
a CUDA device and the extension is not importable, ops raise — there is no
silent eager fallback on GPU (the HIP path is the product; the reference's
equivalent substrate was TensorFlow's native kernels, node.py:106).

GPU tensors may be bf16 (the tuned default) or fp32 (the exact-f32 MFMA
path, `csrc/conv_f32.hip` + `csrc/ops_f32.hip`); the bindings pick the
launcher from the tensor's dtype and raise for anything else. The fused
ops (`conv1x1_prebn`, `conv1x1_chain`, `conv1x1_chain_proj`,
`conv_bn_act_maxpool`) have no fp32 kernel: for fp32 GPU tensors they compose the primitive ops of this module,
which is the same arithmetic the CPU branch runs.

On CPU, ops use the fp32 PyTorch reference implementations (tests and the
no-GPU plumbing config).
"""

import os
from typing import Optional

import torch

from defer_amd.ops import reference as _ref

_hip = None
_hip_err: Optional[Exception] = None


def _load_hip():
    global _hip, _hip_err
    if _hip is not None or _hip_err is not None:
        return _hip
    try:
        import defer_amd._hip_ops as m  # built by build_ext / build.py

        _hip = m
    except Exception as e:  # pragma: no cover - exercised only sans build
        _hip_err = e
    return _hip


def hip_available() -> bool:
    return _load_hip() is not None


def _backend(x: torch.Tensor):
    if x.is_cuda:
        m = _load_hip()
        if m is None:
            raise RuntimeError(
                "defer_amd HIP extension (defer_amd._hip_ops) is not built "
                "but a GPU tensor was passed. Build it with "
                "`python -m defer_amd.build` (gfx950). Import error: "
                f"{_hip_err!r}"
            )
        return m
    return None


_MODES = {None: 0, "": 0, "force": 1, "0": 2}


def _env_mode(name):
    """The 0/1/2 mode that the A/B switch `name` asks for (read at import)."""
    value = os.environ.get(name)
    if value not in _MODES:
        raise ValueError(
            f"{name}={value!r}: expected unset, '0' or 'force'")
    return _MODES[value]


def _built():
    m = _load_hip()
    if m is None:
        raise RuntimeError(
            f"defer_amd HIP extension is not built: {_hip_err!r}")
    return m


def _stats(name):
    return dict(getattr(_built(), name)())


# activation names -> the codes of the bindings (ACT_* of csrc/common.h)
_ACT_CODES = {"none": 0, "relu": 1, "relu6": 2, "hardswish": 3}
_RELU_OR_NONE = ("relu", "none")
_SE_GATES = ("hardsigmoid",)


def _act_code(act, known=tuple(_ACT_CODES), what="act"):
    """The binding's code of activation `act`. Every op checks its act
    through this on every device, so a name the op does not implement
    raises instead of silently meaning "none"."""
    if act not in known:
        raise ValueError(f"{what}={act!r}: expected one of {list(known)}")
    return _ACT_CODES[act]


# A/B switch for the weight-stationary 3x3 kernel (same convention as
# DEFER_CONV_CHAIN): unset = the launcher's measured policy, "0" = always
# the older conv paths, "force" = the new kernel wherever it covers the
# shape.
_CONV_WS_MODE = _env_mode("DEFER_CONV_WS")


def conv2d_bn_act(x, w, scale=None, bias=None, stride=1, padding=1,
                  act="none", residual=None, mode=None, max_blocks=0):
    """act(conv2d(x, w) * scale + bias + residual), NHWC x and OHWI w.

    On GPU, bf16 3x3/s1/p1 convs with 64 -> 64 channels can run the
    weight-stationary window kernel (csrc/conv_ws.hip), whose output is
    bit-identical to the general paths. mode: 0 = policy, 1 = that kernel
    wherever it covers the shape, 2 = never; None = DEFER_CONV_WS. Every
    other shape or dtype runs the general paths under every mode.
    max_blocks caps that kernel's grid (0 = policy). act: "none", "relu",
    "relu6" (min(max(v, 0), 6)) or "hardswish" (v * (min(max(v + 3, 0), 6)
    * (1/6)), see hardswish), applied after scale, bias and residual and
    before the one rounding to the output dtype."""
    code = _act_code(act)
    m = _backend(x)
    if m is None:
        return _ref.conv2d_bn_act(x, w, scale, bias, stride, padding, act,
                                  residual)
    return m.conv2d_bn_act(x, w, scale, bias, residual, stride, padding,
                           code,
                           _CONV_WS_MODE if mode is None else mode,
                           max_blocks)


def dwconv2d_bn_act(x, w, scale=None, bias=None, stride=1, padding=1,
                    act="none"):
    """Depthwise conv + folded BN + activation, NHWC x and [R, S, C] w:

        y[n, oh, ow, c] = act(scale[c] * sum_{r,s} x[n, oh*stride - pad + r,
                              ow*stride - pad + s, c] * w[r, s, c] + bias[c])

    scale and bias are fp32 [C] (None = 1 / 0); act as in conv2d_bn_act. On
    the GPU one HIP kernel (csrc/dwconv.hip) for R == S in {3, 5}, stride
    in {1, 2}, 0 <= padding <= R // 2 and C % 8 == 0 (bf16) or C % 4 == 0
    (fp32); any other geometry raises. fp32 accumulation in the fixed tap
    order (r, then s), one rounding at the end, run-to-run identical."""
    code = _act_code(act)
    m = _backend(x)
    if m is None:
        return _ref.dwconv2d_bn_act(x, w, scale, bias, stride, padding, act)
    return m.dwconv2d_bn_act(x, w, scale, bias, stride, padding, code)


def conv_plan(x_shape, w_shape, stride=1, padding=1, residual=False,
              mode=None, max_blocks=0, variant=None):
    """What conv2d_bn_act (NHWC / OHWI shapes) or linear (2-D shapes) would
    launch on the GPU for bf16 tensors of these shapes, without launching
    it: {"path", "family", the tile config or window height, "grid_x",
    "grid_y", "template_args", ...}. Needs the built extension but no GPU.
    mode as in conv2d_bn_act; variant: a DEFER_CONV_VARIANT value, None =
    the environment's."""
    return dict(_built().conv_plan(
        list(x_shape), list(w_shape), stride, padding, bool(residual),
        _CONV_WS_MODE if mode is None else mode, max_blocks, variant))


def conv_ws_stats():
    """What the weight-stationary 3x3 path of conv2d_bn_act did in this
    process: {"launches": kernel launches so far, "blocks",
    "tiles_per_block": the grid of the last one}. Lets tests tell the new
    kernel from the older paths, whose results are identical by design."""
    return _stats("conv_ws_stats")


def conv1x1_prebn(x, w, scale, bias, out_scale=None, out_bias=None):
    """Fused relu(x*scale+bias) @ w for 1x1/s1/p0 convs (DenseNet
    BNActConv), optionally followed by the NEXT layer's folded BN-ReLU
    on the output accumulator (out_scale/out_bias): saves the
    standalone bn_act round-trips on GPU; CPU composes the reference
    ops."""
    m = _backend(x)
    if m is None:
        z = _ref.batchnorm_apply(x, scale, bias, "relu")
        y = _ref.conv2d_bn_act(z, w, None, None, 1, 0, "none", None)
        if out_scale is not None:
            y = _ref.batchnorm_apply(y, out_scale, out_bias, "relu")
        return y
    if x.dtype == torch.float32:
        z = batchnorm_apply(x, scale, bias, "relu")
        y = conv2d_bn_act(z, w, None, None, 1, 0, "none", None)
        if out_scale is not None:
            y = batchnorm_apply(y, out_scale, out_bias, "relu")
        return y
    return m.conv1x1_prebn(x, w, scale, bias, out_scale, out_bias)


# A/B switch for the chained expand->reduce kernel (mirrors
# DEFER_CONV_VARIANT): unset = the launcher's measured policy, "0" = always
# two launches, "force" = fused wherever an instantiation exists.
_CHAIN_MODE = _env_mode("DEFER_CONV_CHAIN")

# A/B switch for the 128-row tile of the chain kernel (same convention):
# unset = the launcher's measured policy, "0" = never, "force" = wherever a
# class has that form. As the bm argument of conv1x1_chain: 0, 64, 128.
def _env_chain_bm():
    return {0: 0, 1: 128, 2: 64}[_env_mode("DEFER_CHAIN_BM128")]


_CHAIN_BM = _env_chain_bm()


def conv1x1_chain(x, w3, s3, b3, residual, act3, w1, s1, b1, act1,
                  mode=None, max_blocks=0, bm=None):
    """Bottleneck boundary pair in one call:

        y  = act3(conv1x1(x, w3)*s3 + b3 + residual)
        a2 = act1(conv1x1(y, w1)*s1 + b1)

    Returns (y, a2), identical to two conv2d_bn_act calls. On GPU the
    chain kernel (csrc/chain.hip) keeps each y tile in LDS for the second
    GEMM, so y is written once and never read back. mode: 0 = policy,
    1 = fused wherever legal, 2 = two launches; None = DEFER_CONV_CHAIN.
    bm: rows of a fused tile, 0 = the launcher's measured policy, 64, or 128
    (only the 256-channel x, 256-channel a2 class has a 128-row form; every
    other class runs 64 rows whatever bm says); None = DEFER_CHAIN_BM128.
    act3 and act1 are "relu" or "none"."""
    _act_code(act3, _RELU_OR_NONE, "act3")
    _act_code(act1, _RELU_OR_NONE, "act1")
    if bm is None:
        bm = _CHAIN_BM
    if bm not in (0, 64, 128):
        raise ValueError(f"bm={bm!r}: expected 0, 64 or 128")
    m = _backend(x)
    if m is None:
        y = _ref.conv2d_bn_act(x, w3, s3, b3, 1, 0, act3, residual)
        a2 = _ref.conv2d_bn_act(y, w1, s1, b1, 1, 0, act1, None)
        return y, a2
    if x.dtype == torch.float32:
        y = conv2d_bn_act(x, w3, s3, b3, 1, 0, act3, residual)
        a2 = conv2d_bn_act(y, w1, s1, b1, 1, 0, act1, None)
        return y, a2
    return m.conv1x1_chain(x, w3, s3, b3, residual, act3 == "relu", w1, s1,
                           b1, act1 == "relu",
                           _CHAIN_MODE if mode is None else mode, max_blocks,
                           bm)


def conv1x1_chain_stats():
    """What the fused kernel of conv1x1_chain did in this process:
    {"launches": its launches so far, "blocks", "bm": the grid and the rows
    per tile of the last one}. Lets tests tell the 64-row and the 128-row
    form apart, whose results are identical by design."""
    return _stats("conv1x1_chain_stats")


# A/B switch for the chain kernel that makes the projection shortcut itself
# (same convention as DEFER_CONV_CHAIN): unset = the launcher's measured
# policy, "0" = always the projection launch plus conv1x1_chain, "force" =
# the kernel wherever it serves the shape.
_CHAIN_PROJ_MODE = _env_mode("DEFER_CHAIN_PROJ")


def conv1x1_chain_proj(x, w3, s3, b3, xp, wp, sp, bp, act3, w1, s1, b1,
                       act1, mode=None, max_blocks=0):
    """conv1x1_chain whose residual is a 1x1/s1 projection of xp (the
    first bottleneck of a ResNet stage with stride 1):

        res = conv1x1(xp, wp)*sp + bp
        y   = act3(conv1x1(x, w3)*s3 + b3 + res)
        a2  = act1(conv1x1(y, w1)*s1 + b1)

    Returns (y, a2), identical to conv2d_bn_act for res followed by
    conv1x1_chain. On GPU, for 64-channel x and xp and a 64-channel a2, one
    kernel (csrc/chain.hip, PROJ) makes res per tile in registers, so res is
    neither written nor read back. Every other shape, fp32 and the CPU
    compose the two ops. mode: 0 = policy, 1 = the kernel wherever it serves
    the shape, 2 = never; None = DEFER_CHAIN_PROJ. act3 and act1 are "relu"
    or "none"."""
    _act_code(act3, _RELU_OR_NONE, "act3")
    _act_code(act1, _RELU_OR_NONE, "act1")
    if mode is None:
        mode = _CHAIN_PROJ_MODE
    if mode not in (0, 1, 2):
        raise ValueError(f"mode={mode!r}: expected 0, 1 or 2")
    if x.is_cuda and x.dtype == torch.bfloat16 and mode != 2:
        out = _backend(x).conv1x1_chain_proj(
            x, w3, s3, b3, xp, wp, sp, bp, act3 == "relu", w1, s1, b1,
            act1 == "relu", mode, max_blocks)
        if out is not None:
            return out
    res = conv2d_bn_act(xp, wp, sp, bp, 1, 0, "none")
    return conv1x1_chain(x, w3, s3, b3, res, act3, w1, s1, b1, act1)


def chain_proj_stats():
    """What conv1x1_chain_proj did in this process: {"launches": launches
    of the projected-residual kernel so far, "blocks": the grid of the last
    one}. Lets tests tell that kernel from the composed ops, whose results
    are identical by design."""
    return _stats("chain_proj_stats")


# A/B switch for the fused stem conv + max-pool kernel (same convention as
# DEFER_CONV_CHAIN): unset = the binding's policy, "0" = always two
# launches, "force" = fused wherever the kernel covers the shape.
_STEM_POOL_MODE = _env_mode("DEFER_STEM_POOL")


def conv_bn_act_maxpool(x, w, scale, bias, stride, padding, act,
                        pool_kernel, pool_stride, pool_padding, mode=None,
                        max_blocks=0):
    """maxpool2d(conv2d_bn_act(x, w, scale, bias, act=act)) in one call,
    identical to the two ops it replaces. On GPU the 7x7/s2 Cin=3 Cout=64
    ReLU stem followed by a 3x3/s2/p1 pool runs as one kernel
    (csrc/stem_pool.hip) that never writes the conv activation; every other
    geometry runs the two launches. mode: 0 = policy, 1 = fused wherever
    legal, 2 = two launches; None = DEFER_STEM_POOL. act is "relu" or
    "none"."""
    _act_code(act, _RELU_OR_NONE)
    m = _backend(x)
    if m is None:
        y = _ref.conv2d_bn_act(x, w, scale, bias, stride, padding, act, None)
        return _ref.maxpool2d(y, pool_kernel, pool_stride, pool_padding)
    if x.dtype == torch.float32:
        y = conv2d_bn_act(x, w, scale, bias, stride, padding, act, None)
        return maxpool2d(y, pool_kernel, pool_stride, pool_padding)
    return m.conv_bn_act_maxpool(x, w, scale, bias, stride, padding,
                                 act == "relu", pool_kernel, pool_stride,
                                 pool_padding,
                                 _STEM_POOL_MODE if mode is None else mode,
                                 max_blocks)


def stem_pool_stats():
    """What the fused stem path of conv_bn_act_maxpool did in this process:
    {"launches": fused-kernel launches so far, "bands", "rows_per_band":
    the band split of the last one}. Lets tests tell the fused kernel from
    the two launches, whose results are identical by design."""
    return _stats("stem_pool_stats")


# The CPU branch of an op raises what the bindings raise for the same call,
# so a model that runs on the CPU cannot fail on these later on the GPU.

def _check_pool(name, x, kernel, stride, padding):
    if x.dim() != 4:
        raise RuntimeError(f"{name}: x must be NHWC, got {x.dim()}-D")
    if kernel < 1:
        raise RuntimeError(f"{name}: kernel must be >= 1, got {kernel}")
    if stride < 1:
        raise RuntimeError(f"{name}: stride must be >= 1, got {stride}")
    if not 0 <= padding <= kernel // 2:
        raise RuntimeError(
            f"{name}: pad must be in [0, kernel / 2], got pad {padding} "
            f"for kernel {kernel}")
    h, w = x.shape[1], x.shape[2]
    if h + 2 * padding < kernel or w + 2 * padding < kernel:
        raise RuntimeError(
            f"{name}: input {h}x{w} with pad {padding} is smaller than the "
            f"window {kernel}")


def batchnorm_apply(x, scale, bias, act="none"):
    _act_code(act, _RELU_OR_NONE)
    m = _backend(x)
    if m is None:
        c = x.shape[-1] if x.dim() else 0
        if (scale.device != x.device or bias.device != x.device
                or scale.numel() != c or bias.numel() != c):
            raise RuntimeError(
                "batchnorm_apply: scale/bias must be tensors of length C "
                "on x's device")
        return _ref.batchnorm_apply(x, scale, bias, act)
    return m.bn_act(x, scale, bias, act == "relu")


def add_act(a, b, act="relu"):
    _act_code(act, _RELU_OR_NONE)
    m = _backend(a)
    if m is None:
        return _ref.add_act(a, b, act)
    return m.add_act(a, b, act == "relu")


def relu(x):
    m = _backend(x)
    if m is None:
        return _ref.relu(x)
    return m.relu(x)


def relu6(x):
    """min(max(x, 0), 6), with relu's numel rules on the GPU."""
    m = _backend(x)
    if m is None:
        return _ref.relu6(x)
    return m.relu6(x)


def hardswish(x):
    """x * hardsigmoid(x) with hardsigmoid(v) = min(max(v + 3, 0), 6) * c6,
    c6 = 1/6 in fp32, evaluated in fp32 in exactly this order with one
    rounding to x's dtype: x for x >= 3 and 0 for x <= -3, bit for bit.
    relu's numel rules on the GPU."""
    m = _backend(x)
    if m is None:
        return _ref.hardswish(x)
    return m.hardswish(x)


def _check_squeeze_excite(x, w1, b1, w2, b2):
    """What the binding refuses, for the CPU branch."""
    if x.dim() != 4:
        raise RuntimeError(
            f"squeeze_excite: x must be NHWC, got {x.dim()}-D")
    if w1.dtype != x.dtype or w2.dtype != x.dtype:
        raise RuntimeError(
            f"squeeze_excite: w1 and w2 must be {x.dtype} like x (mixed "
            f"dtypes), got {w1.dtype} and {w2.dtype}")
    if not (x.is_contiguous() and w1.is_contiguous()
            and w2.is_contiguous()):
        raise RuntimeError("squeeze_excite: x, w1 and w2 must be contiguous")
    c = x.shape[3]
    if w1.dim() != 2 or w1.shape[1] != c or w1.shape[0] < 1:
        raise RuntimeError(
            f"squeeze_excite: w1 must be [Cr, C] with C = {c}")
    cr = w1.shape[0]
    if w2.dim() != 2 or tuple(w2.shape) != (c, cr):
        raise RuntimeError(
            f"squeeze_excite: w2 must be [C, Cr] = [{c}, {cr}]")
    for name, b, n in (("b1", b1, cr), ("b2", b2, c)):
        if b is not None and (b.device != x.device
                              or b.dtype != torch.float32
                              or not b.is_contiguous()
                              or tuple(b.shape) != (n,)):
            raise RuntimeError(
                f"squeeze_excite: {name} must be a contiguous fp32[{n}] on "
                "x's device")
    if x.shape[1] * x.shape[2] == 0:
        raise RuntimeError("squeeze_excite: empty spatial extent")


def squeeze_excite(x, w1, b1, w2, b2, act="relu", gate="hardsigmoid"):
    """Squeeze-excite of an NHWC x with w1 [Cr, C] and w2 [C, Cr] in x's
    dtype (bf16 or fp32) and fp32 biases b1 [Cr], b2 [C] (or None):

        s = mean over H, W of x                  (fp32, [N, C])
        z = act(w1 @ s + b1)                     (fp32, [N, Cr])
        g = gate(w2 @ z + b2)                    (fp32, [N, C])
        y = round_to_dtype(x * g)

    act is "relu" or "none", gate is "hardsigmoid" (see hardswish). s, z and
    g are never rounded to bf16. On the GPU two HIP launches (csrc/se.hip):
    the gate, one workgroup per image, and the scale pass; no atomics, every
    sum in a fixed order, run-to-run identical. C % 8 == 0 (bf16) or
    C % 4 == 0 (fp32), any Cr >= 1; N == 0 gives an empty tensor."""
    code = _act_code(act, _RELU_OR_NONE)
    if gate not in _SE_GATES:
        raise ValueError(
            f"gate={gate!r}: expected one of {list(_SE_GATES)}")
    m = _backend(x)
    if m is None:
        _check_squeeze_excite(x, w1, b1, w2, b2)
        return _ref.squeeze_excite(x, w1, b1, w2, b2, act, gate)
    return m.squeeze_excite(x, w1, b1, w2, b2, code)


def se_gate(x, w1, b1, w2, b2, act="relu"):
    """The fp32 [N, C] gate g of squeeze_excite, and channel_scale(x, g) its
    second pass: the two launches apart, for tools/sebench.py. GPU only."""
    code = _act_code(act, _RELU_OR_NONE)
    return _gpu_only(x, "se_gate").se_gate(x, w1, b1, w2, b2, code)


def channel_scale(x, g):
    """round_to_dtype(x * g[n, c]) for NHWC x and fp32 g [N, C]. GPU only."""
    return _gpu_only(x, "channel_scale").channel_scale(x, g)


def _gpu_only(x, name):
    m = _backend(x)
    if m is None:
        raise RuntimeError(f"{name}: GPU tensors only")
    return m


def maxpool2d(x, kernel=3, stride=2, padding=1):
    """Max over the window's in-bounds taps, NHWC (a window of -inf gives
    -inf). Raises for kernel < 1, stride < 1, padding outside
    [0, kernel // 2] and an input smaller than the window, like
    F.max_pool2d; avgpool2d likewise."""
    m = _backend(x)
    if m is None:
        _check_pool("maxpool2d", x, kernel, stride, padding)
        return _ref.maxpool2d(x, kernel, stride, padding)
    return m.maxpool2d(x, kernel, stride, padding)


def avgpool2d(x, kernel=2, stride=2, padding=0):
    m = _backend(x)
    if m is None:
        _check_pool("avgpool2d", x, kernel, stride, padding)
        return _ref.avgpool2d(x, kernel, stride, padding)
    return m.avgpool2d(x, kernel, stride, padding)


def concat_channels(xs):
    """Concat NHWC tensors on the channel (last) dim — DenseNet's dense
    connections. GPU: one strided device copy per input (no torch
    compute kernels)."""
    m = _backend(xs[0])
    if m is None:
        return _ref.concat_channels(xs)
    return m.concat_lastdim(list(xs))


def global_avg_pool(x):
    m = _backend(x)
    if m is None:
        if x.dim() != 4:
            raise RuntimeError(
                f"global_avg_pool: x must be NHWC, got {x.dim()}-D")
        if x.shape[1] * x.shape[2] == 0:
            raise RuntimeError("global_avg_pool: empty spatial extent")
        return _ref.global_avg_pool(x)
    return m.global_avg_pool(x)


_LAYOUT_DTYPES = (torch.float32, torch.bfloat16)


def _layout_convert(x, dtype, out, to_nhwc):
    name = "to_nhwc" if to_nhwc else "to_nchw"
    dtype = x.dtype if dtype is None else dtype
    # the same rejections on every device, so a model that lowers on the
    # CPU cannot fail on these later on the GPU
    if x.dtype not in _LAYOUT_DTYPES or dtype not in _LAYOUT_DTYPES:
        raise RuntimeError(
            f"{name}: x and dtype must be bf16 or fp32, got {x.dtype} -> "
            f"{dtype}")
    if x.dim() != 4:
        raise RuntimeError(f"{name}: x must be 4-D, got {x.dim()}-D")
    if not x.is_contiguous():
        raise RuntimeError(f"{name}: x must be contiguous")
    if x.numel() >= 2 ** 31:
        raise RuntimeError(f"{name}: x has 2^31 or more elements")
    m = _backend(x)
    if m is None:
        ref = _ref.to_nhwc if to_nhwc else _ref.to_nchw
        y = ref(x, dtype)
        return y if out is None else out.copy_(y)
    return m.layout_convert(x, to_nhwc, dtype == torch.bfloat16, out)


def to_nhwc(x, dtype=None, out=None):
    """[N, C, H, W] -> a fresh contiguous [N, H, W, C] tensor of `dtype`
    (None = x's). x is contiguous fp32 or bf16; fp32 -> bf16 rounds to
    nearest even like x.to(torch.bfloat16), bf16 -> fp32 is exact. One HIP
    launch on the GPU (csrc/layout.hip). out: a contiguous tensor of the
    result's shape and dtype to write into instead of allocating."""
    return _layout_convert(x, dtype, out, True)


def to_nchw(x, dtype=None, out=None):
    """[N, H, W, C] -> [N, C, H, W]; the inverse of to_nhwc, same rules."""
    return _layout_convert(x, dtype, out, False)


def linear(x, w, bias=None):
    m = _backend(x)
    if m is None:
        return _ref.linear(x, w, bias)
    return m.linear(x, w, bias)


def softmax(x):
    m = _backend(x)
    if m is None:
        if x.dim() < 1 or x.numel() == 0:
            raise RuntimeError("softmax of nothing")
        return _ref.softmax(x)
    return m.softmax(x)
