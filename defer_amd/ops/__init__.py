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


# activation names -> the codes of the bindings (ACT_* of csrc/kernels.h)
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


_VEC_DTYPES = {torch.bfloat16: 8, torch.float32: 4}


def _check_channel_vec(name, x, params, c_max=None):
    """The rules the 16-byte-vector kernels share, for every device: x is a
    contiguous bf16 or fp32 tensor whose channel count is a multiple of one
    vector, and every fp32 [C] parameter lives on x's device. Each refusal
    names its rule."""
    if x.dtype not in _VEC_DTYPES:
        raise RuntimeError(f"{name}: x must be bf16 or fp32, got {x.dtype}")
    if not x.is_contiguous():
        raise RuntimeError(f"{name}: x must be contiguous")
    c, vec = x.shape[-1], _VEC_DTYPES[x.dtype]
    if c == 0 or c % vec:
        raise RuntimeError(
            f"{name}: {x.dtype} needs C % {vec} == 0 (16-byte channel "
            f"vectors), got C = {c}")
    if c_max is not None and c > c_max:
        raise RuntimeError(f"{name}: needs C <= {c_max}, got C = {c}")
    for pname, p in params:
        if p is None:
            continue
        if p.device != x.device:
            raise RuntimeError(
                f"{name}: {pname} must be on x's device {x.device}, got "
                f"{p.device}")
        if (p.dtype != torch.float32 or not p.is_contiguous()
                or tuple(p.shape) != (c,)):
            raise RuntimeError(
                f"{name}: {pname} must be a contiguous fp32[C] with C = {c}, "
                f"got {p.dtype} {tuple(p.shape)}")


def dwconv7x7(x, w, bias=None, max_blocks=0):
    """7x7 depthwise conv, stride 1, padding 3, NHWC x and [7, 7, C] w in
    x's dtype, fp32 bias [C] or None; the output has x's shape:

        y[n, oh, ow, c] = sum_{r,s} x[n, oh-3+r, ow-3+s, c] * w[r, s, c]
                          + bias[c]

    No scale and no activation (ConvNeXt has neither here). On the GPU one
    HIP kernel (csrc/dwconv7.hip) that stages each tile's window and the
    weights in LDS; C % 8 == 0 (bf16) or C % 4 == 0 (fp32), anything else
    raises, on the CPU too. fp32 fmaf in the fixed tap order (r, then s),
    one rounding, run-to-run identical. N == 0 gives an empty tensor.
    max_blocks caps the grid along the tiles (0 = policy), so a few
    workgroups walk many tiles."""
    if x.dim() != 4 or w.dim() != 3:
        raise RuntimeError(
            f"dwconv7x7: x must be NHWC (4-D) and w [7, 7, C] (3-D), got "
            f"{x.dim()}-D and {w.dim()}-D")
    if w.dtype != x.dtype:
        raise RuntimeError(
            f"dwconv7x7: w must be {x.dtype} like x (mixed dtypes), got "
            f"{w.dtype}")
    _check_channel_vec("dwconv7x7", x, (("bias", bias),))
    if tuple(w.shape) != (7, 7, x.shape[-1]):
        raise RuntimeError(
            f"dwconv7x7: w must be [7, 7, C] with C = {x.shape[-1]}, got "
            f"{tuple(w.shape)}")
    if w.device != x.device or not w.is_contiguous():
        raise RuntimeError(
            f"dwconv7x7: w must be contiguous on x's device {x.device}")
    m = _backend(x)
    if m is None:
        return _ref.dwconv7x7(x, w, bias)
    return m.dwconv7x7(x, w, bias, max_blocks)


LAYERNORM_MAX_C = 2048


def layernorm_channels(x, weight, bias, eps=1e-6, max_blocks=0):
    """LayerNorm over the last (channel) dim of a contiguous x of rank >= 2,
    per leading index, with fp32 weight and bias [C]:

        y[..., c] = (x[..., c] - mean) / sqrt(var + eps) * weight[c] + bias[c]

    var is the biased variance. On the GPU one HIP kernel (csrc/layernorm.hip):
    a row is read once, kept in registers and written once; mean, then the
    sum of squared differences from it, in fp32 by xor-shuffle trees; one
    rounding. C % 8 == 0 (bf16) or C % 4 == 0 (fp32) and C <= 2048, anything
    else raises, on the CPU too. No host sync. max_blocks caps the grid (0 =
    policy)."""
    if x.dim() < 2:
        raise RuntimeError(
            f"layernorm_channels: x must have rank >= 2, got {x.dim()}-D")
    _check_channel_vec("layernorm_channels", x,
                       (("weight", weight), ("bias", bias)), LAYERNORM_MAX_C)
    m = _backend(x)
    if m is None:
        return _ref.layernorm_channels(x, weight, bias, eps)
    return m.layernorm_channels(x, weight, bias, eps, max_blocks)


def linear_gelu(x, w, bias=None):
    """gelu(x @ w.T + bias) for x [..., Cin] and w [Cout, Cin]: the exact
    (erf) GELU, 0.5 * v * (1 + erf(v * 0.70710678)), in fp32 before the one
    rounding. On the GPU the GEMM-mode kernels of linear and the 1x1 convs
    with a GELU epilogue (bf16: instantiations of their own in csrc/conv.hip;
    fp32: the runtime act of csrc/conv_f32.hip), with their shape rules:
    Cin % 8 == 0 (bf16) or Cin % 4 == 0 and Cout % 4 == 0 (fp32). This is the
    only way to a GELU: no op takes it as an `act`."""
    if x.dim() < 1 or w.dim() != 2 or w.shape[1] != x.shape[-1]:
        raise RuntimeError(
            f"linear_gelu: x must be [..., Cin] and w [Cout, Cin], got "
            f"{tuple(x.shape)} and {tuple(w.shape)}")
    m = _backend(x)
    if m is None:
        return _ref.linear_gelu(x, w, bias)
    if not x.is_contiguous():
        raise RuntimeError("linear_gelu: x must be contiguous")
    y = m.linear_gelu(x.reshape(-1, x.shape[-1]), w, bias)
    return y.reshape(*x.shape[:-1], w.shape[0])


ATTENTION_D = 64


def attention(qkv, heads):
    """Multi-head attention on a fused qkv: qkv is a contiguous
    [..., T, 3 * C] of rank >= 3, bf16 or fp32, C = heads * D, with the last
    dim laid out [3][heads][D] (q of all heads, then k, then v: what one
    fused QKV linear produces); the leading dims are flattened to N. The
    result is [..., T, C] in qkv's dtype:

        out[n, t, h*D + d] = sum_j P[n, h, t, j] * v[n, j, h, d]
        P[n, h, t, :]      = softmax_j((q[n, t, h, :] . k[n, j, h, :]) * D^-0.5)

    Non-causal, no mask, no dropout. D == 64, T >= 1 and fewer than 2^31
    elements, anything else raises, on the CPU too; N == 0 gives an empty
    tensor. On the GPU one HIP kernel (csrc/attention.hip) reads q, k and v
    in place and never writes the scores. Numerics: S is accumulated in
    fp32; the scale 0.125 is exact; the softmax runs in fp32 with a running
    max over key tiles of 64; the row sum l sums the fp32 p; in bf16, P is
    rounded to bf16 (nearest even) only as the operand of the second MFMA; O
    is accumulated in fp32 and divided by l once; one rounding to the output
    dtype. No atomics and a fixed order of key tiles: run-to-run
    identical. The CPU branch (ops/reference.py) keeps P in fp32."""
    if qkv.dtype not in _VEC_DTYPES:
        raise RuntimeError(
            f"attention: qkv must be bf16 or fp32, got {qkv.dtype}")
    if qkv.dim() < 3:
        raise RuntimeError(
            f"attention: qkv must be [..., T, 3 * C] with rank >= 3, got "
            f"{qkv.dim()}-D")
    if not qkv.is_contiguous():
        raise RuntimeError("attention: qkv must be contiguous")
    t, c3 = qkv.shape[-2], qkv.shape[-1]
    if heads < 1 or c3 == 0 or c3 % (3 * heads):
        raise RuntimeError(
            f"attention: the last dim must be 3 * heads * D, got {c3} for "
            f"heads = {heads}")
    if c3 // (3 * heads) != ATTENTION_D:
        raise RuntimeError(
            f"attention: needs D == {ATTENTION_D} (head dim), got D = "
            f"{c3 // (3 * heads)}")
    if t < 1:
        raise RuntimeError(f"attention: needs T >= 1, got T = {t}")
    if qkv.numel() >= 2 ** 31:
        raise RuntimeError("attention: qkv has 2^31 or more elements")
    m = _backend(qkv)
    if m is None:
        return _ref.attention(qkv, heads)
    return m.attention(qkv, heads)


def attention_plan(t):
    """The bf16 attention kernel's work split for t tokens, a pure function
    of t: {"groups": 16-row query groups, "groups_per_wave", "blocks":
    workgroups per (image, head), "groups_per_block", "lds_bytes"}. Needs
    the built extension but no GPU."""
    return dict(_built().attention_plan(t))


WINDOW_ATTENTION_D = 32


def window_attention(qkv, bias_table, heads, window, shift=0):
    """Swin's shifted-window attention on a fused NHWC qkv: qkv is a
    contiguous [N, H, W, 3 * C], bf16 or fp32, C = heads * 32, with the last
    dim laid out [3][heads][32] (what the block's qkv 1x1 conv writes);
    bias_table is the learned relative-position bias, a contiguous
    [(2 * window - 1)**2, heads] in qkv's dtype. The result is [N, H, W, C]
    in qkv's dtype. With w = window, s = shift, T = w * w:

        shifted frame: (r', c') holds pixel ((r' + s) % H, (c' + s) % W),
            i.e. torch.roll(x, (-s, -s), (1, 2))
        window (r' // w, c' // w), token t = (r' % w) * w + (c' % w) = (i, j)
        score(tq, tk) = (q . k) * 32**-0.5
            + bias_table[(iq - ik + w - 1) * (2w - 1) + (jq - jk + w - 1), head]
            + mask
        mask = -100 (added, not an exclusion) when s > 0 and the tokens' row
            regions or column regions differ; the region of a shifted row r'
            is 0 for r' < H - w, 1 for r' < H - s, else 2; columns with W
        out[pixel of tq] = sum_tk softmax_tk(score)[tk] * v[pixel of tk]

    These are the semantics of the original implementation and of
    torchvision. On the GPU one HIP kernel (csrc/window_attention.hip) does
    the roll, the partition, the bias gather, the mask and their inverses in
    its addressing: nothing but qkv is read and nothing but the result
    written, with no host sync. Scores, bias, softmax and normalisation are
    fp32; in bf16, P is rounded to bf16 once as the operand of the second
    MFMA; one rounding of the output; run-to-run identical. dtype, a 4-D
    contiguous qkv, last dim 3 * heads * 32, 2 <= window with window**2 <=
    64, window dividing H and W, 0 <= shift < window, the table's shape and
    dtype, and fewer than 2^31 elements: anything else raises, on the CPU
    too. N == 0 gives an empty tensor. The CPU branch (ops/reference.py)
    keeps P in fp32."""
    if qkv.dtype not in _VEC_DTYPES:
        raise RuntimeError(
            f"window_attention: qkv must be bf16 or fp32, got {qkv.dtype}")
    if qkv.dim() != 4:
        raise RuntimeError(
            f"window_attention: qkv must be NHWC (4-D), got {qkv.dim()}-D")
    if not qkv.is_contiguous():
        raise RuntimeError("window_attention: qkv must be contiguous")
    h, w, c3 = qkv.shape[1:]
    if heads < 1 or c3 != 3 * heads * WINDOW_ATTENTION_D:
        raise RuntimeError(
            f"window_attention: the last dim must be 3 * heads * "
            f"{WINDOW_ATTENTION_D}, got {c3} for heads = {heads}")
    if window < 2 or window * window > 64:
        raise RuntimeError(
            f"window_attention: needs 2 <= window and window^2 <= 64, got "
            f"window = {window}")
    if h == 0 or w == 0 or h % window or w % window:
        raise RuntimeError(
            f"window_attention: window must divide H and W, got {h}x{w} for "
            f"window = {window}")
    if not 0 <= shift < window:
        raise RuntimeError(
            f"window_attention: needs 0 <= shift < window, got shift = "
            f"{shift}")
    want = ((2 * window - 1) ** 2, heads)
    if (bias_table.dtype != qkv.dtype or bias_table.device != qkv.device
            or not bias_table.is_contiguous()
            or tuple(bias_table.shape) != want):
        raise RuntimeError(
            f"window_attention: bias_table must be a contiguous {qkv.dtype} "
            f"[(2*window - 1)^2, heads] = {list(want)} on qkv's device "
            f"(mixed dtypes), got {bias_table.dtype} "
            f"{tuple(bias_table.shape)}")
    if qkv.numel() >= 2 ** 31:
        raise RuntimeError("window_attention: qkv has 2^31 or more elements")
    m = _backend(qkv)
    if m is None:
        return _ref.window_attention(qkv, bias_table, heads, window, shift)
    return m.window_attention(qkv, bias_table, heads, window, shift)


def window_attention_plan(n, h, w, heads, window):
    """The bf16 window attention kernel's work split for an [n, h, w, 3 *
    heads * 32] qkv, a pure function of the shape: {"tokens": T, "groups":
    16-row query groups of a window, "windows": per image, "pairs": (image,
    window, head) triples, one wave each, "blocks": workgroups of four
    waves, "idle_waves": in the last block, "lds_bytes"}. Needs the built
    extension but no GPU."""
    return dict(_built().window_attention_plan(n, h, w, heads, window))


def patch_merge(x):
    """Swin's patch merging gather, NHWC [N, H, W, C] -> [N, H/2, W/2, 4C]:
    the four pixels of each 2x2 patch side by side in the channels, in
    torchvision's order (even row, even col), (odd, even), (even, odd),
    (odd, odd):

        y[n, oh, ow, k*C + c] = x[n, 2*oh + (k & 1), 2*ow + (k >> 1), c]

    A copy, bit for bit; on the GPU one 16-byte-vector HIP kernel. Odd H or
    W raises, and C % 8 == 0 (bf16) or C % 4 == 0 (fp32), on the CPU too."""
    if x.dim() != 4:
        raise RuntimeError(
            f"patch_merge: x must be NHWC (4-D), got {x.dim()}-D")
    _check_channel_vec("patch_merge", x, ())
    if x.shape[1] % 2 or x.shape[2] % 2:
        raise RuntimeError(
            f"patch_merge: H and W must be even, got {x.shape[1]}x"
            f"{x.shape[2]}")
    m = _backend(x)
    if m is None:
        return _ref.patch_merge(x)
    return m.patch_merge(x)


def embed_tokens(x, cls, pos):
    """NHWC x [N, H, W, C] -> tokens [N, 1, 1 + H*W, C] with a class token:

        y[n, 0, 0, :]     = cls + pos[0]
        y[n, 0, 1 + t, :] = x[n, t, :] + pos[1 + t]      (t over H*W)

    cls is fp32 [C], pos [1 + H*W, C] in x's dtype. fp32 sums, one rounding.
    On the GPU one 16-byte-vector HIP kernel; C % 8 == 0 (bf16) or
    C % 4 == 0 (fp32), anything else raises, on the CPU too."""
    if x.dim() != 4:
        raise RuntimeError(
            f"embed_tokens: x must be NHWC (4-D), got {x.dim()}-D")
    _check_channel_vec("embed_tokens", x, (("cls", cls),))
    want = (1 + x.shape[1] * x.shape[2], x.shape[3])
    if (pos.dtype != x.dtype or pos.device != x.device
            or not pos.is_contiguous() or tuple(pos.shape) != want):
        raise RuntimeError(
            f"embed_tokens: pos must be a contiguous {x.dtype} "
            f"[1 + H*W, C] = {list(want)} on x's device (mixed dtypes), got "
            f"{pos.dtype} {tuple(pos.shape)}")
    m = _backend(x)
    if m is None:
        return _ref.embed_tokens(x, cls, pos)
    return m.embed_tokens(x, cls, pos)


def class_token(x):
    """[N, 1, T, C] -> [N, C]: token 0 of every image. On the GPU one strided
    device copy, as in concat_channels (no compute kernel; a memcpy node
    under hipGraph capture)."""
    if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] < 1:
        raise RuntimeError(
            f"class_token: x must be [N, 1, T, C] with T >= 1, got "
            f"{tuple(x.shape)}")
    if not x.is_contiguous():
        raise RuntimeError("class_token: x must be contiguous")
    m = _backend(x)
    if m is None:
        return _ref.class_token(x)
    return m.class_token(x)


_GCONV_CG = (4, 8, 16, 32)


def _check_gconv(x, w, stride, padding):
    """The geometry csrc/gconv.hip serves; the same refusals on every
    device, each naming the value it refuses."""
    if x.dim() != 4 or w.dim() != 4:
        raise ValueError(
            f"gconv2d_bn_act: x must be NHWC and w [C, 3, 3, Cg], got "
            f"{x.dim()}-D and {w.dim()}-D")
    c, cg = x.shape[-1], w.shape[-1]
    if tuple(w.shape[1:3]) != (3, 3):
        raise ValueError(
            f"gconv2d_bn_act: needs a 3x3 kernel, got "
            f"{w.shape[1]}x{w.shape[2]}")
    if cg not in _GCONV_CG:
        raise ValueError(
            f"gconv2d_bn_act: needs {list(_GCONV_CG)} channels per group, "
            f"got {cg}")
    if c % 16 or c % cg or w.shape[0] != c:
        raise ValueError(
            f"gconv2d_bn_act: needs Cout == Cin == C with C % 16 == 0 and "
            f"C % Cg == 0, got C = {c}, Cout = {w.shape[0]}, Cg = {cg}")
    if stride not in (1, 2):
        raise ValueError(
            f"gconv2d_bn_act: needs stride 1 or 2, got {stride}")
    if padding not in (0, 1):
        raise ValueError(
            f"gconv2d_bn_act: needs padding 0 or 1, got {padding}")
    if x.dtype not in (torch.bfloat16, torch.float32) or w.dtype != x.dtype:
        raise ValueError(
            f"gconv2d_bn_act: x and w must both be bf16 or both fp32, got "
            f"{x.dtype} and {w.dtype}")


def gconv2d_bn_act(x, w, scale=None, bias=None, stride=1, padding=1,
                   act="none"):
    """Grouped 3x3 conv + folded BN + activation, NHWC x and w [C, 3, 3, Cg]
    (OHWI with I = the channels of one group), groups = C // Cg:

        y[n, oh, ow, k] = act(scale[k] * sum_{r,s,c<Cg} x[n, oh*stride - pad
                              + r, ow*stride - pad + s, (k // Cg)*Cg + c]
                              * w[k, r, s, c] + bias[k])

    scale and bias are fp32 [C] (None = 1 / 0); act as in conv2d_bn_act. On
    the GPU one HIP kernel (csrc/gconv.hip; bf16 on the MFMA) for Cin ==
    Cout == C, C % 16 == 0, Cg in {4, 8, 16, 32}, stride in {1, 2} and
    padding in {0, 1}; any other geometry raises, on the CPU too. fp32
    accumulation in one fixed order, one rounding at the end, run-to-run
    identical. Non-finite inputs are outside the contract: the bf16 kernel
    multiplies the other groups' values of a 16-channel slab by zero
    weights, so an inf in one group can make NaNs in its slab neighbours."""
    code = _act_code(act)
    _check_gconv(x, w, stride, padding)
    m = _backend(x)
    if m is None:
        return _ref.gconv2d_bn_act(x, w, scale, bias, stride, padding, act)
    return m.gconv2d_bn_act(x, w, scale, bias, stride, padding, code)


_FP8 = torch.float8_e4m3fn
_FP8_ACTS = ("none", "relu", "relu6")


def quantize_fp8(x, scale, max_blocks=0):
    """x / scale as OCP e4m3 (torch.float8_e4m3fn): byte for byte
    (x.float() * inv).clamp(-448, 448).to(torch.float8_e4m3fn) with inv =
    1 / scale rounded to fp32, round to nearest even, saturating. x is bf16
    or fp32 with numel % 16 == 0; scale a positive host float (no sync). On
    the GPU one HIP kernel (csrc/conv_fp8.hip); max_blocks caps its grid
    (0 = policy)."""
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"quantize_fp8: x must be bf16 or fp32, got "
                         f"{x.dtype}")
    if x.numel() % 16:
        raise ValueError(f"quantize_fp8: needs numel % 16 == 0, got "
                         f"{x.numel()}")
    if not scale > 0.0:
        raise ValueError(f"quantize_fp8: scale must be > 0, got {scale}")
    m = _backend(x)
    if m is None:
        return _ref.quantize_fp8(x, 1.0 / scale)
    return m.quantize_fp8(x, 1.0 / scale, max_blocks)


def _check_conv_fp8(x, w, scale, bias, stride, padding, residual):
    """The contract of csrc/conv_fp8.hip; the same refusals on every
    device, each naming the value it refuses."""
    for name, t in (("x_q", x), ("w_q", w), ("residual_q", residual)):
        if t is not None and t.dtype != _FP8:
            raise ValueError(f"conv2d_bn_act_fp8: {name} must be "
                             f"torch.float8_e4m3fn, got {t.dtype}")
    if x.dim() != 4 or w.dim() != 4:
        raise ValueError(
            f"conv2d_bn_act_fp8: x_q must be NHWC and w_q OHWI, got "
            f"{x.dim()}-D and {w.dim()}-D")
    cout, r, s, cin = w.shape
    if x.shape[-1] != cin or cin % 16 or cout % 16:
        raise ValueError(
            f"conv2d_bn_act_fp8: needs Cin % 16 == 0 and Cout % 16 == 0 "
            f"with x_q and w_q agreeing on Cin, got x_q {tuple(x.shape)} "
            f"and w_q {tuple(w.shape)}")
    if r != s:
        raise ValueError(f"conv2d_bn_act_fp8: needs a square kernel, got "
                         f"{r}x{s}")
    if stride not in (1, 2):
        raise ValueError(f"conv2d_bn_act_fp8: needs stride 1 or 2, got "
                         f"{stride}")
    if not 0 <= padding <= r // 2:
        raise ValueError(f"conv2d_bn_act_fp8: needs 0 <= padding <= "
                         f"{r // 2}, got {padding}")
    for name, t in (("scale", scale), ("bias", bias)):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32
                or t.device != x.device or t.numel() != cout):
            raise ValueError(
                f"conv2d_bn_act_fp8: {name} must be an fp32 tensor of "
                f"{cout} values on {x.device}")
    if residual is not None:
        oh = (x.shape[1] + 2 * padding - r) // stride + 1
        ow = (x.shape[2] + 2 * padding - s) // stride + 1
        if tuple(residual.shape) != (x.shape[0], oh, ow, cout):
            raise ValueError(
                f"conv2d_bn_act_fp8: residual_q must have the output's "
                f"shape {(x.shape[0], oh, ow, cout)}, got "
                f"{tuple(residual.shape)}")


def conv2d_bn_act_fp8(x_q, w_q, scale, bias, stride=1, padding=0,
                      act="none", residual_q=None, res_scale=1.0,
                      out_scale=None, max_blocks=0):
    """Convolution on e4m3 bytes with fp32 accumulation, NHWC x_q and OHWI
    w_q (torch.float8_e4m3fn), for output channel c in fp32:

        v = act(acc * scale[c] + bias[c] + res_scale * float(residual_q))

    scale[c] carries the folded BN scale times the input's activation scale
    times channel c's weight scale. out_scale=None returns bf16 (one
    rounding of v); otherwise e4m3 of clamp(v / out_scale, -448, 448), round
    to nearest even, with 1 / out_scale rounded to fp32 first. res_scale and
    out_scale are host floats: no sync, capturable. act is "none", "relu" or
    "relu6". On the GPU one HIP kernel on the fp8 MFMA (csrc/conv_fp8.hip)
    for Cin % 16 == 0, Cout % 16 == 0, a square kernel, stride 1 or 2 and
    padding <= R // 2; anything else raises, on the CPU too. Deterministic.
    max_blocks caps the grid (0 = policy)."""
    code = _act_code(act, _FP8_ACTS)
    _check_conv_fp8(x_q, w_q, scale, bias, stride, padding, residual_q)
    inv = None if out_scale is None else 1.0 / out_scale
    m = _backend(x_q)
    if m is None:
        return _ref.conv2d_bn_act_fp8(x_q, w_q, scale, bias, stride, padding,
                                      act, residual_q, res_scale, inv)
    return m.conv2d_bn_act_fp8(x_q, w_q, scale, bias, residual_q, stride,
                               padding, code, res_scale, inv, max_blocks)


def conv_fp8_plan(x_shape, w_shape, stride=1, padding=0, max_blocks=0):
    """What conv2d_bn_act_fp8 would launch for these NHWC / OHWI shapes,
    without launching it: {"tile": "large" (128x128) or "small" (64x64),
    "bm", "bn", "m_tiles", "n_tiles", "k_tiles", "grid", "lds_bytes",
    "mfma": "fp8", or "bf16" for K < 128 (the bytes widened in registers)}.
    Needs the built extension but no GPU."""
    return dict(_built().conv_fp8_plan(list(x_shape), list(w_shape), stride,
                                       padding, max_blocks))


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
