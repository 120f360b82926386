"""Checkers for the bf16 conv kernels of csrc/conv.hip and csrc/conv_ws.hip
(a helper module like ops_checks.py and se_checks.py, not collected as
tests). Two checks, both over every output element, neither with a figure
taken from a kernel.

**Exact integers** (`exact_case`, `expected`, `check_exact`). x is an integer
in [-4, 4], w an integer in [-2, 2], `scale` is drawn per channel from {3,
-3, 6}, `bias` and `residual` are multiples of 3 (|residual| <= 255, exact
in bf16; bias is fp32 and reaches +-1020 on half of the channels, so that
shallow convs, too, leave the range where every integer is a bf16 number).
Every product is an integer and every partial sum of K <= 2^17 of them is
below 2^24, so the fp32 accumulator is exact in any summation order and with
any MFMA, and so is the epilogue value v = scale * conv + bias + residual, a
multiple of 3. The output must then be the one round-to-nearest-even of v
(none), of max(v, 0) (relu) or of 0 / 3 / 6 (relu6). Hardswish sees only its
exact regions (`ops.hardswish`: v <= -3 gives 0, 0 gives 0, v >= 3 gives v
bit for bit). `expected` computes this in float64 and converts float64 ->
float32 -> bf16; `check_exact` is `torch.equal`. `linear_case` is the same
with w in 3 * [-2, 2] in place of the scale, for `ops.linear`.

The premises of that argument are asserted on every case when it is made
(`premises`, raising PremiseError): the fp32 CPU conv equals the float64
one; max|v| < 2^24; all v are multiples of 3; at least 10 % of |v| are no
bf16 numbers, so a truncating epilogue fails; ties occur (odd integers in
(256, 512)), so round-to-even is exercised; v <= -3, v == 0 and v >= 6 all
occur; all three scales occur, and inside the last, partial n-tile (64 or
128 columns wide) where there is one.

**Random floats** (`float_case`, `gelu_case`, `check_bound`). Against a
float64 truth t of the inputs as rounded to bf16,

    |got - t| <= u_b |t| + L (K + 7) u mag     (+ 4 GELU_E0 for GELU)

with u_b = 2^-8 (one rounding to bf16), u = 2^-24 (one fp32 operation), K =
R * S * Cin, mag the same conv of absolute values (|scale| * (|x| conv |w|)
+ |bias| + |residual|) and L the largest slope of the activation, which
carries the fp32 error of its argument: 3/2 for none / relu / relu6 /
hardswish, the bound test_se_gpu.py holds these kernels to at the MobileNetV3
shapes, and 1.13 for GELU with the GELU term of test_convnext_gpu.py (see
GELU_E0). The inputs are post-activation-like (x = relu(randn), bias and
residual non-negative), so mag / |t| stays small and the u_b term dominates:
an activation applied to an already rounded pre-activation adds up to L u_b
|v| and breaks it. The bound assumes round-to-nearest fp32 accumulation.

A case is made once per geometry and seed (module-level caches), its
reference convs run once, and every (act, residual) expectation derives
from them. Cases are shared: treat their tensors as read-only.
"""

import functools
import types

import torch
import torch.nn.functional as F

U = 2.0 ** -24
U_B = 2.0 ** -8
# restated from tests/test_convnext_gpu.py (docs/TESTING.md, ConvNeXt): the
# worst error of fp32 F.gelu on the CPU against float64 over 2,000,001 points
# of [-10, 10], measured 1.207e-6 at v = 3.49; kernels get 4x for another erff
GELU_E0 = 1.21e-6
BF16 = torch.bfloat16

ACTS = ("none", "relu", "relu6", "hardswish")
SCALES = (3.0, -3.0, 6.0)
N_TILES = (64, 128)            # the n-tile widths of the conv kernels
SLOPE = {"none": 1.5, "relu": 1.5, "relu6": 1.5, "hardswish": 1.5,
         "gelu": 1.13}


class PremiseError(AssertionError):
    """A case does not have a property that the exact check relies on."""


def out_hw(xs, r, stride, pad):
    return ((xs[1] + 2 * pad - r) // stride + 1,
            (xs[2] + 2 * pad - r) // stride + 1)


def conv_nhwc(x, w, stride, pad, dtype=torch.float64):
    """conv2d of NHWC x with OHWI w in `dtype` on the CPU, NHWC result."""
    y = F.conv2d(x.cpu().to(dtype).permute(0, 3, 1, 2),
                 w.cpu().to(dtype).permute(0, 3, 1, 2), None, stride, pad)
    return y.permute(0, 2, 3, 1).contiguous()


def _bf16_number(v):
    """Which elements of the float64 tensor v are bf16 numbers."""
    return v.float().to(BF16).double() == v


def _require(cond, what):
    if not bool(cond):
        raise PremiseError(what)


def premises(x, w, scale, bias, res, stride, pad):
    """Assert what the exact check relies on (module docstring) for these
    tensors, with and without the residual; returns (v, v + residual) in
    float64. scale None means 1."""
    c64 = conv_nhwc(x, w, stride, pad)
    c32 = conv_nhwc(x, w, stride, pad, torch.float32)
    _require(torch.equal(c32.double(), c64),
             "the fp32 CPU conv differs from the float64 one")
    _require(torch.equal(x.to(BF16).double(), x.double())
             and torch.equal(w.to(BF16).double(), w.double())
             and torch.equal(res.to(BF16).double(), res.double()),
             "x, w and residual must be bf16 numbers")
    cout = w.shape[0]
    if scale is not None:
        _require((scale.double() % 3 == 0).all(),
                 "a scale that is no multiple of 3")
        have = set(scale.tolist())
        _require(have == set(SCALES), f"scales {sorted(have)}, not all of "
                                      f"{SCALES}")
        for bn in N_TILES:
            tail = cout % bn
            if tail:
                got = set(scale[-tail:].tolist())
                _require(len(got) == min(tail, 3),
                         f"the last, partial n-tile of {bn} holds scales "
                         f"{sorted(got)} only")
        c64 = c64 * scale.double()
    v = c64 + bias.double()
    both = (v, v + res.double())
    for name, t in zip(("v", "v + residual"), both):
        _require(t.abs().max() < 2 ** 24, f"max|{name}| >= 2^24")
        _require((t % 3 == 0).all(), f"{name} has non-multiples of 3")
        frac = 1.0 - _bf16_number(t).double().mean().item()
        _require(frac >= 0.10, f"only {frac:.1%} of {name} are no bf16 "
                               "numbers: a truncating epilogue could pass")
        a = t.abs()
        _require(((a > 256) & (a < 512) & (a % 2 == 1)).any(),
                 f"{name} has no tie (odd integer in (256, 512))")
        _require((t <= -3).any() and (t == 0).any() and (t >= 6).any(),
                 f"{name} misses one of v <= -3, v == 0, v >= 6")
    return both


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _exact_bias(g, cout):
    """Multiples of 3: small on about half of the channels, up to +-1020 on
    the others."""
    small = _randint(g, -4, 4, (cout,))
    large = _randint(g, -340, 340, (cout,))
    pick = torch.rand(cout, generator=g) < 0.5
    return torch.where(pick, large, small) * 3


def _case(**kw):
    return types.SimpleNamespace(**kw)


@functools.lru_cache(maxsize=None)
def exact_case(xs, cout, r, stride, pad, seed=0):
    """The exact-integer case of a geometry (NHWC x shape, Cout, R, stride,
    pad) and seed, its premises asserted. Fields: x, w, res (bf16), scale,
    bias (fp32), v (float64, indexed by has_res), and the geometry."""
    g = torch.Generator().manual_seed(1000 * seed + sum(xs) + cout + r)
    cin = xs[3]
    oh, ow = out_hw(xs, r, stride, pad)
    x = _randint(g, -4, 4, xs)
    w = _randint(g, -2, 2, (cout, r, r, cin))
    scale = torch.tensor(SCALES)[torch.randint(0, 3, (cout,), generator=g)]
    n = min(3, cout)
    scale[cout - n:] = torch.tensor(SCALES)[torch.randperm(3, generator=g)][:n]
    bias = _exact_bias(g, cout)
    res = _randint(g, -85, 85, (xs[0], oh, ow, cout)) * 3
    v = premises(x, w, scale, bias, res, stride, pad)
    return _case(xs=xs, cout=cout, r=r, stride=stride, pad=pad,
                 K=r * r * cin, x=x.to(BF16), w=w.to(BF16), scale=scale,
                 bias=bias, res=res.to(BF16), v=v)


@functools.lru_cache(maxsize=None)
def linear_case(m, k, n, seed=0):
    """Exact integers for ops.linear: x [m, k] in [-4, 4], w [n, k] in 3 *
    [-2, 2], bias a multiple of 3; the premises but those on the scale."""
    g = torch.Generator().manual_seed(1000 * seed + m + k + n)
    x = _randint(g, -4, 4, (m, k))
    w = _randint(g, -2, 2, (n, k)) * 3
    bias = _exact_bias(g, n)
    v = premises(x.view(m, 1, 1, k), w.view(n, 1, 1, k), None, bias,
                 torch.zeros(m, 1, 1, n), 1, 0)[0].view(m, n)
    return _case(x=x.to(BF16), w=w.to(BF16), bias=bias, v=(v, v), K=k)


def expected(case, act, has_res=False):
    """What a correct kernel returns for an exact case: float64 -> float32
    -> bf16 of act(v)."""
    v = case.v[bool(has_res)]
    if act == "none":
        e = v
    elif act == "relu":
        e = v.clamp(min=0)
    elif act == "relu6":
        e = v.clamp(0, 6)
    elif act == "hardswish":
        # multiples of 3 lie in the exact regions only
        assert ((v <= -3) | (v == 0) | (v >= 3)).all()
        e = torch.where(v >= 3, v, torch.zeros_like(v))
    else:
        raise ValueError(f"act={act!r}: expected one of {list(ACTS)}")
    return e.float().to(BF16)


def check_exact(case, act, has_res, got, what="conv", tile=None):
    """torch.equal of `got` to expected(case, act, has_res) over every
    element. A mismatch names the first differing (row, column) of the
    [M, Cout] output and, given tile = (BM, BN), the tile it falls in."""
    want = expected(case, act, has_res)
    got = got.detach().cpu()
    assert got.dtype == BF16 and got.shape == want.shape, (got.dtype,
                                                           got.shape)
    if torch.equal(got, want):
        return
    cout = want.shape[-1]
    # compare numbers, not bits: NaN != NaN counts, -0 == 0 does not
    bad = (got.float() != want.float()).reshape(-1, cout).nonzero()
    row, col = bad[0].tolist()
    where = "" if tile is None else (
        f", tile (m, n) = ({row // tile[0]}, {col // tile[1]}) of "
        f"{tile[0]}x{tile[1]}")
    raise AssertionError(
        f"{what} {act} res={bool(has_res)}: {bad.shape[0]} of "
        f"{want.numel()} outputs differ, first at (row, column) ({row}, "
        f"{col}){where}: got {got.reshape(-1, cout)[row, col].item()!r}, "
        f"want {want.reshape(-1, cout)[row, col].item()!r}, v = "
        f"{case.v[bool(has_res)].reshape(-1, cout)[row, col].item()!r}")


# ------------------------------------------------------------ random floats
def _float_fields(x, w, scale, bias, res, stride, pad):
    """(t, mag), each indexed by has_res, in float64 from rounded inputs."""
    c = conv_nhwc(x, w, stride, pad)
    m = conv_nhwc(x.abs(), w.abs(), stride, pad)
    if scale is not None:
        c, m = c * scale.double(), m * scale.double().abs()
    c, m = c + bias.double(), m + bias.double().abs()
    return (c, c + res.double()), (m, m + res.double().abs())


@functools.lru_cache(maxsize=None)
def float_case(xs, cout, r, stride, pad, seed=0):
    """Random post-activation-like floats for a geometry: x = relu(randn), w
    = randn * sqrt(2 / K), scale in [0.5, 1.5), bias and residual >= 0, x, w
    and residual rounded to bf16 before the truth is taken."""
    g = torch.Generator().manual_seed(2000 * seed + sum(xs) + cout + r)
    cin = xs[3]
    K = r * r * cin
    oh, ow = out_hw(xs, r, stride, pad)
    x = torch.randn(*xs, generator=g).clamp(min=0).to(BF16)
    w = (torch.randn(cout, r, r, cin, generator=g) * (2.0 / K) ** 0.5
         ).to(BF16)
    scale = torch.rand(cout, generator=g) + 0.5
    bias = torch.rand(cout, generator=g) * 0.5
    res = torch.randn(xs[0], oh, ow, cout, generator=g).clamp(min=0).to(BF16)
    v, mag = _float_fields(x, w, scale, bias, res, stride, pad)
    return _case(xs=xs, cout=cout, r=r, stride=stride, pad=pad, K=K, x=x,
                 w=w, scale=scale, bias=bias, res=res, v=v, mag=mag)


@functools.lru_cache(maxsize=None)
def gelu_case(m, k, n, seed=0):
    """Non-negative integers for ops.linear_gelu: x [m, k] in [0, 4] with
    every 5th row all zero, w [n, k] in [0, 2] at a density that falls with
    the column so that the pre-activations run from GELU's curved region (a
    few units) to 64 and more, bias a non-negative integer that is 0 on the
    even columns. Every pre-activation is an exact non-negative integer and
    mag == v: the bound is u_b |t| but for the GELU term."""
    g = torch.Generator().manual_seed(3000 * seed + m + k + n)
    x = _randint(g, 0, 4, (m, k))
    x[::5] = 0
    dens = torch.linspace(1.0, 2.0 / k, n).view(n, 1)
    w = _randint(g, 0, 2, (n, k)) * (torch.rand(n, k, generator=g) < dens)
    bias = _randint(g, 0, 3, (n,))
    bias[::2] = 0
    v, mag = _float_fields(x.view(m, 1, 1, k), w.view(n, 1, 1, k), None,
                           bias, torch.zeros(m, 1, 1, n), 1, 0)
    assert torch.equal(v[0], mag[0]) and v[0].max() < 2 ** 24
    assert ((v[0] > 0) & (v[0] < 4)).any() and (v[0] >= 64).any()
    view = lambda t: (t[0].view(m, n),) * 2  # noqa: E731
    return _case(x=x.to(BF16), w=w.to(BF16), bias=bias, v=view(v),
                 mag=view(mag), K=k)


def truth(case, act, has_res=False):
    """The float64 value of act at the float64 pre-activation of a case."""
    v = case.v[bool(has_res)]
    if act == "none":
        return v
    if act == "relu":
        return v.clamp(min=0)
    if act == "relu6":
        return v.clamp(0, 6)
    if act == "hardswish":
        return v * (v + 3).clamp(0, 6) / 6
    if act == "gelu":
        return F.gelu(v)
    raise ValueError(f"act={act!r}")


def err_and_bound(case, act, has_res, got):
    """(|got - t|, the bound, t) per element, in float64."""
    t = truth(case, act, has_res)
    got = got.detach().cpu()
    assert got.dtype == BF16 and got.shape == t.shape, (got.dtype, got.shape)
    bound = U_B * t.abs() + SLOPE[act] * (case.K + 7) * U * case.mag[
        bool(has_res)]
    if act == "gelu":
        bound = bound + 4 * GELU_E0
    return (got.double() - t).abs(), bound, t


def check_bound(case, act, has_res, got, what="conv"):
    """Assert |got - t| <= u_b |t| + L (K + 7) u mag (+ 4 GELU_E0 for act
    "gelu") on every element; returns the worst err / bound."""
    err, bound, t = err_and_bound(case, act, has_res, got)
    got = got.detach().cpu()
    bad = ~(err <= bound)                      # a NaN is over the bound
    if bad.any():
        cout = t.shape[-1]
        row, col = bad.reshape(-1, cout).nonzero()[0].tolist()
        i = (row, col)
        raise AssertionError(
            f"{what} {act} res={bool(has_res)}: {int(bad.sum())} of "
            f"{t.numel()} elements over the bound, worst err / bound "
            f"{(err / bound).max().item():.3f}, first at (row, column) {i}: "
            f"got {got.reshape(-1, cout)[i].item()!r}, truth "
            f"{t.reshape(-1, cout)[i].item()!r}, err "
            f"{err.reshape(-1, cout)[i].item():.3e} > bound "
            f"{bound.reshape(-1, cout)[i].item():.3e}")
    ok = bound > 0
    return (err[ok] / bound[ok]).max().item() if ok.any() else 0.0


# ---------------------------------------------- rows behind a forced variant
# Rows that only a DEFER_CONV_VARIANT reaches, by its letter: (row, x shape
# NHWC, Cout, R, stride, pad), the smallest shapes that plan them
# (tests/data/conv_plans.json lists workload shapes that do). tools/
# convrowscheck.py runs them in a process of their own, since the variable
# is latched at first use. The legacy 128x128 STEM row needs a stem K = R *
# TR >= 1024 and 384 m-tiles: 7x7 on 22 channels is 7 * 160.
FORCED_CASES = {
    "l": [
        ("igemm: AMODE_GEMM, true, 128, 64, 3, 3, 2",
         (1, 120, 409, 64), 64, 1, 1, 0),
        ("igemm: AMODE_CONV, true, 128, 64, 3, 3, 2",
         (1, 239, 817, 64), 64, 1, 2, 0),
        ("igemm: AMODE_GEMM, true, 64, 64, 3, 3, 2",
         (1, 30, 33, 64), 64, 1, 1, 0),
        ("igemm: AMODE_CONV, true, 64, 64, 3, 3, 2",
         (1, 59, 65, 64), 64, 1, 2, 0),
        ("igemm: AMODE_STEM, false, 128, 128, 2, 2, 2",
         (1, 222, 221, 22), 128, 7, 1, 3),
    ],
    "w": [
        ("win: 64, 4, 256, 2", (3, 28, 28, 128), 128, 3, 1, 1),
    ],
}
# the two legacy rows of gelu_rows, as (row, M, K, N) of ops.linear_gelu
FORCED_GELU = {
    "l": [
        ("igemm: AMODE_GEMM, true, 128, 64, 3, 3, 2", 49080, 64, 64),
        ("igemm: AMODE_GEMM, true, 64, 64, 3, 3, 2", 990, 64, 64),
    ],
    "w": [],
}
