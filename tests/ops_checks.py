"""Per-element checkers for the pooling, elementwise, concat and softmax ops
(a helper module like torch_nets.py, not collected as tests).

Each `check_<op>(inputs..., got)` takes the op's inputs and its output, on
any device, and asserts a bound on every element against a float64 truth
computed from the same (already rounded) inputs. It returns the worst
observed error over its bound (0.0 for the exact ops), so a caller can
print or record it; the assertion never depends on that figure.

u = 2^-24 is the roundoff of one fp32 operation and u_b = 2^-8 the worst
relative error of one round-to-nearest to bf16 (8 significant bits). For
fp32 tensors the u_b term is dropped. No bound here comes from a
measurement:

* relu, relu6, maxpool2d, concat_channels, add_act: `torch.equal` to
  `defer_amd.ops.reference`, and equal `isinf` masks. Selections and copies
  are exact; add_act is one IEEE fp32 add, one max and one rounding on both
  sides. `torch.equal` compares with ==, so the sign of a zero is not
  pinned. NaN inputs are outside the contract (docs/TESTING.md).
* batchnorm_apply: |got - t| <= u_b*|t| + 3u*A, A = |x*scale| + |bias|, t
  after the activation (1-Lipschitz, so the bound carries over). Unfused,
  the product carries u*|x*scale| and the sum u*(|x*scale| + |bias|)(1 + u);
  fused, one u*A. 3u*A covers either times the (1 + u_b) of the rounding.
* avgpool2d: |got - t| <= u_b*|t| + (k^2 + 2)u*mean|taps|, both means over
  the valid taps (count_include_pad=False): at most k^2 - 1 adds, one
  reciprocal (or division) and one product.
* global_avg_pool: |got - t| <= u_b*|t| + (HW + 2)u*mean|x|, likewise.
* softmax: per-element relative error <= u_b + (cols + 2R + 16)u with R the
  row's logit range: the sum of cols terms, 2R for the argument of the
  exponential (x - m scaled by log2(e) in fp32 has an absolute error of up
  to R*u, which is a relative error of the result) and 16 for the
  subtraction, two exponentials, the reciprocal and the product. A logit of
  -inf has probability exactly 0. Rows sum to 1 within u_b + cols*u. The
  caller keeps R + ln(cols) below 87 so that no fp32 probability is a
  denormal, where a relative bound means nothing.
"""

import math

import torch
import torch.nn.functional as F

from defer_amd.ops import reference as ref

U = 2.0 ** -24
U_B = 2.0 ** -8

# lanes of the largest grid the 1-D kernels launch (2048 blocks x 256): a
# launch with more lanes of work than this iterates its grid-stride loop
GRID_CAP_LANES = 2048 * 256


def lanes(numel, dtype):
    """Lanes of work of an elementwise launch over `numel` elements: one
    16-byte vector per lane."""
    per = 8 if dtype == torch.bfloat16 else 4
    assert numel % per == 0
    return numel // per


def _ub(t):
    assert t.dtype in (torch.bfloat16, torch.float32), t.dtype
    return U_B if t.dtype == torch.bfloat16 else 0.0


def _cpu(t):
    return t.detach().cpu()


def _same_kind(got, like, shape):
    assert got.dtype == like.dtype, (got.dtype, like.dtype)
    assert tuple(got.shape) == tuple(shape), (tuple(got.shape), tuple(shape))


def _check_equal(got, want, what):
    got, want = _cpu(got), _cpu(want)
    _same_kind(got, want, want.shape)
    assert torch.equal(torch.isinf(got), torch.isinf(want)), \
        f"{what}: inf mask differs"
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(
            f"{what}: {len(bad)} of {got.numel()} elements differ, first at "
            f"{i}: got {got[i].item()!r}, want {want[i].item()!r}")
    return 0.0


def _check_bound(got, truth, bound, what):
    """|got - truth| <= bound on every element (float64 tensors); returns
    the worst err / bound."""
    got = got.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - truth).abs()
    ok = err <= bound
    if not ok.all():
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(
            f"{what}: {len(bad)} of {got.numel()} elements beyond the bound, "
            f"first at {i}: got {got[i].item()!r}, truth {truth[i].item()!r},"
            f" err {err[i].item():.3e} > bound {bound[i].item():.3e}")
    pos = bound > 0
    return (err[pos] / bound[pos]).max().item() if pos.any() else 0.0


def check_relu(x, got):
    return _check_equal(got, ref.relu(_cpu(x)), "relu")


def check_relu6(x, got):
    return _check_equal(got, ref.relu6(_cpu(x)), "relu6")


def check_add_act(a, b, act, got):
    return _check_equal(got, ref.add_act(_cpu(a), _cpu(b), act),
                        f"add_act({act})")


def check_maxpool2d(x, kernel, stride, pad, got):
    return _check_equal(got, ref.maxpool2d(_cpu(x), kernel, stride, pad),
                        f"maxpool2d({kernel}/{stride}/{pad})")


def check_concat_channels(xs, got):
    return _check_equal(got, ref.concat_channels([_cpu(t) for t in xs]),
                        "concat_channels")


def check_batchnorm_apply(x, scale, bias, act, got):
    x, got = _cpu(x), _cpu(got)
    _same_kind(got, x, x.shape)
    xs = x.double() * _cpu(scale).double()
    b = _cpu(bias).double()
    t = xs + b
    if act == "relu":
        t = torch.relu(t)
    else:
        assert act == "none", act
    bound = _ub(x) * t.abs() + 3 * U * (xs.abs() + b.abs())
    return _check_bound(got, t, bound, f"batchnorm_apply({act})")


def _avg64(x, kernel, stride, pad):
    y = F.avg_pool2d(x.permute(0, 3, 1, 2), kernel, stride, pad,
                     count_include_pad=False)
    return y.permute(0, 2, 3, 1)


def check_avgpool2d(x, kernel, stride, pad, got):
    x, got = _cpu(x), _cpu(got)
    xd = x.double()
    t = _avg64(xd, kernel, stride, pad)
    mean_abs = _avg64(xd.abs(), kernel, stride, pad)
    _same_kind(got, x, t.shape)
    bound = _ub(x) * t.abs() + (kernel * kernel + 2) * U * mean_abs
    return _check_bound(got, t, bound,
                        f"avgpool2d({kernel}/{stride}/{pad})")


def check_global_avg_pool(x, got):
    x, got = _cpu(x), _cpu(got)
    n, h, w, c = x.shape
    xd = x.double()
    t = xd.mean(dim=(1, 2))
    mean_abs = xd.abs().mean(dim=(1, 2))
    _same_kind(got, x, (n, c))
    bound = _ub(x) * t.abs() + (h * w + 2) * U * mean_abs
    return _check_bound(got, t, bound, "global_avg_pool")


def check_softmax(x, got):
    """Returns (worst per-element ratio, worst row-sum ratio)."""
    x, got = _cpu(x), _cpu(got)
    _same_kind(got, x, x.shape)
    cols = x.shape[-1]
    xd = x.double().reshape(-1, cols)
    gd = got.double().reshape(-1, cols)
    finite = torch.isfinite(xd)
    assert (finite | (xd == -math.inf)).all(), "softmax input: +inf or NaN"
    assert finite.any(dim=-1).all(), "softmax input: a row of -inf only"
    hi = xd.max(dim=-1, keepdim=True).values
    lo = torch.where(finite, xd, hi).min(dim=-1, keepdim=True).values
    R = hi - lo
    assert (R + math.log(cols) < 87).all(), \
        "softmax input: a probability would be an fp32 denormal"
    t = F.softmax(xd, dim=-1)
    assert torch.isfinite(gd).all(), "softmax: non-finite output"
    assert (gd[~finite] == 0).all(), "softmax: p(-inf) is not exactly 0"
    rel_bound = (_ub(x) + (cols + 2 * R + 16) * U).expand_as(t)
    rel = torch.where(finite, (gd - t).abs() / t, torch.zeros_like(t))
    ok = rel <= rel_bound
    if not ok.all():
        i = tuple((~ok).nonzero()[0].tolist())
        raise AssertionError(
            f"softmax: {int((~ok).sum())} of {t.numel()} elements beyond the "
            f"bound, first at {i}: got {gd[i].item()!r}, truth "
            f"{t[i].item()!r}, rel err {rel[i].item():.3e} > bound "
            f"{rel_bound[i].item():.3e}")
    sum_err = (gd.sum(dim=-1) - 1).abs()
    sum_bound = _ub(x) + cols * U
    assert (sum_err <= sum_bound).all(), \
        f"softmax: a row sums to 1 +- {sum_err.max().item():.3e} > " \
        f"{sum_bound:.3e}"
    return (rel / rel_bound).max().item(), (sum_err / sum_bound).max().item()


# ---- the small shapes and the data, shared by the CPU tests of the
# checkers (run on the reference) and the GPU tests (run on the kernels) ----

DTYPES = [torch.bfloat16, torch.float32]
DTYPE_IDS = ["bf16", "fp32"]

POOL_GEOMS = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 2, 0)]
# [1, 3, 3, 8]: every window touches a border; [3, 5, 6, 72]: 9 lanes a
# pixel, H != W, three images
POOL_SHAPES = [(2, 9, 11, 8), (1, 7, 7, 16), (1, 3, 3, 8), (3, 5, 6, 72)]
POOL_CASES = [(s, g) for s in POOL_SHAPES for g in POOL_GEOMS]
POOL_CASES.append(((1, 2, 2, 8), (2, 2, 0)))      # one output pixel
POOL_IDS = ["x".join(map(str, s)) + "-k%ds%dp%d" % g for s, g in POOL_CASES]

# bf16: one block covers 2048 channels, fp32 1024. 2056 / 1028: a second
# block with a single live lane; HW = 1; two full blocks
GAP_SHAPES = {
    torch.bfloat16: [(3, 7, 7, 2056), (1, 1, 1, 8), (2, 14, 14, 512),
                     (1, 3, 5, 4096)],
    torch.float32: [(3, 7, 7, 1028), (1, 1, 1, 4), (1, 3, 5, 2048)],
}

# (rows, cols, scale of the logits): cols < 64 leaves lanes without an
# element, 64 / 65 are the wave and one past it, rows % 4 != 0 leaves waves
# of the last block without a row
SOFTMAX_CASES = [(5, 1000, 4), (3, 1, 4), (7, 63, 4), (4, 64, 4), (9, 65, 8),
                 (2, 4096, 2), (1, 10, 15)]

BN_SHAPE = (2, 9, 11, 72)
ELEMENTWISE_SHAPES = [(8,), (2, 9, 11, 72)]

# two-input concat through the kernel: (rows shape, c1, c2)
CAT2_CASES = [((2, 7, 7), 8, 24), ((1, 5, 3), 256, 32), ((3, 2, 2), 32, 8),
              ((1,), 16, 8)]


def randn(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(dtype)


def relu6_data(shape, dtype, seed):
    """Values around both clamps, with exact 0 and 6 and their neighbours
    in `dtype` on both sides."""
    x = randn(shape, dtype, seed, 4.0).flatten()
    zero = torch.zeros((), dtype=dtype)
    six = torch.full((), 6.0, dtype=dtype)
    inf = torch.full((), math.inf, dtype=dtype)
    edge = torch.stack([
        zero, -zero, six,
        torch.nextafter(zero, inf), torch.nextafter(zero, -inf),
        torch.nextafter(six, inf), torch.nextafter(six, -inf), -six])
    x[:8] = edge
    return x.reshape(shape)


def maxpool_special(kind, dtype):
    """[2, 9, 11, 8] tensors for the running maximum's start value."""
    x = randn((2, 9, 11, 8), dtype, 7)
    if kind == "negative":          # zero padding would win every border
        return -(x.abs() + 0.5)
    if kind == "neg_inf_image":     # the true maximum is -inf
        x[0] = -math.inf
        return x
    assert kind == "huge_negative"  # every tap below -1e30
    x[1] = -3.0e38
    x[1, 2, 3, 1] = math.inf
    x[1, 6, 8, 2] = 0.0
    x[1, 4, 5, 3] = -1e30
    return x


MAXPOOL_SPECIALS = ["negative", "neg_inf_image", "huge_negative"]


def softmax_special(kind, dtype):
    if kind == "some_neg_inf":      # lanes and whole strides of -inf
        x = randn((2, 130), dtype, 11, 4.0)
        x[0, [0, 5, 64, 129]] = -math.inf
        x[1, 3:70] = -math.inf
        return x
    assert kind == "all_huge_negative"
    x = randn((3, 100), dtype, 12, 4.0)
    x[1] = -3.0e38                  # m = -3e38, every exp(0): uniform
    return x


SOFTMAX_SPECIALS = ["some_neg_inf", "all_huge_negative"]
