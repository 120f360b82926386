"""The 128x128 implicit-GEMM tile (conv_igemm_kernel<..., 128, 128, 2, 2, 2>)
puts every output where it belongs and changes no bit.

The tile's four waves sit 2 x 2 (64 rows x 64 columns a wave) and read their
fragments one ks step ahead; every other tile stacks 32-row slabs. Each case
is checked two ways: against the CPU reference kept in fp32 at the project's
conv tolerance (0.5 %, profiles/numerics_envelope.txt), and with torch.equal
against the same conv cut along M into pieces small enough that plan_conv
gives each a 64-row tile (asserted). An output pixel depends on its own
image (3x3) or its own row (1x1) only, every tile walks K in the same order
with the same MFMA and the same epilogue expression, so the pieces put
together must equal the whole in every bit, the partial last m-tile and the
clamped columns included.

Shapes are the smallest that plan the tile: plan_conv asks for
ceil(M/128) * (Cout/128) >= 384 and K >= 1024 (or a 1x1 with K >= 512).
3x3, 128 -> 128 at 28x28 output: NB = 63, M = 49,392 = 385 * 128 + 112.
1x1, K = 512, Cout = 256: M >= 191 * 128 + 1 = 24,449 = 23 * 1063.
"""

import pytest
import torch

import defer_amd.ops as ops
from defer_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

CASES = {
    # name: (x shape NHWC, Cout, R, stride, pad, act, residual, piece)
    # piece: images (3x3) or image rows (1x1) per small-plan launch
    # 1. partial last m-tile
    "3x3s1_m_tail": ((63, 28, 28, 128), 128, 3, 1, 1, "relu", False, 8),
    # 2. the stride path of a_setup, same M
    "3x3s2_m_tail": ((63, 56, 56, 128), 128, 3, 2, 1, "relu", False, 8),
    # 3. GEMM mode with residual and ReLU, smallest M + 40 rows = 27 * 907
    "1x1_res_relu": ((1, 27, 907, 512), 256, 1, 1, 0, "relu", True, 8),
    # 4. second n-tile partial, Cout % 8 == 0: interior beside clamped columns
    "3x3_cout136": ((63, 28, 28, 128), 136, 3, 1, 1, "relu", True, 8),
    # 5. Cout % 8 != 0: every tile takes the non-interior stores
    "3x3_cout130": ((63, 28, 28, 128), 130, 3, 1, 1, "none", True, 8),
    # 6. the four (act, residual) pairs on the smallest 1x1 shape, whose last
    # m-tile holds one row
    "1x1_min_none": ((1, 23, 1063, 512), 256, 1, 1, 0, "none", False, 8),
    "1x1_min_relu": ((1, 23, 1063, 512), 256, 1, 1, 0, "relu", False, 8),
    "1x1_min_none_res": ((1, 23, 1063, 512), 256, 1, 1, 0, "none", True, 8),
    "1x1_min_relu_res": ((1, 23, 1063, 512), 256, 1, 1, 0, "relu", True, 8),
}


def _relerr(got, want):
    got = got.float().cpu()
    want = want.float().cpu()
    denom = want.abs().max().clamp(min=1e-6)
    return ((got - want).abs().max() / denom).item()


def _tile(xs, cout, r, stride, pad, has_res):
    plan = ops.conv_plan(xs, (cout, r, r, xs[3]), stride, pad, has_res)
    return plan["family"], plan["BM"], plan["BN"]


_inputs = {}


def _data(xs, cout, r):
    """Seeded inputs, one set per (x shape, Cout, R), shared and read-only."""
    key = (xs, cout, r)
    if key not in _inputs:
        g = torch.Generator().manual_seed(len(_inputs) + 1)
        cin = xs[3]
        x = torch.randn(*xs, generator=g).to(torch.bfloat16)
        w = (torch.randn(cout, r, r, cin, generator=g)
             * (2.0 / (cin * r * r)) ** 0.5).to(torch.bfloat16)
        scale = torch.rand(cout, generator=g) + 0.5
        bias = torch.randn(cout, generator=g) * 0.1
        _inputs[key] = (x, w, scale, bias)
    return _inputs[key]


@pytest.mark.parametrize("name", list(CASES))
def test_tile128_matches_reference_and_small_tile(name):
    xs, cout, r, stride, pad, act, has_res, piece = CASES[name]
    # the shape still plans the tile it is here for
    assert _tile(xs, cout, r, stride, pad, has_res) == ("igemm", 128, 128)
    nb, h, w_, cin = xs
    oh = (h + 2 * pad - r) // stride + 1
    ow = (w_ + 2 * pad - r) // stride + 1
    x, w, scale, bias = _data(xs, cout, r)
    res = None
    if has_res:
        g = torch.Generator().manual_seed(99)
        res = torch.randn(nb, oh, ow, cout, generator=g).to(torch.bfloat16)
    # the reference stays in fp32 (fp32 copies of the bf16 inputs, no final
    # rounding): the kernel's one bf16 rounding is then at most half an ulp,
    # 2^-8 = 0.39 % of the largest output, inside the bound for any data. Two
    # bf16-rounded results can differ by a whole ulp, 0.78 %.
    want = ref.conv2d_bn_act(x.float(), w.float(), scale, bias, stride, pad,
                             act, res.float() if has_res else None)
    assert want.dtype == torch.float32

    xd, wd, sd, bd = x.to(DEV), w.to(DEV), scale.to(DEV), bias.to(DEV)
    rd = res.to(DEV) if has_res else None
    got = ops.conv2d_bn_act(xd, wd, sd, bd, stride=stride, padding=pad,
                            act=act, residual=rd)
    assert got.shape == want.shape
    e = _relerr(got, want)
    print(f"{name}: rel err {e:.3e}")
    assert e < 0.005, f"conv rel err {e} for {name}"

    # the same conv in pieces along M, each on a 64-row tile: a 3x3 is cut
    # by image, a 1x1 by image row
    dim = 0 if r > 1 else 1
    n = xs[dim]
    parts = []
    for lo in range(0, n, piece):
        hi = min(lo + piece, n)
        xp = xd.narrow(dim, lo, hi - lo).contiguous()
        rp = rd.narrow(dim, lo, hi - lo).contiguous() if has_res else None
        fam, bm, _ = _tile(tuple(xp.shape), cout, r, stride, pad, has_res)
        assert fam == "igemm" and bm == 64, (fam, bm)
        parts.append(ops.conv2d_bn_act(xp, wd, sd, bd, stride=stride,
                                       padding=pad, act=act, residual=rp))
    small = torch.cat(parts, dim=dim)
    assert small.shape == got.shape
    if not torch.equal(got, small):
        bad = (got != small).reshape(-1, cout).nonzero()
        raise AssertionError(
            f"{name}: {bad.shape[0]} outputs differ from the 64-row tile, "
            f"first (row, column) {bad[0].tolist()}")
