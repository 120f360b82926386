"""Every row of the conv dispatch table that the default policy reaches runs
and agrees with the CPU fp32 reference.

One case per implicit-GEMM tile config (BM, BN, DA, DB, WPS) crossed with
each (gather, B_PERSIST) combination the config keeps, and one TH 8 window
case; the four (act, res) pairs rotate over the cases. Each shape is the
smallest with several tiles and an M tail that plans its row: the 128x64
rows need ceil(M/128) * ceil(Cout/64) >= 384 and, for the gathers that
prefer small tiles, fewer than 768 64x64 tiles, which leaves M = 49080.
Rows left out are reached only under a forced DEFER_CONV_VARIANT: the
B_PERSIST rows at the 3,3 depths (legacy), the STEM gather on the 128x128
tile (legacy) and the TH 4 window (tools/wincheck.py).
"""

import pytest
import torch

import defer_amd.ops as ops
from defer_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAIRS = [("relu", False), ("relu", True), ("none", True), ("none", False)]

CASES = [
    # (row, x shape NHWC, Cout, R, stride, pad)
    ("igemm: AMODE_GEMM, true, 128, 64, 4, 2, 2", (1, 120, 409, 64), 64, 1, 1, 0),
    ("igemm: AMODE_CONV, true, 128, 64, 4, 2, 2", (1, 239, 817, 64), 64, 1, 2, 0),
    ("igemm: AMODE_GEMM, false, 128, 64, 3, 3, 2", (1, 120, 409, 128), 64, 1, 1, 0),
    ("igemm: AMODE_CONV, false, 128, 64, 3, 3, 2", (1, 100, 123, 72), 256, 3, 1, 1),
    ("igemm: AMODE_RSC, false, 128, 64, 3, 3, 2", (1, 120, 409, 128), 64, 3, 1, 1),
    ("igemm: AMODE_STEM, false, 128, 64, 3, 3, 2", (3, 80, 818, 3), 64, 7, 2, 3),
    ("igemm: AMODE_GEMM, false, 128, 128, 2, 2, 2", (1, 100, 122, 512), 512, 1, 1, 0),
    ("igemm: AMODE_CONV, false, 128, 128, 2, 2, 2", (1, 100, 122, 120), 512, 3, 1, 1),
    ("igemm: AMODE_RSC, false, 128, 128, 2, 2, 2", (1, 100, 122, 128), 512, 3, 1, 1),
    ("igemm: AMODE_GEMM, false, 64, 128, 3, 3, 2", (1, 90, 100, 512), 256, 1, 1, 0),
    ("igemm: AMODE_CONV, false, 64, 128, 3, 3, 2", (1, 90, 100, 120), 256, 3, 1, 1),
    ("igemm: AMODE_RSC, false, 64, 128, 3, 3, 2", (1, 90, 100, 128), 256, 3, 1, 1),
    ("igemm: AMODE_STEM, false, 64, 128, 3, 3, 2", (1, 90, 100, 36), 256, 7, 1, 3),
    ("igemm: AMODE_GEMM, true, 64, 64, 4, 2, 4", (1, 100, 123, 64), 256, 1, 1, 0),
    ("igemm: AMODE_CONV, true, 64, 64, 4, 2, 4", (1, 199, 245, 64), 256, 1, 2, 0),
    ("igemm: AMODE_GEMM, false, 64, 64, 3, 3, 3", (1, 100, 123, 128), 256, 1, 1, 0),
    ("igemm: AMODE_CONV, false, 64, 64, 3, 3, 3", (1, 100, 123, 8), 256, 3, 1, 1),
    ("igemm: AMODE_RSC, false, 64, 64, 3, 3, 3", (1, 100, 123, 64), 256, 3, 1, 1),
    ("igemm: AMODE_STEM, false, 64, 64, 3, 3, 3", (4, 224, 224, 3), 64, 7, 2, 3),
    ("igemm: AMODE_GEMM, true, 64, 64, 4, 2, 2", (1, 30, 33, 64), 64, 1, 1, 0),
    ("igemm: AMODE_CONV, true, 64, 64, 4, 2, 2", (1, 59, 65, 64), 64, 1, 2, 0),
    ("igemm: AMODE_GEMM, false, 64, 64, 3, 3, 2", (1, 30, 33, 128), 64, 1, 1, 0),
    ("igemm: AMODE_CONV, false, 64, 64, 3, 3, 2", (1, 30, 33, 72), 64, 3, 1, 1),
    ("igemm: AMODE_RSC, false, 64, 64, 3, 3, 2", (1, 59, 65, 64), 128, 3, 2, 1),
    ("igemm: AMODE_STEM, false, 64, 64, 3, 3, 2", (1, 60, 66, 3), 64, 7, 2, 3),
    ("win: 64, 8, 256, 2", (19, 56, 60, 128), 64, 3, 1, 1),
]


def planned_row(case, has_res):
    row, xs, cout, r, stride, pad = case
    plan = ops.conv_plan(xs, (cout, r, r, xs[3]), stride, pad, has_res)
    return f"{plan['family']}: {plan['template_args'].split(', ', 1)[1]}"


def _relerr(got, want):
    got = got.float().cpu()
    want = want.float().cpu()
    denom = want.abs().max().clamp(min=1e-6)
    return ((got - want).abs().max() / denom).item()


def test_cases_cover_the_default_rows():
    import defer_amd._hip_ops as hip

    left_out = {"igemm: AMODE_GEMM, true, 128, 64, 3, 3, 2",
                "igemm: AMODE_CONV, true, 128, 64, 3, 3, 2",
                "igemm: AMODE_GEMM, true, 64, 64, 3, 3, 2",
                "igemm: AMODE_CONV, true, 64, 64, 3, 3, 2",
                "igemm: AMODE_STEM, false, 128, 128, 2, 2, 2",
                "win: 64, 4, 256, 2"}
    rows = {r for r in hip.conv_table_rows() if not r.startswith("swin")}
    assert {c[0] for c in CASES} == rows - left_out


@pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
@pytest.mark.parametrize("i", range(len(CASES)),
                         ids=[c[0].replace(", ", "-").replace(": ", "-")
                              for c in CASES])
def test_dispatch_row_numerics(i):
    case = CASES[i]
    row, xs, cout, r, stride, pad = case
    act, has_res = PAIRS[i % 4]
    # the shape still plans the row it is here for
    assert planned_row(case, has_res) == row
    nb, h, w_, cin = xs
    oh = (h + 2 * pad - r) // stride + 1
    ow = (w_ + 2 * pad - r) // stride + 1
    assert nb * oh * ow * cout * 2 <= 16 << 20
    x = torch.randn(*xs).to(torch.bfloat16)
    w = (torch.randn(cout, r, r, cin) * (2.0 / (cin * r * r)) ** 0.5
         ).to(torch.bfloat16)
    scale = torch.rand(cout) + 0.5
    bias = torch.randn(cout) * 0.1
    res = torch.randn(nb, oh, ow, cout).to(torch.bfloat16) if has_res else None
    want = ref.conv2d_bn_act(x, w, scale, bias, stride, pad, act, res)
    got = ops.conv2d_bn_act(x.to(DEV), w.to(DEV), scale.to(DEV),
                            bias.to(DEV), stride=stride, padding=pad,
                            act=act, residual=res.to(DEV) if has_res else None)
    assert got.shape == want.shape
    e = _relerr(got, want)
    assert e < 0.005, f"conv rel err {e} for {row}"
