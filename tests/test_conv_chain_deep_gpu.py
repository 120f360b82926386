"""GPU: the 8-wave (two waves per SIMD) instantiations of the chained
expand->reduce kernel (csrc/chain.hip, K1 = 256) against the two
conv2d_bn_act launches they replace. Both outputs must match bit for bit;
y is also checked against the fp32 reference at the project's 0.5 %."""

import pytest
import torch

import defer_amd.ops as ops
from defer_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K1, N1 = 256, 1024


def _relerr(got, want):
    got = got.float().cpu()
    want = want.float().cpu()
    denom = want.abs().max().clamp(min=1e-6)
    return ((got - want).abs().max() / denom).item()


def _inputs(N, H, W, N2, affine=True):
    g = torch.Generator().manual_seed(4321 + N2 + N * H * W)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = r(N, H, W, K1).to(DEV, torch.bfloat16)
    res = r(N, H, W, N1).to(DEV, torch.bfloat16)
    w3 = (r(N1, 1, 1, K1) * (2.0 / K1) ** 0.5).to(DEV, torch.bfloat16)
    w1 = (r(N2, 1, 1, N1) * (2.0 / N1) ** 0.5).to(DEV, torch.bfloat16)
    if affine:
        s3 = (torch.rand(N1, generator=g) + 0.5).to(DEV)
        b3 = (r(N1) * 0.1).to(DEV)
    else:
        s3 = b3 = None
    s1 = (torch.rand(N2, generator=g) + 0.5).to(DEV)
    b1 = (r(N2) * 0.1).to(DEV)
    return x, w3, s3, b3, res, w1, s1, b1


def _two_launches(x, w3, s3, b3, res, act3, w1, s1, b1, act1):
    y = ops.conv2d_bn_act(x, w3, s3, b3, stride=1, padding=0, act=act3,
                          residual=res)
    a2 = ops.conv2d_bn_act(y, w1, s1, b1, stride=1, padding=0, act=act1)
    return y, a2


DEEP_CASES = [
    # (N, H, W), N2, act3, affine3, max_blocks
    ((1, 7, 7), 256, "relu", True, 0),     # M=49 < one tile: clamped rows
    ((1, 8, 8), 256, "relu", True, 0),     # M=64 exactly
    ((2, 14, 14), 256, "relu", True, 2),   # 7 tiles, 4 + 3, wraps, M tail
    ((2, 14, 14), 256, "relu", True, 1),   # every tile in one block
    ((1, 9, 9), 256, "none", True, 0),     # no-activation epilogue
    ((1, 9, 9), 256, "relu", False, 0),    # ones/zeros substitution
    ((1, 9, 9), 512, "relu", True, 1),     # layer3->4, 2 tiles in one block
]


@pytest.mark.parametrize("case", DEEP_CASES,
                         ids=[f"d{i}" for i in range(len(DEEP_CASES))])
def test_deep_chain_bitwise_equals_two_launches(case):
    (N, H, W), N2, act3, affine, max_blocks = case
    x, w3, s3, b3, res, w1, s1, b1 = _inputs(N, H, W, N2, affine)
    want_y, want_a2 = _two_launches(x, w3, s3, b3, res, act3, w1, s1, b1,
                                    "relu")
    y, a2 = ops.conv1x1_chain(x, w3, s3, b3, res, act3, w1, s1, b1, "relu",
                              mode=1, max_blocks=max_blocks)
    torch.cuda.synchronize()
    assert y.shape == want_y.shape and a2.shape == want_a2.shape
    assert torch.equal(y, want_y)
    assert torch.equal(a2, want_a2)
    yr = ref.conv2d_bn_act(x.cpu(), w3.cpu(),
                           None if s3 is None else s3.cpu(),
                           None if b3 is None else b3.cpu(), 1, 0, act3,
                           res.cpu())
    assert _relerr(y, yr) < 0.005


def test_balanced_grid_equals_two_launches():
    # M = 19182: 300 tiles, more than one round of the 256 blocks the
    # launcher may use, so it spreads them as 150 blocks x 2 tiles; the
    # last tile has 46 rows
    x, w3, s3, b3, res, w1, s1, b1 = _inputs(1, 138, 139, 256)
    want_y, want_a2 = _two_launches(x, w3, s3, b3, res, "relu", w1, s1, b1,
                                    "relu")
    y, a2 = ops.conv1x1_chain(x, w3, s3, b3, res, "relu", w1, s1, b1, "relu",
                              mode=1)
    assert torch.equal(y, want_y) and torch.equal(a2, want_a2)


def test_policy_mode_equals_two_launches():
    # 256-1024-256 is in the launcher's policy table: mode 0 runs the fused
    # kernel on its own grid (here 7 tiles, one per block)
    x, w3, s3, b3, res, w1, s1, b1 = _inputs(2, 14, 14, 256)
    y0, a0 = ops.conv1x1_chain(x, w3, s3, b3, res, "relu", w1, s1, b1,
                               "relu", mode=0)
    y2, a2 = ops.conv1x1_chain(x, w3, s3, b3, res, "relu", w1, s1, b1,
                               "relu", mode=2)
    assert torch.equal(y0, y2) and torch.equal(a0, a2)
