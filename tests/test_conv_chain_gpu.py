"""GPU: the chained expand->reduce kernel (csrc/chain.hip) against the two
conv2d_bn_act launches it replaces. Both outputs must match bit for bit:
the kernel accumulates in the same order with the same epilogue."""

import pytest
import torch

import defer_amd.ops as ops
from defer_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _relerr(got, want):
    got = got.float().cpu()
    want = want.float().cpu()
    denom = want.abs().max().clamp(min=1e-6)
    return ((got - want).abs().max() / denom).item()


def _inputs(N, H, W, K1, N1, N2, affine=True):
    g = torch.Generator().manual_seed(1234 + K1 + N1 + N2 + N * H * W)
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


BITWISE_CASES = [
    # (N, H, W), K1, N1, N2, act3, affine3, max_blocks
    ((1, 7, 7), 64, 256, 64, "relu", True, 0),      # M=49 < BM, one k-tile
    ((3, 9, 9), 64, 256, 128, "relu", True, 0),     # M=243 tail, L1->L2
    ((2, 14, 14), 128, 512, 128, "relu", True, 2),  # m-tiles/block, prefetch
    ((2, 8, 8), 128, 512, 256, "relu", True, 0),    # widest required acc2
    ((1, 8, 8), 64, 256, 64, "none", True, 0),      # no-ReLU epilogue
    ((1, 8, 8), 64, 256, 64, "relu", False, 0),     # ones/zeros substitution
    ((1, 9, 9), 256, 1024, 256, "relu", True, 0),   # layer3 class, M tail
    ((1, 9, 9), 256, 1024, 512, "relu", True, 1),   # layer3->4, 2 m-tiles
]


@pytest.mark.parametrize("case", BITWISE_CASES,
                         ids=[f"b{i}" for i in range(len(BITWISE_CASES))])
def test_chain_bitwise_equals_two_launches(case):
    (N, H, W), K1, N1, N2, act3, affine, max_blocks = case
    x, w3, s3, b3, res, w1, s1, b1 = _inputs(N, H, W, K1, N1, N2, affine)
    want_y, want_a2 = _two_launches(x, w3, s3, b3, res, act3, w1, s1, b1,
                                    "relu")
    y, a2 = ops.conv1x1_chain(x, w3, s3, b3, res, act3, w1, s1, b1, "relu",
                              mode=1, max_blocks=max_blocks)
    torch.cuda.synchronize()
    assert y.shape == want_y.shape and a2.shape == want_a2.shape
    assert torch.equal(y, want_y)
    assert torch.equal(a2, want_a2)
    # and the pair is the right function, not merely self-consistent
    yr = ref.conv2d_bn_act(x.cpu(), w3.cpu(),
                           None if s3 is None else s3.cpu(),
                           None if b3 is None else b3.cpu(), 1, 0, act3,
                           res.cpu())
    assert _relerr(y, yr) < 0.005


@pytest.mark.parametrize("K1,N2", [(96, 64), (64, 40)])
@pytest.mark.parametrize("mode", [0, 1])
def test_unsupported_shapes_fall_back(K1, N2, mode):
    x, w3, s3, b3, res, w1, s1, b1 = _inputs(2, 9, 9, K1, 256, N2)
    want_y, want_a2 = _two_launches(x, w3, s3, b3, res, "relu", w1, s1, b1,
                                    "relu")
    y, a2 = ops.conv1x1_chain(x, w3, s3, b3, res, "relu", w1, s1, b1,
                              "relu", mode=mode)
    assert torch.equal(y, want_y) and torch.equal(a2, want_a2)
    yr = ref.conv2d_bn_act(x.cpu(), w3.cpu(), s3.cpu(), b3.cpu(), 1, 0,
                           "relu", res.cpu())
    ar = ref.conv2d_bn_act(y.cpu(), w1.cpu(), s1.cpu(), b1.cpu(), 1, 0,
                           "relu", None)
    assert _relerr(y, yr) < 0.005
    assert _relerr(a2, ar) < 0.005


def test_mode2_equals_mode1():
    args = _inputs(3, 9, 9, 64, 256, 128)
    x, w3, s3, b3, res, w1, s1, b1 = args
    y1, a1 = ops.conv1x1_chain(x, w3, s3, b3, res, "relu", w1, s1, b1,
                               "relu", mode=1)
    y2, a2 = ops.conv1x1_chain(x, w3, s3, b3, res, "relu", w1, s1, b1,
                               "relu", mode=2)
    assert torch.equal(y1, y2) and torch.equal(a1, a2)


def test_resnet50_logits_unchanged_by_chain(monkeypatch):
    from defer_amd.graph import GraphModel
    from defer_amd.models import resnet50
    from defer_amd.parallel.fusion import ChainedExpandReduce
    from defer_amd.parallel.pipeline import StageExecutor

    m = resnet50()
    x = torch.randn(2, 64, 64, 3).to(DEV, torch.bfloat16)
    off = StageExecutor(GraphModel(m.graph), DEV, torch.bfloat16,
                        chain=False)
    with torch.no_grad():
        want = off.run(x).clone()
    # fused kernel wherever it is legal, whatever the policy table says
    monkeypatch.setattr(ops, "_CHAIN_MODE", 1)
    on = StageExecutor(GraphModel(m.graph), DEV, torch.bfloat16)
    assert sum(isinstance(n.layer, ChainedExpandReduce)
               for n in on.model.graph.nodes) == 15
    with torch.no_grad():
        got = on.run(x)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
