"""GPU: the chain kernel that makes the projection shortcut itself
(csrc/chain.hip, PROJ) against the projection launch plus conv1x1_chain it
replaces. Both outputs must match bit for bit: the shortcut is accumulated
and rounded as the projection launch does it, and added as the chain
kernel's residual is. The two paths give the same numbers by design, so
chain_proj_stats() tells which one ran."""

import itertools

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


def _inputs(N, H, W, N1, KP=64, K1=64, N2=64, affine=True):
    g = torch.Generator().manual_seed(4321 + N1 + KP + N * H * W)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = r(N, H, W, K1).to(DEV, torch.bfloat16)
    xp = r(N, H, W, KP).to(DEV, torch.bfloat16)
    w3 = (r(N1, 1, 1, K1) * (2.0 / K1) ** 0.5).to(DEV, torch.bfloat16)
    wp = (r(N1, 1, 1, KP) * (2.0 / KP) ** 0.5).to(DEV, torch.bfloat16)
    w1 = (r(N2, 1, 1, N1) * (2.0 / N1) ** 0.5).to(DEV, torch.bfloat16)
    if affine:
        s3 = (torch.rand(N1, generator=g) + 0.5).to(DEV)
        b3 = (r(N1) * 0.1).to(DEV)
        sp = (torch.rand(N1, generator=g) + 0.5).to(DEV)
        bp = (r(N1) * 0.1).to(DEV)
    else:
        s3 = b3 = sp = bp = None
    s1 = (torch.rand(N2, generator=g) + 0.5).to(DEV)
    b1 = (r(N2) * 0.1).to(DEV)
    return dict(x=x, w3=w3, s3=s3, b3=b3, xp=xp, wp=wp, sp=sp, bp=bp,
                w1=w1, s1=s1, b1=b1)


def _call(t, act3, act1, mode, max_blocks=0):
    return ops.conv1x1_chain_proj(
        t["x"], t["w3"], t["s3"], t["b3"], t["xp"], t["wp"], t["sp"],
        t["bp"], act3, t["w1"], t["s1"], t["b1"], act1, mode=mode,
        max_blocks=max_blocks)


def _launches():
    return ops.chain_proj_stats()["launches"]


def _check_bitwise(t, act3="relu", act1="relu", max_blocks=0, blocks=None):
    n0 = _launches()
    want_y, want_a2 = _call(t, act3, act1, 2)
    assert _launches() == n0, "mode=2 must not launch the kernel"
    y, a2 = _call(t, act3, act1, 1, max_blocks)
    st = ops.chain_proj_stats()
    assert st["launches"] == n0 + 1, "mode=1 must launch the kernel"
    if blocks is not None:
        assert st["blocks"] == blocks
    assert y.shape == want_y.shape and a2.shape == want_a2.shape
    assert torch.equal(y, want_y)
    assert torch.equal(a2, want_a2)
    # a second call gives the same bits
    y2, a22 = _call(t, act3, act1, 1, max_blocks)
    assert _launches() == n0 + 2
    assert torch.equal(y2, y) and torch.equal(a22, a2)
    return y, a2


BITWISE_CASES = [
    # (N, H, W), N1, max_blocks, grid expected
    ((1, 5, 7), 256, 0, 1),     # M = 35: a single partial tile
    ((2, 9, 9), 256, 1, 1),     # M = 162: one block walks 3 tiles, 34-row
    ((2, 9, 9), 256, 2, 2),     # tail; two blocks walk 2 + 1
    ((3, 8, 8), 64, 0, 3),      # NJ = 1: the chunk look-ahead wraps
    ((3, 8, 8), 128, 0, 3),
]


@pytest.mark.parametrize("case", BITWISE_CASES,
                         ids=[f"b{i}" for i in range(len(BITWISE_CASES))])
def test_proj_bitwise_equals_composed(case):
    (N, H, W), N1, max_blocks, blocks = case
    _check_bitwise(_inputs(N, H, W, N1), max_blocks=max_blocks,
                   blocks=blocks)


@pytest.mark.parametrize("act3,act1", list(itertools.product(
    ["relu", "none"], repeat=2)))
def test_proj_activations(act3, act1):
    _check_bitwise(_inputs(2, 9, 9, 256), act3, act1, max_blocks=2)


def test_proj_without_affines():
    # absent scale/bias: the ones/zeros substitution of every conv
    _check_bitwise(_inputs(1, 5, 7, 256, affine=False))


def test_proj_against_fp32_reference():
    t = _inputs(2, 9, 9, 256)
    y, a2 = _call(t, "relu", "relu", 1, 2)
    c = {k: (None if v is None else v.cpu()) for k, v in t.items()}
    res = ref.conv2d_bn_act(c["xp"], c["wp"], c["sp"], c["bp"], 1, 0,
                            "none", None)
    yr = ref.conv2d_bn_act(c["x"], c["w3"], c["s3"], c["b3"], 1, 0, "relu",
                           res)
    ar = ref.conv2d_bn_act(yr, c["w1"], c["s1"], c["b1"], 1, 0, "relu",
                           None)
    assert _relerr(y, yr) < 0.005
    assert _relerr(a2, ar) < 0.005


def test_unsupported_shape_composes():
    # KP = 128: no kernel serves it, mode=1 runs the two ops
    t = _inputs(2, 9, 9, 256, KP=128)
    n0 = _launches()
    y, a2 = _call(t, "relu", "relu", 1)
    assert _launches() == n0
    res = ops.conv2d_bn_act(t["xp"], t["wp"], t["sp"], t["bp"], stride=1,
                            padding=0, act="none")
    want_y, want_a2 = ops.conv1x1_chain(t["x"], t["w3"], t["s3"], t["b3"],
                                        res, "relu", t["w1"], t["s1"],
                                        t["b1"], "relu")
    assert torch.equal(y, want_y) and torch.equal(a2, want_a2)


def test_resnet50_logits_unchanged_by_proj(monkeypatch):
    from defer_amd.graph import GraphModel
    from defer_amd.models import resnet50
    from defer_amd.parallel.fusion import ChainedExpandReduceProj
    from defer_amd.parallel.pipeline import StageExecutor

    m = resnet50()
    x = torch.randn(2, 64, 64, 3).to(DEV, torch.bfloat16)
    monkeypatch.setattr(ops, "_CHAIN_PROJ_MODE", 2)
    ex = StageExecutor(GraphModel(m.graph), DEV, torch.bfloat16)
    assert sum(isinstance(n.layer, ChainedExpandReduceProj)
               for n in ex.model.graph.nodes) == 1
    n0 = _launches()
    with torch.no_grad():
        want = ex.run(x).clone()
    assert _launches() == n0
    monkeypatch.setattr(ops, "_CHAIN_PROJ_MODE", 1)
    with torch.no_grad():
        got = ex.run(x)
    torch.cuda.synchronize()
    assert _launches() == n0 + 1
    assert torch.equal(got, want)
