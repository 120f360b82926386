"""The layout kernels (csrc/layout.hip) and lowered torch models on the
GPU. CPU counterparts and the nets: test_lower_torch.py, torch_nets.py."""

import pytest
import torch
import torch.nn as nn

import torch_nets as T
from defer_amd import ops
from defer_amd.graph import GraphModel, LayerGraph
from defer_amd.lower import lower_torch
from defer_amd.parallel.pipeline import StageExecutor
from test_ops_gpu import _relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TV_SHAPE = (2, 3, 32, 32)
VGG_SHAPE = (2, 3, 8, 8)

# (N, C, H, W); the tile is 64 x 64, vectors are 4 fp32 / 8 bf16, and
# C <= 8 takes the per-pixel kernel
LAYOUT_CASES = [
    (1, 1, 1, 1),
    (2, 3, 5, 7),
    (2, 1, 16, 16),
    (3, 8, 4, 4),       # the last C of the per-pixel kernel
    (1, 9, 3, 3),       # the first C of the tile kernel
    (2, 67, 3, 11),     # C and HW off every vector and tile edge
    (1, 64, 8, 8),      # exactly one tile, 16-byte accesses on both sides
    (2, 130, 9, 9),     # two tiles and a tail in both dims
    (1, 72, 4, 12),     # 16-byte accesses with a partial tile in both dims
    (1, 5, 1, 300),     # long row, tiny C
    (1, 256, 1, 1),
    (2, 12, 2, 4),      # fp32 vectors (C % 4, HW % 4) where bf16 has none
]
_DT = (torch.float32, torch.bfloat16)

_SPECIALS = [
    0.0, -0.0, float("inf"), float("-inf"), float("nan"),
    1e-40, -1e-40, 1.4e-45,                 # fp32 denormals
    1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,   # ties: to even down / up
    -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -23,   # just above a tie
    3.4e38, -3.4e38,                        # rounds to inf in bf16
    2.0 ** -126, 2.0 ** -133,               # smallest normal, bf16 denormal
]


def _layout_input(shape, dtype):
    gen = torch.Generator().manual_seed(sum(shape) * 31 + shape[1])
    x = torch.randn(*shape, generator=gen)
    flat = x.view(-1)
    # specials in the first and the last elements (first and last tile)
    sp = torch.tensor(_SPECIALS)
    k = min(len(sp), flat.numel())
    flat[:k] = sp[:k]
    if flat.numel() >= 2 * len(sp):
        flat[-len(sp):] = sp
    return x.to(dtype)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _assert_same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan])


# ---------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("dst", _DT, ids=["to_f32", "to_bf16"])
@pytest.mark.parametrize("src", _DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", LAYOUT_CASES,
                         ids=["x".join(map(str, s)) for s in LAYOUT_CASES])
def test_layout_kernels_bit_exact(shape, src, dst):
    x = _layout_input(shape, src)
    N, C, H, W = shape
    for op, xin, perm in ((ops.to_nhwc, x, (0, 2, 3, 1)),
                          (ops.to_nchw,
                           x.permute(0, 2, 3, 1).contiguous(),
                           (0, 3, 1, 2))):
        want = xin.permute(*perm).contiguous().to(dst)      # on the CPU
        xg = xin.to(DEV)
        got = op(xg, dst)
        assert got.is_contiguous() and got.data_ptr() != xg.data_ptr()
        _assert_same_bits(got, want)
        # into a view of a longer buffer: the 64 elements after it stay
        sentinel = 12345.0
        buf = torch.full((want.numel() + 64,), sentinel, dtype=dst,
                         device=DEV)
        view = buf[:want.numel()].view(want.shape)
        assert op(xg, dst, out=view).data_ptr() == buf.data_ptr()
        _assert_same_bits(view, want)
        assert (buf[want.numel():] == sentinel).all()
    # dtype=None keeps the dtype
    assert ops.to_nhwc(x.to(DEV)).dtype == src


def test_layout_ops_reject_on_the_gpu():
    x = torch.randn(2, 4, 3, 3, device=DEV)
    for op in (ops.to_nhwc, ops.to_nchw):
        with pytest.raises(RuntimeError, match="contiguous"):
            op(x.permute(0, 2, 3, 1))
        with pytest.raises(RuntimeError, match="bf16 or fp32"):
            op(x.half())
        with pytest.raises(RuntimeError, match="4-D"):
            op(x[0])
    assert ops.to_nhwc(torch.empty(0, 3, 4, 4, device=DEV)).shape == (
        0, 4, 4, 3)


# ------------------------------------------- 2. exact integers, fp32 GPU
def _logits_graph(graph):
    """The graph without a trailing Softmax (its exp is not integer
    arithmetic; it is compared at a tolerance instead)."""
    if type(graph.nodes[-1].layer).__name__ != "Softmax":
        return graph
    return LayerGraph(graph.nodes[:-1])


@pytest.mark.parametrize("cls,shape", [(T.TVBlock, TV_SHAPE),
                                       (T.VGGHead, VGG_SHAPE)])
def test_exact_integers_fp32_gpu(cls, shape):
    """Integer sums below 2^24 are order-independent (the convention of
    test_ops_fp32_gpu.py): the lowered graph on the GPU in fp32 EQUALS the
    torch model on the CPU."""
    net = T.integerize(cls().eval())
    x = T.int_input(shape)
    with torch.no_grad():
        want = net(x)
        logits_net = net if cls is T.TVBlock else nn.Sequential(
            net.features, net.flatten, net.classifier)
        want_logits = logits_net(x)
    g = lower_torch(net, shape)
    ex = StageExecutor(GraphModel(_logits_graph(g)), DEV, torch.float32)
    got = ex.run(x.to(DEV)).cpu()
    assert got.dtype == torch.float32
    assert torch.equal(got, want_logits)
    if cls is T.VGGHead:
        ex = StageExecutor(GraphModel(lower_torch(net, shape)), DEV,
                           torch.float32)
        probs = ex.run(x.to(DEV)).cpu()
        assert torch.allclose(probs, want, atol=1e-6)


# ------------------------------------------------------------------ 3. bf16
def _round_weights_to_bf16(graph):
    for n in graph.nodes:
        for p in getattr(n.layer, "parameters", lambda: [])():
            if p.dim() >= 2:
                p.data = p.data.bfloat16().float()
    return graph


def test_tv_block_bf16_gpu_vs_cpu_reference():
    gen = torch.Generator().manual_seed(7)
    torch.manual_seed(7)
    net = T.randomize_bn(T.TVBlock().eval(), gen)
    x = torch.randn(*TV_SHAPE, generator=gen).bfloat16()
    cpu = _round_weights_to_bf16(lower_torch(net, TV_SHAPE))
    gpu = lower_torch(net, TV_SHAPE)
    with torch.no_grad():
        want_conv = cpu.split(["relu"])[0].forward(x.float())
        want = cpu.forward(x.float())
    # first conv: the stage [input__nhwc, relu]
    ex = StageExecutor(GraphModel(gpu.split(["relu"])[0]), DEV,
                       torch.bfloat16)
    got_conv = ex.run(x.to(DEV))
    assert got_conv.dtype == torch.bfloat16
    assert got_conv.shape == (2, 32, 32, 16)
    e = _relerr(got_conv, want_conv)
    print(f"first conv rel err {e:.5f}")
    assert e < 0.005, f"first conv rel err {e}"
    ex = StageExecutor(GraphModel(lower_torch(net, TV_SHAPE)), DEV,
                       torch.bfloat16)
    got = ex.run(x.to(DEV)).float().cpu()
    cos = torch.nn.functional.cosine_similarity(got, want, dim=-1)
    print(f"logits cosine {cos}")
    assert (cos > 0.98).all(), f"cosine {cos}"


def test_island_net_runs_in_bf16():
    """StageExecutor leaves the grouped nn.Conv2d with a bf16 weight and an
    fp32 bias; TorchIsland makes that harmless."""
    shape = (2, 3, 16, 16)
    gen = torch.Generator().manual_seed(9)
    torch.manual_seed(9)
    net = T.IslandNet().eval()
    x = torch.randn(*shape, generator=gen)
    with torch.no_grad():
        want = net(x)
    ex = StageExecutor(GraphModel(lower_torch(net, shape)), DEV,
                       torch.bfloat16)
    got = ex.run(x.to(DEV, torch.bfloat16))
    assert got.dtype == torch.bfloat16 and got.shape == want.shape
    cos = torch.nn.functional.cosine_similarity(got.float().cpu(), want,
                                                dim=-1)
    assert (cos > 0.98).all(), f"cosine {cos}"


@pytest.mark.parametrize("dtype", _DT, ids=["f32", "bf16"])
def test_twelve_channel_conv_and_island_pool_on_the_gpu(dtype):
    """Lowering admits what the bindings admit: a conv with Cout % 4 == 0
    that is no multiple of 8 (the bf16 kernel's scalar store tail), here
    with the max-pool it feeds kept as torch code between a to_nchw and a
    to_nhwc of a 12-channel tensor."""
    shape = (2, 3, 16, 16)
    gen = torch.Generator().manual_seed(21)
    torch.manual_seed(21)
    net = T.TwelveNet().eval()
    x = torch.randn(*shape, generator=gen)
    with torch.no_grad():
        want = net(x)
    ex = StageExecutor(GraphModel(lower_torch(net, shape)), DEV, dtype)
    got = ex.run(x.to(DEV, dtype))
    assert got.dtype == dtype and got.shape == want.shape
    got = got.float().cpu()
    if dtype == torch.float32:
        # first-order worst case of the chain: summation lengths 27 + 108
        # (convs) + 64 (mean) + 8 (fc) = 207, plus the epilogue roundings,
        # in units of u = 2^-24: 256 u of the largest logit
        e = _relerr(got, want)
        print(f"fp32 rel err {e:.3e}")
        assert e < 256 * 2.0 ** -24
    else:
        cos = torch.nn.functional.cosine_similarity(got, want, dim=-1)
        assert (cos > 0.98).all(), f"cosine {cos}"


# ---------------------------------------------------- 4. passes and graphs
def test_fusion_passes_and_hip_graph_do_not_change_fp32_logits():
    net = T.integerize(T.TVBlock().eval())
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(*TV_SHAPE, generator=gen).to(DEV)
    outs = {}
    for key, kw in (("fused", dict(fuse=True)),
                    ("plain", dict(fuse=False)),
                    ("graph", dict(fuse=True, use_graph=True))):
        ex = StageExecutor(GraphModel(lower_torch(net, TV_SHAPE)), DEV,
                           torch.float32, **kw)
        outs[key] = ex.run(x).clone()
        if key == "graph":
            assert ex.use_graph and ex._graph is not None   # captured
            outs["replay"] = ex.run(x).clone()
    assert torch.equal(outs["fused"], outs["plain"])
    assert torch.equal(outs["graph"], outs["fused"])
    assert torch.equal(outs["replay"], outs["fused"])
    # the passes found the zoo's structure in the lowered graph: both adds
    # went into their conv3, and block1's add, projection and block2's
    # conv1 into one chained node
    from defer_amd.parallel.fusion import (ChainedExpandReduceProj,
                                           FusedConvAddAct)

    ex = StageExecutor(GraphModel(lower_torch(net, TV_SHAPE)), DEV,
                       torch.float32)
    kinds = [type(n.layer) for n in ex.model.graph.nodes]
    assert kinds.count(ChainedExpandReduceProj) == 1
    assert kinds.count(FusedConvAddAct) == 1
