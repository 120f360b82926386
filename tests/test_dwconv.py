"""Depthwise convolution, ReLU6 and MobileNetV2 on the CPU: the reference
op, the act-name checks of defer_amd.ops, the model, the partitioner and
the fusion passes. The HIP kernels: test_dwconv_gpu.py."""

import functools
import queue
import threading

import pytest
import torch
import torch.nn.functional as F

from defer_amd import DEFER, PipelineConfig, ops
from defer_amd.graph import GraphModel
from defer_amd.models import MODELS, mobilenet_v2
from defer_amd.models import layers as L
from defer_amd.ops import reference as ref
from defer_amd.parallel import fusion
from defer_amd.parallel.partitioner import auto_partition, node_times

IDENTITY_BLOCKS = (2, 4, 5, 7, 8, 9, 11, 12, 14, 15)


# ------------------------------------------------------------ reference op
def _loop_dwconv64(x, w, scale, bias, stride, pad):
    """One F.conv2d per channel, in float64."""
    outs = []
    for c in range(x.shape[-1]):
        xc = x[..., c].double().unsqueeze(1)                # [N, 1, H, W]
        wc = w[..., c].double().view(1, 1, *w.shape[:2])
        y = F.conv2d(xc, wc, stride=stride, padding=pad)
        outs.append(y[:, 0] * scale[c].double() + bias[c].double())
    return torch.stack(outs, dim=-1)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("R", [3, 5])
def test_reference_matches_per_channel_loop(R, stride):
    gen = torch.Generator().manual_seed(R * 10 + stride)
    for pad in range(R // 2 + 1):
        x = torch.randn(2, 9, 12, 6, generator=gen)         # H != W
        w = torch.randn(R, R, 6, generator=gen)
        scale = torch.rand(6, generator=gen) + 0.5
        bias = torch.randn(6, generator=gen)
        want = _loop_dwconv64(x, w, scale, bias, stride, pad)
        got = ref.dwconv2d_bn_act(x, w, scale, bias, stride, pad, "none")
        assert got.dtype == torch.float32
        assert got.shape == want.shape == (
            2, (9 + 2 * pad - R) // stride + 1,
            (12 + 2 * pad - R) // stride + 1, 6)
        # fp32 against float64: (R*R + 2) roundings of values below
        # sum|x*w|*|scale| + |bias|
        mag = _loop_dwconv64(x.abs(), w.abs(), scale, bias.abs(), stride,
                             pad)
        assert ((got.double() - want).abs()
                <= (R * R + 2) * 2.0 ** -24 * mag).all()
        for act, fn in (("relu", torch.relu),
                        ("relu6", lambda t: t.clamp(0, 6))):
            y = ref.dwconv2d_bn_act(x, w, scale, bias, stride, pad, act)
            assert torch.equal(y, fn(got))
        # the op on the CPU is the reference
        assert torch.equal(
            ops.dwconv2d_bn_act(x, w, scale, bias, stride, pad, "none"), got)
    y = ref.dwconv2d_bn_act(x, w, None, None, stride, 1, "none")
    assert torch.equal(y, ref.dwconv2d_bn_act(
        x, w, torch.ones(6), torch.zeros(6), stride, 1, "none"))


def test_relu6_clamps_at_both_ends():
    x = torch.tensor([-3.0, -0.0, 0.0, 0.5, 5.999, 6.0, 6.001, 100.0])
    want = torch.tensor([0.0, 0.0, 0.0, 0.5, 5.999, 6.0, 6.0, 6.0])
    assert torch.equal(ref.relu6(x), want)
    assert torch.equal(ops.relu6(x), want)
    assert torch.equal(L.Relu6()(x), want)
    xb = x.bfloat16()
    assert ops.relu6(xb).dtype == torch.bfloat16
    # through the convs: identity 1x1 conv and depthwise centre tap
    x4 = x.view(1, 1, 1, 8)
    y = ops.conv2d_bn_act(x4, torch.eye(8).view(8, 1, 1, 8), None, None,
                          1, 0, "relu6")
    assert torch.equal(y.view(-1), want)
    w = torch.zeros(3, 3, 8)
    w[1, 1] = 1
    y = ops.dwconv2d_bn_act(x4, w, None, None, 1, 1, "relu6")
    assert torch.equal(y.view(-1), want)
    # after scale, bias and residual
    res = torch.full((1, 1, 1, 8), 4.0)
    y = ops.conv2d_bn_act(x4, torch.eye(8).view(8, 1, 1, 8),
                          torch.full((8,), 2.0), torch.ones(8), 1, 0,
                          "relu6", res)
    assert torch.equal(y.view(-1), (x * 2 + 1 + 4).clamp(0, 6))


# ------------------------------------------------------- act names raise
def _act_calls():
    x = torch.randn(1, 4, 4, 8)
    w1 = torch.randn(8, 1, 1, 8)
    v = torch.ones(8)
    return {
        "conv2d_bn_act": lambda a: ops.conv2d_bn_act(x, w1, v, v, 1, 0, a),
        "dwconv2d_bn_act": lambda a: ops.dwconv2d_bn_act(
            x, torch.randn(3, 3, 8), v, v, 1, 1, a),
        "batchnorm_apply": lambda a: ops.batchnorm_apply(x, v, v, a),
        "add_act": lambda a: ops.add_act(x, x, a),
        "conv1x1_chain.act3": lambda a: ops.conv1x1_chain(
            x, w1, v, v, x, a, w1, v, v, "relu"),
        "conv1x1_chain.act1": lambda a: ops.conv1x1_chain(
            x, w1, v, v, x, "relu", w1, v, v, a),
        "conv1x1_chain_proj.act3": lambda a: ops.conv1x1_chain_proj(
            x, w1, v, v, x, w1, v, v, a, w1, v, v, "relu"),
        "conv1x1_chain_proj.act1": lambda a: ops.conv1x1_chain_proj(
            x, w1, v, v, x, w1, v, v, "none", w1, v, v, a),
        "conv_bn_act_maxpool": lambda a: ops.conv_bn_act_maxpool(
            x, w1, v, v, 1, 0, a, 3, 2, 1),
    }


RELU6_OPS = ("conv2d_bn_act", "dwconv2d_bn_act")


@pytest.mark.parametrize("name", sorted(_act_calls()))
def test_unknown_act_raises(name):
    call = _act_calls()[name]
    with pytest.raises(ValueError, match="gelu"):
        call("gelu")
    call("relu")
    call("none")
    if name in RELU6_OPS:
        call("relu6")
    else:
        with pytest.raises(ValueError, match="relu6"):
            call("relu6")


def test_layers_with_relu6():
    torch.manual_seed(0)
    x = torch.randn(1, 6, 6, 8) * 4
    c = L.ConvBNAct(8, 16, 3, act="relu6")
    y = c(x)
    assert y.min() == 0 and y.max() == 6
    d = L.DepthwiseConvBNAct(8, stride=2)
    assert d.act == "relu6" and d.padding == 1 and d.weight.shape == (3, 3, 8)
    assert d(x).shape == (1, 3, 3, 8)
    assert d.flops_per_pixel() == 2 * 9 * 8
    assert "depthwise 8 k3 s2 p1 act=relu6" in repr(d)
    assert L.DepthwiseConvBNAct(8, 5).padding == 2
    assert L.DepthwiseConvBNAct(8, bn=False).scale is None


# --------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def _mbv2():
    torch.manual_seed(0)
    m = mobilenet_v2()
    x = torch.randn(2, 96, 96, 3, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        y = m(x)
    return m, x, y


def test_mobilenet_v2_shape_and_parameters():
    m, x, y = _mbv2()
    assert MODELS["mobilenetv2"] is mobilenet_v2
    assert sum(p.numel() for p in m.parameters()) == 3504872
    assert y.shape == (2, 1000)
    assert torch.allclose(y.sum(-1), torch.ones(2), atol=1e-5)
    names = [n.name for n in m.graph.nodes]
    assert names[:3] == ["Conv1", "expanded_conv_depthwise",
                         "expanded_conv_project"]
    assert names[-4:] == ["Conv_1", "global_average_pooling2d",
                          "predictions", "softmax"]
    for k in range(1, 17):
        for part in ("expand", "depthwise", "project"):
            assert f"block_{k}_{part}" in names
    assert [n for n in names if n.endswith("_add")] == [
        f"block_{k}_add" for k in IDENTITY_BLOCKS]
    by = m.graph.by_name
    assert all(by[f"block_{k}_add"].layer.act == "none"
               for k in IDENTITY_BLOCKS)
    dws = [n.layer for n in m.graph.nodes
           if isinstance(n.layer, L.DepthwiseConvBNAct)]
    assert len(dws) == 17 and all(d.act == "relu6" for d in dws)
    assert by["Conv1"].layer.act == "relu6" and by["Conv1"].layer.stride == 2
    assert by["Conv_1"].layer.act == "relu6" and by["Conv_1"].layer.cout == 1280
    head = mobilenet_v2(num_classes=10, include_top=False)
    assert head.graph.output == "Conv_1"


def test_mobilenet_v2_cut_points():
    """Every block_k_add is a cut, and so is the block_k_project of every
    block without an identity add. (The project conv of an identity block
    is not: the skip tensor crosses it, two values would be live.)"""
    m, _, _ = _mbv2()
    cuts = set(m.graph.valid_cut_points())
    for k in range(1, 17):
        if k in IDENTITY_BLOCKS:
            assert f"block_{k}_add" in cuts
            assert f"block_{k}_project" not in cuts
        else:
            assert f"block_{k}_project" in cuts
    assert "expanded_conv_project" in cuts


def test_mobilenet_v2_auto_partition_and_cost_model():
    m, _, _ = _mbv2()
    cuts, stages = auto_partition(m, 4, input_shape=(1, 96, 96, 3))
    assert len(cuts) == 3 and len(stages) == 4
    assert len(set(cuts)) == 3
    flops, out_b, t_us = node_times(m.graph, (1, 96, 96, 3))
    # block_1_depthwise: 48x48x96 in, stride 2, 24x24x96 out
    assert flops["block_1_depthwise"] == 24 * 24 * 2 * 9 * 96
    in_b, o_b = 48 * 48 * 96 * 2.0, 24 * 24 * 96 * 2.0
    assert out_b["block_1_depthwise"] == o_b
    assert t_us["block_1_depthwise"] == pytest.approx(
        (in_b + o_b) / 5.0e12 * 1e6)


def test_mobilenet_v2_threaded_defer_two_cpu_stages():
    m, x, want = _mbv2()
    eng = DEFER(["cpu", "cpu"], config=PipelineConfig(device="cpu",
                                                      dtype="fp32"))
    in_q, out_q = queue.Queue(4), queue.Queue(4)
    t = threading.Thread(target=eng.run_defer,
                         args=(m, ["block_6_project"], in_q, out_q))
    t.start()
    in_q.put(x)
    in_q.put(None)
    out = out_q.get(timeout=120)
    t.join(timeout=120)
    assert not t.is_alive()
    assert torch.equal(out, want)


# ------------------------------------------------------------ fusion passes
def _fused(graph):
    g = fusion.fuse_residual_adds(graph)
    g = fusion.fuse_chain_projection(fusion.fuse_expand_reduce(g))
    return fusion.fuse_conv_pool(g)


def test_fusion_passes_leave_relu6_convs_out_of_the_chain_kernels():
    m, x, want = _mbv2()
    g = _fused(m.graph)
    kinds = [type(n.layer) for n in g.nodes]
    assert not any(issubclass(k, fusion.ChainedExpandReduce) for k in kinds)
    assert fusion.FusedConvPool not in kinds
    assert kinds.count(fusion.FusedConvAddAct) == 10
    assert [n.name for n in g.nodes
            if type(n.layer) is fusion.FusedConvAddAct] == [
        f"block_{k}_add" for k in IDENTITY_BLOCKS]
    with torch.no_grad():
        got = g.forward(x)
    assert torch.equal(got, want)
    # one stage on its own, as StageExecutor fuses it
    stage = m.stage_models(["block_6_project"])[1]
    g1 = _fused(stage.graph)
    assert not any(issubclass(type(n.layer), fusion.ChainedExpandReduce)
                   for n in g1.nodes)
    xs = torch.randn(1, 6, 6, 64)
    with torch.no_grad():
        assert torch.equal(g1.forward(xs), stage(xs))


def test_fuse_expand_reduce_still_chains_relu_convs():
    """The guard is on the activation, not on the pass: the same shape of
    graph with ReLU convs chains, with a relu6 expand conv it does not."""
    from defer_amd.graph import GraphNode, LayerGraph

    def graph(act):
        nodes = [
            GraphNode("a", L.ConvBNAct(8, 8, 1, 1, 0, "relu"), ["input"]),
            GraphNode("c3", L.ConvBNAct(8, 16, 1, 1, 0, "none"), ["a"]),
            GraphNode("p", L.ConvBNAct(8, 16, 1, 1, 0, "none"), ["input"]),
            GraphNode("add", L.AddAct("none"), ["c3", "p"]),
            GraphNode("c1", L.ConvBNAct(16, 8, 1, 1, 0, act), ["add"])]
        return LayerGraph(nodes, output="c1")

    torch.manual_seed(0)
    g = fusion.fuse_expand_reduce(fusion.fuse_residual_adds(graph("relu")))
    assert any(type(n.layer) is fusion.ChainedExpandReduce for n in g.nodes)
    g6 = graph("relu6")
    f6 = fusion.fuse_expand_reduce(fusion.fuse_residual_adds(g6))
    assert not any(type(n.layer) is fusion.ChainedExpandReduce
                   for n in f6.nodes)
    x = torch.randn(1, 4, 4, 8) * 8
    with torch.no_grad():
        assert torch.equal(f6.forward(x), g6.forward(x))
        assert f6.forward(x).max() == 6
