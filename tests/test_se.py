"""Squeeze-excite, hardswish and MobileNetV3-Large on the CPU: the reference
ops, the act and gate name checks of defer_amd.ops, the layers, the model,
the partitioner and the fusion passes. The HIP kernels: test_se_gpu.py."""

import functools
import queue
import threading

import pytest
import torch
import torch.nn.functional as F

import se_checks
from defer_amd import DEFER, PipelineConfig, ops
from defer_amd.models import MODELS, mobilenet_v3_large
from defer_amd.models import layers as L
from defer_amd.models.mobilenet import make_divisible
from defer_amd.ops import reference as ref
from defer_amd.parallel import fusion
from defer_amd.parallel.partitioner import auto_partition, node_times

# (expanded channels, squeeze channels) of the 8 squeeze-excite blocks
SE_PAIRS = [(72, 24), (120, 32), (120, 32), (480, 120), (672, 168),
            (672, 168), (960, 240), (960, 240)]
IDENTITY_BLOCKS = (0, 2, 4, 5, 7, 8, 9, 11, 13, 14)
HS_BLOCKS = tuple(range(6, 15))


# ----------------------------------------------------------- reference ops
def se_inputs(shape, cr, seed, bias=True):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) + 0.5
    w1 = torch.randn(cr, c, generator=g) * (2.0 / c) ** 0.5
    w2 = torch.randn(c, cr, generator=g) * 3 * (1.0 / cr) ** 0.5
    b1 = torch.randn(cr, generator=g) * 0.5 if bias else None
    b2 = torch.randn(c, generator=g) if bias else None
    return x, w1, b1, w2, b2


@pytest.mark.parametrize("act", ["relu", "none"])
@pytest.mark.parametrize("shape,cr", [((2, 7, 7, 72), 24), ((1, 1, 1, 8), 8),
                                      ((3, 5, 3, 40), 6), ((2, 4, 4, 16), 1)])
def test_reference_squeeze_excite_against_float64(shape, cr, act):
    for bias in (True, False):
        x, w1, b1, w2, b2 = se_inputs(shape, cr, sum(shape) + cr, bias)
        got = ref.squeeze_excite(x, w1, b1, w2, b2, act)
        worst = se_checks.check_squeeze_excite(x, w1, b1, w2, b2, act, got)
        print(f"reference {shape}/{cr} {act} bias={bias}: worst err/bound "
              f"{worst:.3f}")
        assert torch.equal(ops.squeeze_excite(x, w1, b1, w2, b2, act), got)
        # with b2 the gate varies whatever z is, or the case shows little
        g = se_checks.truth64(x, w1, b1, w2, b2, act)[2]
        assert not bias or g.max() - g.min() > 0.3
    xb = x.bfloat16()
    yb = ref.squeeze_excite(xb, w1.bfloat16(), b1, w2.bfloat16(), b2, act)
    assert yb.dtype == torch.bfloat16
    se_checks.check_squeeze_excite(xb, w1.bfloat16(), b1, w2.bfloat16(), b2,
                                   act, yb)


def test_checker_rejects_a_gate_rounded_to_bf16():
    x, w1, b1, w2, b2 = se_inputs((2, 7, 7, 72), 24, 3)
    g = se_checks.truth64(x, w1, b1, w2, b2, "relu")[2]
    bad = (x.double() * g.bfloat16().double()[:, None, None, :]).float()
    with pytest.raises(AssertionError, match="over the bound"):
        se_checks.check_squeeze_excite(x, w1, b1, w2, b2, "relu", bad)


def test_hardswish_is_exact_outside_the_ramp():
    x = torch.tensor([-100.0, -3.015625, -3.0, -0.0, 0.0, 3.0, 6.5, 100.0,
                      1e30, 2.984375])
    want = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 3.0, 6.5, 100.0, 1e30])
    for fn in (ref.hardswish, ops.hardswish, L.Hardswish()):
        y = fn(x)
        assert torch.equal(y[:9], want)
        assert 2.96 < y[9] < 2.984375           # on the ramp, below x
    assert ops.hardswish(x.bfloat16()).dtype == torch.bfloat16
    # the order of the spec, not torch's x * relu6(x + 3) / 6
    c6 = torch.tensor(1.0) / 6
    v = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 4
    assert torch.equal(ref.hardswish(v), v * ((v + 3).clamp(0, 6) * c6))
    assert torch.allclose(ref.hardswish(v), F.hardswish(v), atol=1e-6)
    # through the convs: identity 1x1 conv and depthwise centre tap
    x4 = x[:8].view(1, 1, 1, 8)
    y = ops.conv2d_bn_act(x4, torch.eye(8).view(8, 1, 1, 8), None, None, 1,
                          0, "hardswish")
    assert torch.equal(y.view(-1), want[:8])
    w = torch.zeros(3, 3, 8)
    w[1, 1] = 1
    y = ops.dwconv2d_bn_act(x4, w, None, None, 1, 1, "hardswish")
    assert torch.equal(y.view(-1), want[:8])


def test_squeeze_excite_gate_is_exactly_0_half_and_1():
    x = torch.ones(1, 2, 2, 8)
    w1 = torch.eye(8)
    w2 = torch.zeros(8, 8)
    b2 = torch.tensor([-9.0, -3.0, 0.0, 3.0, 9.0, -1.5, 1.5, 0.0])
    y = ops.squeeze_excite(x, w1, None, w2, b2)
    assert torch.equal(y[0, 0, 0],
                       torch.tensor([0, 0, .5, 1, 1, .25, .75, .5]))


# ------------------------------------------------------- names that raise
def _act_calls():
    x = torch.randn(1, 4, 4, 8)
    w1 = torch.randn(8, 1, 1, 8)
    v = torch.ones(8)
    m = torch.randn(8, 8)
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
        "squeeze_excite": lambda a: ops.squeeze_excite(x, m, v, m, v, a),
        "Dense": lambda a: L.Dense(8, 8, act=a),
        "SqueezeExcite": lambda a: L.SqueezeExcite(8, 8, act=a),
        "BNAct": lambda a: L.BNAct(8, a)(x),
        "AddAct": lambda a: L.AddAct(a)(x, x),
    }


HARDSWISH_OPS = ("conv2d_bn_act", "dwconv2d_bn_act")


@pytest.mark.parametrize("name", sorted(_act_calls()))
def test_unknown_act_raises(name):
    call = _act_calls()[name]
    with pytest.raises(ValueError, match="gelu"):
        call("gelu")
    call("relu")
    call("none")
    if name in HARDSWISH_OPS:
        call("hardswish")
    else:
        with pytest.raises(ValueError, match="hardswish"):
            call("hardswish")
        with pytest.raises(ValueError, match="relu6"):
            call("relu6")


def test_unknown_gate_raises():
    x, m, v = torch.randn(1, 4, 4, 8), torch.randn(8, 8), torch.ones(8)
    for gate in ("sigmoid", "hardswish", "none", None):
        with pytest.raises(ValueError, match="gate"):
            ops.squeeze_excite(x, m, v, m, v, "relu", gate)
        with pytest.raises(ValueError, match="gate"):
            ref.squeeze_excite(x, m, v, m, v, "relu", gate)
        with pytest.raises(ValueError, match="gate"):
            L.SqueezeExcite(8, 8, gate=gate)
    ops.squeeze_excite(x, m, v, m, v, "relu", "hardsigmoid")


def test_squeeze_excite_refusals_on_the_cpu():
    x = torch.randn(2, 4, 4, 8)
    w1, w2 = torch.randn(4, 8), torch.randn(8, 4)
    b1, b2 = torch.zeros(4), torch.zeros(8)
    call = ops.squeeze_excite
    call(x, w1, b1, w2, b2)
    call(x, w1, None, w2, None)
    with pytest.raises(RuntimeError, match="NHWC"):
        call(x[0], w1, b1, w2, b2)
    with pytest.raises(RuntimeError, match="contiguous"):
        call(x.permute(0, 2, 1, 3), w1, b1, w2, b2)
    with pytest.raises(RuntimeError, match="contiguous"):
        call(x, w2.t(), b1, w2, b2)
    with pytest.raises(RuntimeError, match="mixed dtypes"):
        call(x, w1.bfloat16(), b1, w2, b2)
    with pytest.raises(RuntimeError, match="mixed dtypes"):
        call(x.bfloat16(), w1.bfloat16(), b1, w2, b2)
    with pytest.raises(RuntimeError, match=r"w1 must be \[Cr, C\]"):
        call(x, torch.randn(4, 16), b1, w2, b2)
    with pytest.raises(RuntimeError, match=r"w2 must be \[C, Cr\]"):
        call(x, w1, b1, w1, b2)
    with pytest.raises(RuntimeError, match="b1 must be"):
        call(x, w1, b2, w2, b2)
    with pytest.raises(RuntimeError, match="b2 must be"):
        call(x, w1, b1, w2, b2.bfloat16())
    with pytest.raises(RuntimeError, match="b1 must be"):
        call(x, w1, b1.double(), w2, b2)
    with pytest.raises(RuntimeError, match="empty spatial extent"):
        call(x[:, :0], w1, b1, w2, b2)
    assert call(x[:0], w1, b1, w2, b2).shape == (0, 4, 4, 8)


# ------------------------------------------------------------------ layers
def test_layers():
    torch.manual_seed(0)
    se = L.SqueezeExcite(16, 8)
    assert (se.act, se.gate) == ("relu", "hardsigmoid")
    assert se.w1.shape == (8, 16) and se.w2.shape == (16, 8)
    assert se.b1.shape == (8,) and se.b2.shape == (16,)
    assert "squeeze_excite=16->8->16 act=relu gate=hardsigmoid" in repr(se)
    assert se.flops_per_image() == 2 * 2 * 16 * 8
    x = torch.randn(2, 5, 5, 16)
    with torch.no_grad():
        assert torch.equal(se(x), ref.squeeze_excite(
            x, se.w1, se.b1, se.w2, se.b2, "relu"))
    c = L.ConvBNAct(16, 8, 1, act="hardswish")
    assert "act=hardswish" in repr(c)
    with torch.no_grad():
        assert torch.equal(c(x), ref.hardswish(
            ref.conv2d_bn_act(x, c.weight, c.scale, c.bias, 1, 0)))
    d = L.DepthwiseConvBNAct(16, 5, 2, act="hardswish")
    with torch.no_grad():
        assert torch.equal(d(x), ref.hardswish(
            ref.dwconv2d_bn_act(x, d.weight, d.scale, d.bias, 2, 2)))


# --------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def _mbv3():
    torch.manual_seed(0)
    m = mobilenet_v3_large()
    x = torch.randn(2, 96, 96, 3, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        y = m(x)
    return m, x, y


def _p(k):
    return "expanded_conv" if k == 0 else f"expanded_conv_{k}"


def test_make_divisible():
    assert [make_divisible(e / 4) for e, _ in SE_PAIRS] == [
        cr for _, cr in SE_PAIRS]
    assert make_divisible(4) == 8 and make_divisible(11) == 16


def test_mobilenet_v3_large_shape_and_parameters():
    m, x, y = _mbv3()
    assert MODELS["mobilenetv3large"] is mobilenet_v3_large
    assert sum(p.numel() for p in m.parameters()) == 5483032
    assert y.shape == (2, 1000)
    assert torch.allclose(y.sum(-1), torch.ones(2), atol=1e-5)
    names = [n.name for n in m.graph.nodes]
    assert names[:3] == ["Conv", "expanded_conv_depthwise",
                         "expanded_conv_project"]
    assert "expanded_conv_expand" not in names
    assert names[-6:] == ["Conv_1", "global_average_pooling2d", "Conv_2",
                          "Conv_2_hard_swish", "predictions", "softmax"]
    by = m.graph.by_name
    for k in range(1, 15):
        for part in ("expand", "depthwise", "project"):
            assert f"{_p(k)}_{part}" in names
    assert [n for n in names if n.endswith("_add")] == [
        f"{_p(k)}_add" for k in IDENTITY_BLOCKS]
    ses = [n for n in m.graph.nodes if isinstance(n.layer, L.SqueezeExcite)]
    assert [n.name for n in ses] == [
        f"{_p(k)}_squeeze_excite" for k in (3, 4, 5, 10, 11, 12, 13, 14)]
    assert [(n.layer.c, n.layer.cr) for n in ses] == SE_PAIRS
    assert all(n.inputs == [n.name.replace("squeeze_excite", "depthwise")]
               and (n.layer.act, n.layer.gate) == ("relu", "hardsigmoid")
               for n in ses)
    dws = [n.layer for n in m.graph.nodes
           if isinstance(n.layer, L.DepthwiseConvBNAct)]
    assert [d.kernel for d in dws] == [3, 3, 3, 5, 5, 5, 3, 3, 3, 3, 3, 3,
                                       5, 5, 5]
    assert [d.act for d in dws] == ["relu"] * 6 + ["hardswish"] * 9
    assert [d.stride for d in dws] == [1, 2, 1, 2, 1, 1, 2, 1, 1, 1, 1, 1,
                                       2, 1, 1]
    for k in range(1, 15):
        want = "hardswish" if k in HS_BLOCKS else "relu"
        assert by[f"{_p(k)}_expand"].layer.act == want
        assert by[f"{_p(k)}_project"].layer.act == "none"
    assert by["Conv"].layer.act == "hardswish" and by["Conv"].layer.stride == 2
    assert by["Conv_1"].layer.act == "hardswish"
    assert by["Conv_1"].layer.cout == 960
    assert type(by["Conv_2_hard_swish"].layer) is L.Hardswish
    assert (by["Conv_2"].layer.cin, by["Conv_2"].layer.cout) == (960, 1280)
    head = mobilenet_v3_large(num_classes=10, include_top=False)
    assert head.graph.output == "Conv_1"
    assert mobilenet_v3_large(num_classes=10).graph.by_name[
        "predictions"].layer.cout == 10


def test_mobilenet_v3_large_cut_points():
    """Every _add is a cut, and so is the _project of every block without an
    identity add (the skip tensor crosses the others). A squeeze-excite node
    has one input, so it adds no second live value."""
    m, _, _ = _mbv3()
    cuts = set(m.graph.valid_cut_points())
    for k in range(15):
        if k in IDENTITY_BLOCKS:
            assert f"{_p(k)}_add" in cuts
            assert f"{_p(k)}_project" not in cuts
        else:
            assert f"{_p(k)}_project" in cuts
    assert "expanded_conv_3_squeeze_excite" in cuts


def test_mobilenet_v3_large_auto_partition_and_cost_model():
    m, _, _ = _mbv3()
    for stages_n in (2, 4):
        cuts, stages = auto_partition(m, stages_n, input_shape=(1, 96, 96, 3))
        assert len(cuts) == stages_n - 1 and len(stages) == stages_n
        assert len(set(cuts)) == stages_n - 1
    flops, out_b, t_us = node_times(m.graph, (1, 96, 96, 3))
    # expanded_conv_3: 24x24x72 -> 5x5/s2 -> 12x12x72 -> squeeze-excite
    b = 12 * 12 * 72 * 2.0
    assert out_b["expanded_conv_3_squeeze_excite"] == b
    assert t_us["expanded_conv_3_squeeze_excite"] == pytest.approx(
        3 * b / 5.0e12 * 1e6)
    assert flops["expanded_conv_3_squeeze_excite"] == 4 * 72 * 24
    assert flops["expanded_conv_3_depthwise"] == 12 * 12 * 2 * 25 * 72


def test_mobilenet_v3_large_threaded_defer_two_cpu_stages():
    m, x, want = _mbv3()
    eng = DEFER(["cpu", "cpu"], config=PipelineConfig(device="cpu",
                                                      dtype="fp32"))
    in_q, out_q = queue.Queue(4), queue.Queue(4)
    t = threading.Thread(target=eng.run_defer,
                         args=(m, ["expanded_conv_6_project"], in_q, out_q))
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


def test_fusion_passes_leave_hardswish_convs_out_of_the_chain_kernels():
    assert "hardswish" not in fusion._CHAIN_ACTS
    m, x, want = _mbv3()
    g = _fused(m.graph)
    kinds = [type(n.layer) for n in g.nodes]
    assert fusion.FusedConvPool not in kinds
    # the relu blocks 2, 4 and 5 may chain (add -> relu expand): only the
    # hardswish convs must stay out
    for n in g.nodes:
        if issubclass(type(n.layer), fusion.ChainedExpandReduce):
            assert not any(f"_{k}_" in n.name + "_" for k in HS_BLOCKS), n.name
    assert kinds.count(L.SqueezeExcite) == 8
    with torch.no_grad():
        got = g.forward(x)
    assert torch.equal(got, want)


def test_fuse_passes_refuse_a_hardswish_conv():
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
    gh = graph("hardswish")
    fh = fusion.fuse_expand_reduce(fusion.fuse_residual_adds(gh))
    assert not any(type(n.layer) is fusion.ChainedExpandReduce
                   for n in fh.nodes)
    x = torch.randn(1, 4, 4, 8) * 8
    with torch.no_grad():
        assert torch.equal(fh.forward(x), gh.forward(x))
    # a hardswish stem conv in front of a max-pool stays two nodes
    nodes = [GraphNode("stem", L.ConvBNAct(3, 64, 7, 2, 3, "hardswish"),
                       ["input"]),
             GraphNode("pool", L.MaxPool(3, 2, 1), ["stem"])]
    gp = fusion.fuse_conv_pool(LayerGraph(nodes, output="pool"))
    assert fusion.FusedConvPool not in [type(n.layer) for n in gp.nodes]
