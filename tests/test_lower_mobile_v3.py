"""Lowering a torchvision-style MobileNetV3 (mobile_nets_v3.py) onto the
NHWC layers, on the CPU: the squeeze-excite chain in its spellings, the
hardswish spellings, in place and not. The same graphs run the HIP kernels
in test_se_gpu.py."""

import pytest
import torch
import torch.nn as nn

import mobile_nets_v3 as M3
import torch_nets as T
from defer_amd.graph import GraphModel, LayerGraph
from defer_amd.lower import lower_torch, lowering_report
from defer_amd.models import layers as L

MB_SHAPE = (2, 3, 32, 32)
SMALL_SHAPE = (2, 3, 16, 16)
INT_SEED = 0                # of integerize_v3 / int_input_v3


def _kept(graph):
    return [(n, r) for n, r in lowering_report(graph) if r != "lowered"]


def _types(graph):
    return {n.name: type(n.layer) for n in graph.nodes}


def node_values(graph, x):
    """{node name: value} of one forward pass of a LayerGraph."""
    env = {LayerGraph.INPUT: x}
    with torch.no_grad():
        for n in graph.nodes:
            env[n.name] = n.layer(*[env[p] for p in n.inputs], **n.kwargs)
    del env[LayerGraph.INPUT]
    return env


def _act_args(graph, vals, x):
    """{node name: the argument of its activation} for every node with a
    hardswish: the same layer run with act "none"."""
    env = dict(vals, **{LayerGraph.INPUT: x})
    out = {}
    for n in graph.nodes:
        lay = n.layer
        if type(lay) is L.Hardswish:
            out[n.name] = env[n.inputs[0]]
        elif getattr(lay, "act", None) == "hardswish":
            lay.act = "none"
            with torch.no_grad():
                out[n.name] = lay(*[env[p] for p in n.inputs])
            lay.act = "hardswish"
    return out


def _gate_args(graph, vals):
    """{node name: w2 @ relu(w1 @ mean(x) + b1) + b2 in double}"""
    out = {}
    for n in graph.nodes:
        lay = n.layer
        if type(lay) is L.SqueezeExcite:
            x = vals[n.inputs[0]].double()
            z = (x.mean(dim=(1, 2)) @ lay.w1.double().t()
                 + lay.b1.double()).clamp(min=0)
            out[n.name] = (z @ lay.w2.double().t() + lay.b2.double()).detach()
    return out


def exact_int_net():
    """(net, x, lowered graph, torch output): TinyMobileNetV3 with the
    integer parameters and input of mobile_nets_v3. Asserts the premise the
    exact comparisons rest on:
      - every hardswish argument is <= -3, 0 or >= 3, where hardswish is v
        or 0 exactly, and both regions and the 0 occur;
      - every gate argument is a multiple of 3, so every gate is exactly 0,
        0.5 or 1, and all three occur in both squeeze-excites;
      - every 4-D value is a multiple of 1/2 with |v| <= 256, so it is exact
        in bf16 (8 significant bits) as well as in fp32, in any summation
        order; the values after the pool are multiples of 1/64 below
        2^24 / 64 (exact in fp32, not in bf16)."""
    net = M3.integerize_v3(M3.TinyMobileNetV3().eval(), seed=INT_SEED)
    x = M3.int_input_v3(MB_SHAPE, seed=INT_SEED)
    g = lower_torch(net, MB_SHAPE, strict=True)
    with torch.no_grad():
        want = net(x)
    vals = node_values(g, x)
    args = _act_args(g, vals, x)
    assert len(args) == 1 + 2 + 2 + 1 + 1       # stem, 2 blocks, last, head
    low = high = zero = False
    for name, a in args.items():
        a = a.double()
        assert ((a <= -3) | (a == 0) | (a >= 3)).all(), name
        low, high = low or (a <= -3).any(), high or (a >= 3).any()
        zero = zero or (a == 0).any()
    assert low and high and zero
    gates = _gate_args(g, vals)
    assert len(gates) == 2
    for name, a in gates.items():
        assert torch.equal(a, (a / 3).round() * 3), name
        gate = (a + 3).clamp(0, 6) / 6
        assert set(gate.unique().tolist()) == {0.0, 0.5, 1.0}, name
    for n in g.nodes:
        v = vals[n.name].double()
        if v.dim() == 4:
            assert torch.equal(v * 2, (v * 2).round()), n.name
            assert v.abs().max() <= 256, (n.name, v.abs().max().item())
        else:
            k = v * 64
            assert torch.equal(k, k.round()), n.name
            assert k.abs().max() < 2 ** 24
    return net, x, g, want


# ------------------------------------------------------------ whole model
def test_tiny_mobilenet_v3_lowers_completely():
    net = M3.TinyMobileNetV3().eval()
    g = lower_torch(net, MB_SHAPE, strict=True)
    assert _kept(g) == []
    gm = GraphModel(g)
    assert not [m for m in gm.modules()
                if isinstance(m, (nn.Conv2d, nn.BatchNorm2d, nn.Linear,
                                  nn.Hardswish, nn.Hardsigmoid,
                                  nn.AdaptiveAvgPool2d, L.TorchIsland))]
    ty = _types(g)
    assert [n for n, t in ty.items() if t is L.ToNHWC] == ["input__nhwc"]
    assert L.ToNCHW not in ty.values()
    kinds = list(ty.values())
    ses = [n.layer for n in g.nodes if type(n.layer) is L.SqueezeExcite]
    assert [(s.c, s.cr) for s in ses] == list(M3.SE_BLOCKS)
    assert all((s.act, s.gate) == ("relu", "hardsigmoid") for s in ses)
    assert all(s.w1.shape == (s.cr, s.c) and s.w2.shape == (s.c, s.cr)
               and s.b1.shape == (s.cr,) and s.b2.shape == (s.c,)
               for s in ses)
    # stem; block 1 expand, project; block 2 expand, project; block 3
    # expand, project; the last 1x1
    convs = [n.layer for n in g.nodes if type(n.layer) is L.ConvBNAct]
    assert [c.act for c in convs] == ["hardswish", "relu", "none",
                                      "hardswish", "none", "hardswish",
                                      "none", "hardswish"]
    dws = [n.layer for n in g.nodes if type(n.layer) is L.DepthwiseConvBNAct]
    assert [(d.c, d.kernel, d.stride, d.act) for d in dws] == [
        (16, 5, 2, "relu"), (32, 3, 1, "hardswish"), (24, 3, 1, "hardswish")]
    # a squeeze-excite sits between its depthwise and its project conv
    names = [n.name for n in g.nodes]
    for n in g.nodes:
        if type(n.layer) is L.SqueezeExcite:
            i = names.index(n.name)
            assert type(g.nodes[i - 1].layer) is L.DepthwiseConvBNAct
            assert n.inputs == [names[i - 1]]
            assert g.nodes[i + 1].inputs == [n.name]
    assert kinds.count(L.AddAct) == 2
    # every in-place hardswish fused into its conv: the only one that
    # stands alone follows the Linear, which has no hardswish epilogue
    hs = [n for n in g.nodes if type(n.layer) is L.Hardswish]
    assert len(hs) == 1
    assert type(g.by_name[hs[0].inputs[0]].layer) is L.Dense
    assert L.Relu not in kinds and L.Relu6 not in kinds
    assert kinds.count(L.GlobalAvgPool) == 1 and kinds.count(L.Dense) == 2
    assert len(g.nodes) == 1 + 8 + 3 + 2 + 2 + 1 + 2 + 1


def test_tiny_mobilenet_v3_exact_integers():
    """Integer parameters and input (exact_int_net asserts the premise): the
    lowered graph EQUALS the torch model in double. A wrong [Cout, Cin, 1, 1]
    -> [Cout, Cin] reshape, a swapped w1 / w2, a hardswish taken for a ReLU
    or a gate off by a rounding fails here."""
    net, x, g, want = exact_int_net()
    with torch.no_grad():
        want64 = T.as_double(net)(x.double())
        got = g.forward(x)
    assert torch.equal(want.double(), want64)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got.double(), want64)
    assert (got != 0).float().mean() >= 0.5


def test_tiny_mobilenet_v3_random_floats():
    gen = torch.Generator().manual_seed(3)
    torch.manual_seed(3)
    net = T.randomize_bn(M3.TinyMobileNetV3().eval(), gen)
    x = torch.randn(*MB_SHAPE, generator=gen)
    with torch.no_grad():
        ref = T.as_double(net)(x.double())
        got = lower_torch(net, MB_SHAPE).forward(x)
    err = ((got.double() - ref).abs().max() / ref.abs().max()).item()
    print(f"lowered fp32 vs float64 torch: rel err {err:.3e}")
    # the criterion of test_tiny_mobilenet_random_floats
    assert err < 2.0 ** -16


# --------------------------------------------------------------- hardswish
@pytest.mark.parametrize("depthwise", [False, True], ids=["conv", "dw"])
@pytest.mark.parametrize("bn", [False, True], ids=["nobn", "bn"])
@pytest.mark.parametrize("how", M3.HARDSWISH_SPELLINGS)
def test_hardswish_spelling_fuses_into_conv(how, bn, depthwise):
    net = M3.HardswishNet(how, depthwise=depthwise, bn=bn).eval()
    g = lower_torch(net, SMALL_SHAPE, strict=True)
    kind = L.DepthwiseConvBNAct if depthwise else L.ConvBNAct
    assert [n.layer.act for n in g.nodes if type(n.layer) is kind] == [
        "hardswish"]
    assert L.Hardswish not in _types(g).values()
    x = torch.randn(*SMALL_SHAPE) * 4
    with torch.no_grad():
        assert torch.allclose(g.forward(x), net(x), atol=1e-5)


@pytest.mark.parametrize("how", M3.HARDSWISH_SPELLINGS)
def test_hardswish_spelling_standalone(how):
    net = M3.HardswishNet(how, after_pool=True).eval()
    g = lower_torch(net, SMALL_SHAPE, strict=True)
    ty = _types(g)
    assert list(ty.values()).count(L.Hardswish) == 1
    assert [n.layer.act for n in g.nodes
            if type(n.layer) is L.ConvBNAct] == ["none"]
    x = torch.randn(*SMALL_SHAPE) * 4
    with torch.no_grad():
        assert torch.allclose(g.forward(x), net(x), atol=1e-5)


def test_standalone_hardswish_follows_relu6s_numel_rule():
    net = M3.HardswishNet("module", after_pool=True).eval()
    g = lower_torch(net, (1, 3, 2, 2))      # pooled: 1 x 8 x 1 x 1, legal
    assert _kept(g) == []

    class Odd(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv2d(3, 4, 3, padding=1)
            self.pool = nn.MaxPool2d(3)
            self.act = nn.Hardswish()

        def forward(self, x):
            return self.act(self.pool(self.conv(x)))

    g = lower_torch(Odd().eval(), (1, 3, 3, 3))
    kept = dict(_kept(g))
    assert kept["act"] == ("Hardswish of 4 elements: hardswish needs "
                           "numel % 8 == 0")
    with pytest.raises(ValueError, match="hardswish needs"):
        lower_torch(Odd().eval(), (1, 3, 3, 3), strict=True)


def test_inplace_hardswish_rebinds_its_input():
    """torch writes an in-place Hardswish into its input: `x + act(x)` is
    2 * hardswish(x), not x + hardswish(x)."""
    net = M3.InplaceHardswishShared().eval()
    g = lower_torch(net, SMALL_SHAPE, strict=True)
    x = torch.randn(*SMALL_SHAPE) * 4
    with torch.no_grad():
        want = net(x)
        assert torch.allclose(g.forward(x), want, atol=1e-5)
    add = next(n for n in g.nodes if type(n.layer) is L.AddAct)
    assert add.inputs[0] == add.inputs[1]


# ---------------------------------------------------------- squeeze-excite
SE_SPELLINGS = [dict(pool=p, mul=m, act=a, gate=g, bias=b)
                for p, m, a, g, b in (
    ("module", "scale_first", "relu", "module", True),
    ("functional", "x_first", "relu_inplace", "functional", True),
    ("mean", "torch", "none", "module", False),
    ("module", "method", "relu", "functional", False),
    ("mean", "x_first", "relu", "module", True),
    ("functional", "scale_first", "none", "functional", True))]


@pytest.mark.parametrize("kw", SE_SPELLINGS,
                         ids=["-".join(map(str, k.values()))
                              for k in SE_SPELLINGS])
def test_squeeze_excite_spelling_lowers(kw):
    torch.manual_seed(1)
    net = M3.SeNet(c=16, cr=4, **kw).eval()
    g = lower_torch(net, SMALL_SHAPE, strict=True)
    ses = [n.layer for n in g.nodes if type(n.layer) is L.SqueezeExcite]
    assert len(ses) == 1
    se = ses[0]
    assert (se.c, se.cr, se.gate) == (16, 4, "hardsigmoid")
    assert se.act == ("none" if kw["act"] == "none" else "relu")
    assert torch.equal(se.w1, net.fc1.weight.view(4, 16))
    assert torch.equal(se.w2, net.fc2.weight.view(16, 4))
    if kw["bias"]:
        assert torch.equal(se.b1, net.fc1.bias)
        assert torch.equal(se.b2, net.fc2.bias)
    else:
        assert not se.b1.any() and not se.b2.any()
    ty = _types(g)
    assert L.ToNCHW not in ty.values()
    assert list(ty.values()).count(L.ConvBNAct) == 1      # fc1, fc2 are gone
    x = torch.randn(*SMALL_SHAPE) * 2
    with torch.no_grad():
        assert torch.allclose(g.forward(x), net(x), atol=1e-5)


@pytest.mark.parametrize("kw,why", [
    (dict(gate="sigmoid"), "gate sigmoid"),
    (dict(act="silu"), "SiLU after its first conv"),
    (dict(c=12, cr=4), "C=12: squeeze_excite needs C % 8 == 0"),
    (dict(c=8, cr=8, reuse="pooled"), "read by more than the next node"),
    (dict(reuse="hidden"), "read by more than the next node"),
    (dict(c=8, cr=8, reuse="gate"), "read by more than the next node"),
], ids=["sigmoid", "silu", "c12", "pooled", "hidden", "gate"])
def test_squeeze_excite_non_matches_stay_islands(kw, why):
    torch.manual_seed(2)
    net = M3.SeNet(**kw).eval()
    g = lower_torch(net, SMALL_SHAPE)
    assert L.SqueezeExcite not in _types(g).values()
    kept = _kept(g)
    reasons = [r for _, r in kept if r.startswith("squeeze-excite")]
    assert len(reasons) == 1 and why in reasons[0], kept
    # the pooling node carries the reason, the multiply stays torch code
    assert any(r.startswith("no lowering for mul") for _, r in kept)
    with pytest.raises(ValueError, match="squeeze-excite"):
        lower_torch(net, SMALL_SHAPE, strict=True)
    x = torch.randn(*SMALL_SHAPE) * 2
    with torch.no_grad():
        assert torch.allclose(g.forward(x), net(x), atol=1e-5)


def test_global_pool_into_flatten_is_still_a_global_avg_pool():
    """A pool to 1x1 that no 1x1 conv reads is not a squeeze-excite."""
    net = M3.TinyMobileNetV3().eval()
    g = lower_torch(net, MB_SHAPE, strict=True)
    assert list(_types(g).values()).count(L.GlobalAvgPool) == 1


def test_pooled_conv_branch_without_a_multiply_is_no_squeeze_excite():
    """An image-pooling branch (pool to 1x1, 1x1 conv, nothing multiplied
    with the pooled value) keeps the reason it had before squeeze-excite
    was lowered; the report does not call it one."""

    class PoolBranch(nn.Module):
        def __init__(self):
            super().__init__()
            self.c1 = nn.Conv2d(3, 8, 3, padding=1)
            self.pool = nn.AdaptiveAvgPool2d(1)
            self.fc1 = nn.Conv2d(8, 8, 1)
            self.fc = nn.Linear(8, 8)

        def forward(self, x):
            v = torch.relu(self.c1(x))
            b = torch.relu(self.fc1(self.pool(v)))
            return self.fc((v + b).mean(dim=(2, 3)))

    net = PoolBranch().eval()
    g = lower_torch(net, SMALL_SHAPE)
    kept = dict(_kept(g))
    assert not any("squeeze-excite" in r for r in kept.values()), kept
    assert kept["pool"] == ("AdaptiveAvgPool2d(1) that is not followed by a "
                            "flatten")
    x = torch.randn(*SMALL_SHAPE)
    with torch.no_grad():
        assert torch.allclose(g.forward(x), net(x), atol=1e-5)
