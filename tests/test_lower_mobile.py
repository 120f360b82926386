"""Lowering a torchvision-style MobileNetV2 (mobile_nets.py) onto the NHWC
layers, on the CPU: depthwise convs, the ReLU6 spellings, the functional
global pool. The same graphs run the HIP kernels in test_dwconv_gpu.py."""

import pytest
import torch
import torch.nn as nn

import mobile_nets as M
import torch_nets as T
from defer_amd.graph import GraphModel, LayerGraph
from defer_amd.lower import lower_torch, lowering_report
from defer_amd.models import layers as L

MB_SHAPE = (2, 3, 32, 32)
SMALL_SHAPE = (2, 3, 16, 16)
INT_SEED = 0                # of integerize / int_input, see exact_int_net


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


def exact_int_net():
    """(net, x, lowered graph, torch output): TinyMobileNetV2 with integer
    parameters and input. Asserts the premise the exact GPU comparisons
    rest on: every 4-D intermediate is an integer with |v| <= 256, so it
    is exact in bf16 (8 significant bits) as well as in fp32, in any
    summation order. The head is not: the mean over 8x8 positions of
    values up to 6 is k / 64 with k up to 384, which fp32 holds exactly
    and bf16 does not. The values after the pool are therefore only
    required to be multiples of 1/64 below 2^24 / 64 (exact in fp32)."""
    net = T.integerize(M.TinyMobileNetV2().eval(), seed=INT_SEED)
    x = T.int_input(MB_SHAPE, seed=INT_SEED)
    g = lower_torch(net, MB_SHAPE, strict=True)
    with torch.no_grad():
        want = net(x)
    vals = node_values(g, x)
    for n in g.nodes:
        v = vals[n.name].double()
        if v.dim() == 4:
            assert torch.equal(v, v.round()), n.name
            assert v.abs().max() <= 256, (n.name, v.abs().max().item())
        else:
            k = v * 64
            assert torch.equal(k, k.round()), n.name
            assert k.abs().max() < 2 ** 24
    return net, x, g, want


# ------------------------------------------------------------ whole model
def test_tiny_mobilenet_lowers_completely():
    net = M.TinyMobileNetV2().eval()
    g = lower_torch(net, MB_SHAPE, strict=True)
    assert _kept(g) == []
    gm = GraphModel(g)
    assert not [m for m in gm.modules()
                if isinstance(m, (nn.Conv2d, nn.BatchNorm2d, nn.Linear,
                                  nn.ReLU6, L.TorchIsland))]
    ty = _types(g)
    assert [n for n, t in ty.items() if t is L.ToNHWC] == ["input__nhwc"]
    assert L.ToNCHW not in ty.values()
    kinds = [t for t in ty.values()]
    # stem, block 2 and 3 expand, the last 1x1 (relu6) + three projects
    convs = [n.layer for n in g.nodes if type(n.layer) is L.ConvBNAct]
    assert [c.act for c in convs] == ["relu6", "none", "relu6", "none",
                                      "relu6", "none", "relu6"]
    dws = [n.layer for n in g.nodes if type(n.layer) is L.DepthwiseConvBNAct]
    assert [(d.c, d.stride, d.act) for d in dws] == [
        (8, 1, "relu6"), (32, 2, "relu6"), (32, 1, "relu6")]
    assert all(d.kernel == 3 and d.padding == 1 and d.weight.shape ==
               (3, 3, d.c) for d in dws)
    assert kinds.count(L.AddAct) == 1
    add = next(n.layer for n in g.nodes if type(n.layer) is L.AddAct)
    assert add.act == "none"
    # every in-place ReLU6 fused into its conv: none stands alone
    assert L.Relu6 not in kinds and L.Relu not in kinds
    assert kinds.count(L.GlobalAvgPool) == 1 and kinds.count(L.Dense) == 1
    assert len(g.nodes) == 1 + 7 + 3 + 1 + 2


def test_tiny_mobilenet_exact_integers():
    """Integer parameters and input: the lowered graph EQUALS the torch
    model in double. A wrong [C,1,R,S] -> [R,S,C] permutation, BN fold or a
    ReLU6 taken for a ReLU fails here."""
    net, x, g, want = exact_int_net()
    with torch.no_grad():
        want64 = T.as_double(net)(x.double())
        got = g.forward(x)
    assert torch.equal(want.double(), want64)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got.double(), want64)
    assert (got != 0).float().mean() >= 0.5
    # both clamps of a ReLU6 were hit on the way
    vals = node_values(g, x)
    dw = [vals[n.name] for n in g.nodes
          if type(n.layer) is L.DepthwiseConvBNAct]
    assert any((v == 6).any() for v in dw) and any((v == 0).any() for v in dw)


def test_tiny_mobilenet_random_floats():
    gen = torch.Generator().manual_seed(3)
    torch.manual_seed(3)
    net = T.randomize_bn(M.TinyMobileNetV2().eval(), gen)
    x = torch.randn(*MB_SHAPE, generator=gen)
    with torch.no_grad():
        ref = T.as_double(net)(x.double())
        got = lower_torch(net, MB_SHAPE).forward(x)
    err = ((got.double() - ref).abs().max() / ref.abs().max()).item()
    print(f"lowered fp32 vs float64 torch: rel err {err:.3e}")
    # fp32 against a double run: the longest chain is 27 + 8 + 9 + ... taps
    # through 11 layers; 2^-16 leaves 2^8 ulps for it
    assert err < 2.0 ** -16


# ------------------------------------------------------------------ ReLU6
@pytest.mark.parametrize("how", M.RELU6_SPELLINGS)
def test_relu6_spelling_fuses_into_conv(how):
    net = M.Relu6Net(how).eval()
    g = lower_torch(net, SMALL_SHAPE, strict=True)
    convs = [n.layer for n in g.nodes if type(n.layer) is L.ConvBNAct]
    assert [c.act for c in convs] == ["relu6"]
    assert L.Relu6 not in _types(g).values()
    x = torch.randn(*SMALL_SHAPE) * 4
    with torch.no_grad():
        assert torch.allclose(g.forward(x), net(x), atol=1e-5)


@pytest.mark.parametrize("how", M.RELU6_SPELLINGS)
def test_relu6_spelling_standalone(how):
    net = M.Relu6Net(how, after_pool=True).eval()
    g = lower_torch(net, SMALL_SHAPE, strict=True)
    kinds = list(_types(g).values())
    assert kinds.count(L.Relu6) == 1
    assert [n.layer.act for n in g.nodes
            if type(n.layer) is L.ConvBNAct] == ["none"]
    x = torch.randn(*SMALL_SHAPE) * 4
    with torch.no_grad():
        want = net(x)
        got = g.forward(x)
    assert torch.allclose(got, want, atol=1e-5)


def test_hardtanh_with_other_bounds_stays_an_island():
    net = M.Relu6Net("module").eval()
    net.act = nn.Hardtanh(-1., 6.)
    kept = _kept(lower_torch(net, SMALL_SHAPE))
    assert len(kept) == 1 and "Hardtanh" in kept[0][1]


def test_relu6_after_bn_add_and_linear_is_its_own_node():
    """bn_act, add_act and Dense do not learn relu6: a Relu6 node follows."""

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.c1 = nn.Conv2d(3, 8, 3, padding=1)
            self.pool = nn.MaxPool2d(2)
            self.bn = nn.BatchNorm2d(8)
            self.act = nn.ReLU6()
            self.fc = nn.Linear(8, 8)

        def forward(self, x):
            x = self.pool(self.c1(x))
            y = self.act(self.bn(x))
            z = self.act(x + y)
            return self.act(self.fc(z.mean(dim=(2, 3))))

    net = Net().eval()
    g = lower_torch(net, SMALL_SHAPE, strict=True)
    kinds = list(_types(g).values())
    assert kinds.count(L.Relu6) == 3
    assert g.by_name["bn"].layer.act == "none"
    assert [n.layer.act for n in g.nodes if type(n.layer) is L.AddAct] == [
        "none"]
    assert [n.layer.act for n in g.nodes if type(n.layer) is L.Dense] == [
        "none"]
    x = torch.randn(*SMALL_SHAPE) * 4
    with torch.no_grad():
        assert torch.allclose(g.forward(x), net(x), atol=1e-5)


def test_inplace_relu6_rebinds_its_input():
    """x = pool(...); y = relu6_(x); both later readers of x see y."""

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.c1 = nn.Conv2d(3, 8, 3, padding=1)
            self.pool = nn.MaxPool2d(2)
            self.act = nn.ReLU6(inplace=True)
            self.fc = nn.Linear(8, 8)

        def forward(self, x):
            x = self.pool(self.c1(x))
            y = self.act(x)
            return self.fc((x + y).mean(dim=(2, 3)))

    net = Net().eval()
    g = lower_torch(net, SMALL_SHAPE, strict=True)
    x = torch.randn(*SMALL_SHAPE) * 4
    with torch.no_grad():
        want = net(x.clone())
        got = g.forward(x)
    assert torch.allclose(got, want, atol=1e-5)
    add = next(n for n in g.nodes if type(n.layer) is L.AddAct)
    assert add.inputs == ["act", "act"]


# -------------------------------------------------------------- depthwise
@pytest.mark.parametrize("kw", [
    dict(kernel_size=3, padding=1), dict(kernel_size=3, stride=2, padding=0),
    dict(kernel_size=5, padding=2), dict(kernel_size=5, stride=2, padding=1)],
    ids=["3x3", "3x3s2p0", "5x5", "5x5s2p1"])
def test_depthwise_geometries_lower(kw):
    torch.manual_seed(5)
    net = M.DepthwiseNet(8, **kw).eval()
    g = lower_torch(net, SMALL_SHAPE, strict=True)
    dw = g.by_name["relu6"].layer
    assert type(dw) is L.DepthwiseConvBNAct and dw.act == "relu6"
    assert dw.scale is None                 # no BatchNorm in this net
    x = torch.randn(*SMALL_SHAPE) * 2
    with torch.no_grad():
        assert torch.allclose(g.forward(x), net(x), atol=1e-5)


@pytest.mark.parametrize("kw,word", [
    (dict(c=8, cout=16, kernel_size=3, padding=1), "groups=8"),
    (dict(c=8, kernel_size=3, padding=2, dilation=2), "dilat"),
    (dict(c=12, kernel_size=3, padding=1), "groups=12"),
    (dict(c=8, kernel_size=7, padding=3), "groups=8"),
    (dict(c=8, kernel_size=3, padding=2), "groups=8"),
], ids=["multiplier2", "dilation2", "c12", "7x7", "pad2"])
def test_depthwise_outside_the_kernel_stays_an_island(kw, word):
    net = M.DepthwiseNet(**kw).eval()
    g = lower_torch(net, SMALL_SHAPE)
    kept = _kept(g)
    # (with 12 channels the pool and the Linear behind it stay torch too)
    assert [n for n, _ in kept][0] == "dw", kept
    assert ("mean" in dict(kept)) == (kw.get("c") == 12), kept
    assert word in kept[0][1], kept[0][1]
    assert L.DepthwiseConvBNAct not in _types(g).values()
    with pytest.raises(ValueError, match="dw"):
        lower_torch(net, SMALL_SHAPE, strict=True)
    x = torch.randn(*SMALL_SHAPE)
    with torch.no_grad():
        assert torch.allclose(g.forward(x), net(x), atol=1e-5)


def test_functional_adaptive_pool_forms():
    import torch.nn.functional as F

    class Net(nn.Module):
        def __init__(self, size):
            super().__init__()
            self.size = size
            self.c1 = nn.Conv2d(3, 8, 3, padding=1)
            self.fc = nn.Linear(8 if size != 2 else 32, 8)

        def forward(self, x):
            x = F.adaptive_avg_pool2d(torch.relu(self.c1(x)), self.size)
            return self.fc(torch.flatten(x, 1))

    for size in (1, (1, 1)):
        net = Net(size).eval()
        g = lower_torch(net, SMALL_SHAPE, strict=True)
        assert list(_types(g).values()).count(L.GlobalAvgPool) == 1
        x = torch.randn(*SMALL_SHAPE)
        with torch.no_grad():
            assert torch.allclose(g.forward(x), net(x), atol=1e-5)
    kept = _kept(lower_torch(Net(2).eval(), SMALL_SHAPE))
    assert kept and "AdaptiveAvgPool2d" in kept[0][1]
