"""CPU: the grouped-conv reference op, GroupedConvBNAct, the ResNeXt graphs,
the grouped pattern of lower_torch and the cost model. The HIP kernels:
test_gconv_gpu.py."""

import pytest
import torch
import torch.nn as nn

from defer_amd import ops
from defer_amd.graph import GraphModel
from defer_amd.lower import lower_torch, lowering_report
from defer_amd.models import MODELS, resnet50, resnext50_32x4d
from defer_amd.models import layers as L
from defer_amd.models.resnet import _resnet
from defer_amd.ops import reference as ref
from defer_amd.parallel.partitioner import auto_partition, node_times


@pytest.mark.parametrize("cg", (4, 8, 16, 32))
@pytest.mark.parametrize("stride,pad", [(1, 1), (2, 1), (1, 0), (2, 0)])
def test_reference_is_a_conv_per_group(cg, stride, pad):
    g = torch.Generator().manual_seed(cg)
    c = 2 * max(16, cg)
    x = torch.randn(2, 9, 7, c, generator=g)
    w = torch.randn(c, 3, 3, cg, generator=g)
    scale = torch.rand(c, generator=g) + 0.5
    bias = torch.randn(c, generator=g)
    for act in ("none", "relu6", "hardswish"):
        want = torch.cat([
            ref.conv2d_bn_act(x[..., i:i + cg], w[i:i + cg], scale[i:i + cg],
                              bias[i:i + cg], stride, pad, act)
            for i in range(0, c, cg)], dim=-1)
        got = ops.gconv2d_bn_act(x, w, scale, bias, stride, pad, act)
        assert got.dtype == torch.float32
        assert torch.allclose(got, want, rtol=0,
                              atol=(9 * cg + 4) * 2.0 ** -24 * 64)


def test_cpu_op_refuses_what_the_gpu_refuses():
    bad = [((1, 4, 4, 32), (32, 3, 3, 2), 1, 1, "got 2"),
           ((1, 4, 4, 48), (48, 3, 3, 12), 1, 1, "got 12"),
           ((1, 4, 4, 24), (24, 3, 3, 8), 1, 1, "C = 24"),
           ((1, 8, 8, 32), (32, 5, 5, 8), 1, 1, "5x5"),
           ((1, 8, 8, 32), (32, 3, 3, 8), 3, 1, "got 3"),
           ((1, 8, 8, 32), (32, 3, 3, 8), 1, 2, "got 2")]
    for xs, ws, stride, pad, match in bad:
        with pytest.raises(ValueError, match=match):
            ops.gconv2d_bn_act(torch.zeros(xs), torch.zeros(ws), None, None,
                               stride, pad)
    with pytest.raises(ValueError, match="swish"):
        ops.gconv2d_bn_act(torch.zeros(1, 4, 4, 32), torch.zeros(32, 3, 3, 8),
                           act="swish")


def test_layer_shapes_flops_and_cost():
    lay = L.GroupedConvBNAct(128, 32, stride=2)
    assert tuple(lay.weight.shape) == (128, 3, 3, 4)
    assert lay.flops_per_pixel() == 2 * 9 * 4 * 128
    assert not isinstance(lay, L.ConvBNAct)
    y = lay(torch.randn(2, 9, 9, 128))
    assert tuple(y.shape) == (2, 5, 5, 128) and (y >= 0).all()
    flops, out_b, t_us = node_times(resnext50_32x4d().graph)
    # res2_0_conv2: 56x56x128 in and out, 4 channels per group
    assert flops["res2_0_conv2"] == 56 * 56 * 2 * 9 * 4 * 128
    assert t_us["res2_0_conv2"] == pytest.approx(
        2 * 56 * 56 * 128 * 2.0 / 4.5e12 * 1e6)


def test_resnext_models():
    for name, params in (("resnext50_32x4d", 25028904),
                         ("resnext101_64x4d", 83455272)):
        model = MODELS[name]()
        assert sum(p.numel() for p in model.parameters()) == params
    convs = [n.layer for n in model.graph.nodes if n.name.endswith("_conv2")]
    assert len(convs) == 33
    assert all(type(c) is L.GroupedConvBNAct and c.groups == 64
               for c in convs)
    assert [c.c for c in convs[:4]] == [256, 256, 256, 512]
    cuts, stages = auto_partition(resnext50_32x4d(), 4)
    assert len(set(cuts)) == 3 and len(stages) == 4
    assert set(cuts) <= set(resnext50_32x4d().graph.valid_cut_points())


def test_resnet_graphs_are_unchanged():
    a, b = resnet50(), _resnet((3, 4, 6, 3), "resnet50", groups=1)
    assert [(n.name, repr(n.layer), n.inputs) for n in a.graph.nodes] == \
        [(n.name, repr(n.layer), n.inputs) for n in b.graph.nodes]
    assert not any(isinstance(n.layer, L.GroupedConvBNAct)
                   for n in a.graph.nodes)
    assert sum(p.numel() for p in a.parameters()) == 25557032
    x = resnext50_32x4d()
    assert [n.name for n in x.graph.nodes] == [n.name for n in a.graph.nodes]


class _Grouped(nn.Module):
    def __init__(self, c=32, cout=None, groups=4, act=nn.Hardswish, **kw):
        super().__init__()
        kw = dict(dict(kernel_size=3, padding=1), **kw)
        self.conv = nn.Conv2d(c, cout or c, groups=groups, **kw)
        self.bn = nn.BatchNorm2d(cout or c)
        self.act = act()

    def forward(self, x):
        return self.act(self.bn(self.conv(x)))


@pytest.mark.parametrize("kw", [dict(), dict(stride=2, act=nn.ReLU6),
                                dict(c=64, groups=2, padding=0, act=nn.ReLU),
                                dict(groups=2, bias=False, act=nn.Identity)],
                         ids=["cg8", "s2_relu6", "cg32_p0", "cg16_none"])
def test_lowering_emits_the_grouped_layer(kw):
    torch.manual_seed(1)
    net = _Grouped(**kw).eval()
    net.bn.running_mean.normal_(0, 0.3)
    net.bn.running_var.uniform_(0.5, 2.0)
    c = net.conv.in_channels
    g = lower_torch(net, (2, c, 9, 11), strict=True)
    lay = [n.layer for n in g.nodes if isinstance(n.layer,
                                                  L.GroupedConvBNAct)]
    assert len(lay) == 1 and lay[0].groups == net.conv.groups
    assert tuple(lay[0].weight.shape) == (c, 3, 3, c // net.conv.groups)
    x = torch.randn(2, c, 9, 11)
    with torch.no_grad():
        assert torch.allclose(GraphModel(g).forward(x), net(x), atol=1e-5)


@pytest.mark.parametrize("kw", [
    dict(c=8, groups=2), dict(c=24, groups=3), dict(c=32, groups=16),
    dict(c=32, cout=64, groups=4), dict(kernel_size=5, padding=2),
    dict(padding=2, dilation=2), dict(padding=2), dict(stride=3)],
    ids=["c8", "c24", "cg2", "multiplier", "5x5", "dilated", "pad2", "s3"])
def test_illegal_grouped_convs_stay_islands(kw):
    net = _Grouped(**kw).eval()
    g = lower_torch(net, (2, net.conv.in_channels, 12, 12))
    kept = [r for _, r in lowering_report(g) if r != "lowered"]
    assert len(kept) == 1 and f"groups={net.conv.groups}" in kept[0]
    assert not any(isinstance(n.layer, L.GroupedConvBNAct) for n in g.nodes)
