"""CPU: the reference forms of dwconv7x7, layernorm_channels and linear_gelu
against plain torch in float64, the refusals of the two channel-vector ops,
the three layers and convnext_tiny()."""

import pytest
import torch
import torch.nn.functional as F

from defer_amd import ops
from defer_amd.models import MODELS, convnext_tiny
from defer_amd.models.layers import (ConvBNAct, Dense, DepthwiseConv7x7,
                                     LayerNormC, PointwiseGelu)
from defer_amd.parallel.partitioner import partition_model


def _close(got, want64, tol=1e-5):
    return (got.double() - want64).abs().max() <= tol * want64.abs().max()


def test_reference_ops_match_float64_torch():
    x = torch.randn(2, 9, 5, 8)
    w, b = torch.randn(7, 7, 8) / 7, torch.randn(8)
    want = F.conv2d(x.double().permute(0, 3, 1, 2),
                    w.double().permute(2, 0, 1).unsqueeze(1), b.double(),
                    padding=3, groups=8).permute(0, 2, 3, 1)
    assert _close(ops.dwconv7x7(x, w, b), want)
    assert _close(ops.dwconv7x7(x, w), want - b.double())

    g, b = torch.randn(8), torch.randn(8)
    for t in (100 + x, x[0, 0]):
        want = F.layer_norm(t.double(), (8,), g.double(), b.double(), 1e-6)
        assert _close(ops.layernorm_channels(t.contiguous(), g, b), want,
                      1e-4)

    wl, b = torch.randn(12, 8), torch.randn(12)
    want = F.gelu(F.linear(x.double(), wl.double(), b.double()))
    got = ops.linear_gelu(x, wl, b)
    assert got.shape == (2, 9, 5, 12) and _close(got, want)


X = torch.zeros(1, 4, 4, 8)
W7, V8 = torch.zeros(7, 7, 8), torch.zeros(8)
DWCONV_REFUSALS = {
    "rank": ((X[0], W7, V8), "4-D"),
    "w rank": ((X, W7[0], V8), "3-D"),
    "strided": ((X.transpose(1, 2), W7, V8), "contiguous"),
    "mixed": ((X, W7.bfloat16(), V8), "mixed dtypes"),
    "bf16 C % 8": ((torch.zeros(1, 4, 4, 12).bfloat16(),
                    torch.zeros(7, 7, 12).bfloat16(), None), "C % 8 == 0"),
    "fp32 C % 4": ((torch.zeros(1, 4, 4, 6), torch.zeros(7, 7, 6), None),
                   "C % 4 == 0"),
    "short bias": ((X, W7, V8[:4]), "fp32[C]"),
    "5x5": ((X, torch.zeros(5, 5, 8), V8), "[7, 7, C]"),
}
LAYERNORM_REFUSALS = {
    "rank": ((V8, V8, V8), "rank >= 2"),
    "strided": ((X.transpose(1, 2), V8, V8), "contiguous"),
    "bf16 C % 8": ((torch.zeros(3, 12).bfloat16(), torch.zeros(12),
                    torch.zeros(12)), "C % 8 == 0"),
    "C > 2048": ((torch.zeros(2, 2052), torch.zeros(2052),
                  torch.zeros(2052)), "C <= 2048"),
    "short weight": ((X, V8[:4], V8), "fp32[C]"),
    "bf16 bias": ((X, V8, V8.bfloat16()), "fp32[C]"),
}


@pytest.mark.parametrize("op,case", [(ops.dwconv7x7, c)
                                     for c in DWCONV_REFUSALS.values()]
                         + [(ops.layernorm_channels, c)
                            for c in LAYERNORM_REFUSALS.values()],
                         ids=[f"dwconv7x7 {k}" for k in DWCONV_REFUSALS]
                         + [f"layernorm {k}" for k in LAYERNORM_REFUSALS])
def test_refusals_name_the_rule(op, case):
    args, rule = case
    with pytest.raises(RuntimeError) as e:
        op(*args)
    assert rule in str(e.value)


def test_gelu_is_no_act_of_an_existing_op():
    assert "gelu" not in ops._ACT_CODES
    with pytest.raises(ValueError):
        ops.conv2d_bn_act(X, torch.zeros(8, 1, 1, 8), padding=0, act="gelu")
    with pytest.raises(ValueError):
        Dense(8, 8, act="gelu")


def test_layers():
    x = torch.randn(2, 5, 6, 8)
    for layer, shape in ((DepthwiseConv7x7(8), x.shape),
                         (LayerNormC(8), x.shape),
                         (PointwiseGelu(8, 32), (2, 5, 6, 32))):
        assert layer(x).shape == shape and layer.extra_repr()
    assert DepthwiseConv7x7(8).weight.dim() == 3
    assert DepthwiseConv7x7(8).flops_per_pixel() == 2 * 49 * 8
    assert LayerNormC(8)(x[0, 0]).shape == (6, 8)
    assert ops.dwconv7x7(x[:0], W7, V8).shape == (0, 5, 6, 8)


def test_convnext_tiny():
    torch.manual_seed(0)
    model = convnext_tiny()
    assert MODELS["convnext_tiny"] is convnext_tiny
    assert sum(p.numel() for p in model.parameters()) == 28_589_128
    adds = [n.name for n in model.graph.nodes if n.name.endswith("_add")]
    assert len(adds) == 18
    assert set(adds) <= set(model.graph.valid_cut_points())
    stem = model.graph.nodes[0].layer
    assert isinstance(stem, ConvBNAct) and stem.scale is None
    x = torch.randn(1, 64, 64, 3)
    with torch.no_grad():
        whole = model(x)
        y = x
        for stage in partition_model(model, [adds[8]]):
            y = stage(y)
    assert whole.shape == (1, 1000) and torch.equal(y, whole)
