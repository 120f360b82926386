"""CPU: the fp8 ops' reference branch, their refusals, the quantising pass
and the tile plan (fp8_checks.py has the data and the bounds)."""

import collections

import pytest
import torch

import fp8_checks as C
from defer_amd import ops, quant
from defer_amd.graph import GraphModel
from defer_amd.models import resnet50

FP8 = C.FP8


@pytest.mark.parametrize("case", C.CASES[:3] + C.CASES[4:5])
@pytest.mark.parametrize("act", C.ACTS)
def test_reference_exact(case, act):
    """Exact data: the reference op's bytes are the float64 value cast once,
    and the data holds ties, saturation and subnormals."""
    x, w, res, scale, bias = C.make_inputs(case, exact=True)
    for r in (None, res):
        t, _ = C.expected(case, x, w, scale, bias, act, r, C.EXACT_RES_SCALE)
        assert bool((t.float().double() == t).all())
        tq = t / C.EXACT_OUT_SCALE
        if act == "none":
            assert bool((tq.abs() > 448).any())                 # saturation
            assert bool(((tq != 0) & (tq.abs() < 2.0 ** -6)).any())
            frac = (tq.abs() * 2.0 ** 9) % 1.0                  # subnormal ulps
            assert bool(((frac == 0.5) & (tq.abs() < 2.0 ** -6)).any())  # ties
        got = ops.conv2d_bn_act_fp8(
            x, w, scale, bias, case[6], case[7], act, r, C.EXACT_RES_SCALE,
            C.EXACT_OUT_SCALE)
        want = tq.float().clamp(-448.0, 448.0).to(FP8)
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
        got = ops.conv2d_bn_act_fp8(x, w, scale, bias, case[6], case[7], act,
                                    r, C.EXACT_RES_SCALE)
        assert torch.equal(got, t.float().to(torch.bfloat16))


@pytest.mark.parametrize("case", C.CASES)
def test_reference_inside_bound(case):
    x, w, res, scale, bias = C.make_inputs(case, exact=False)
    for act, r, out_scale in (("none", None, None), ("relu", res, 0.01),
                              ("relu6", res, None), ("none", res, 0.004)):
        t, mag = C.expected(case, x, w, scale, bias, act, r, 0.75)
        got = ops.conv2d_bn_act_fp8(x, w, scale, bias, case[6], case[7], act,
                                    r, 0.75, out_scale)
        C.check_bound(case, got, t, mag, out_scale)


def test_quantize_fp8_reference():
    x = torch.tensor([500.0, -1e4, 0.0, 2.0 ** -10, 17.0, -0.3] + [1.0] * 10)
    q = ops.quantize_fp8(x, 0.5)
    assert q.dtype == FP8 and torch.isfinite(q.float()).all()
    assert q.float()[:2].tolist() == [448.0, -448.0]


def test_refusals():
    case = C.CASES[0]
    x, w, res, scale, bias = C.make_inputs(case, exact=True)
    good = dict(x_q=x, w_q=w, scale=scale, bias=bias, stride=1, padding=1)
    ops.conv2d_bn_act_fp8(**good)
    for bad in (dict(x_q=x.float()), dict(w_q=w.to(torch.bfloat16)),
                dict(residual_q=res.float()), dict(residual_q=res[:, :3]),
                dict(scale=scale[:8]), dict(bias=bias.double()),
                dict(scale=None), dict(act="hardswish"), dict(stride=3),
                dict(padding=2), dict(x_q=x[..., :8].contiguous()),
                dict(w_q=w[:8].contiguous(), scale=scale[:8], bias=bias[:8]),
                dict(w_q=w[:, :, :2].contiguous())):
        with pytest.raises(ValueError):
            ops.conv2d_bn_act_fp8(**{**good, **bad})
    with pytest.raises(ValueError):
        ops.quantize_fp8(torch.zeros(16, dtype=torch.float64), 1.0)
    with pytest.raises(ValueError):
        ops.quantize_fp8(torch.zeros(24), 1.0)
    with pytest.raises(ValueError):
        ops.quantize_fp8(torch.zeros(16), 0.0)


def test_quantize_graph_toy():
    g = C.toy_resnet()
    x = torch.randn(2, 32, 32, 3)
    q = quant.quantize_graph(g, [x])
    status = dict(quant.report(q))
    # names kept: the fused add takes the add's name, nothing else renamed
    kept = [n for n in g.layer_names() if not n.endswith("_conv3")]
    assert [n for n in q.layer_names() if n != "pool1_fp8"] == kept
    assert status["conv1"].startswith("kept: channels 3->64")
    assert status["pool1_fp8"] == "quantize"
    assert q.by_name["pool1_fp8"].inputs == ["pool1"]
    assert q.by_name["res2_0_conv1"].inputs == ["pool1_fp8"]
    assert q.by_name["res2_0_proj"].inputs == ["pool1_fp8"]
    assert q.by_name["add_1"].inputs == ["res2_0_conv2", "res2_0_proj"]
    convs = [n for n, s in status.items() if s.startswith("fp8")]
    assert len(convs) == 12
    # e4m3 wherever every reader is a converted conv; the last add feeds GAP
    assert [n for n in convs if status[n] == "fp8 -> bf16"] == ["add_3"]
    lay = q.by_name["add_1"].layer
    assert lay.weight_q.dtype == FP8 and not list(lay.parameters())
    y, yq = GraphModel(g)(x), GraphModel(q)(x)
    assert yq.shape == y.shape and torch.isfinite(yq.float()).all()
    # the original graph is untouched and still runs unfused
    assert torch.equal(GraphModel(g)(x), y)


def test_report_resnet50():
    rows = quant.report(resnet50())
    counts = collections.Counter(s.split(":")[0] for _, s in rows)
    assert counts["fp8"] == 52
    assert dict(rows)["conv1"].startswith("kept: channels 3->64")


def test_plan_tiles():
    for case in C.CASES:
        n, h, w, cin, cout, r, stride, pad = case
        plan = ops.conv_fp8_plan((n, h, w, cin), (cout, r, r, cin), stride,
                                 pad, C.MAX_BLOCKS.get(case, 0))
        m = C.out_shape(case)[0] * C.out_shape(case)[1] * C.out_shape(case)[2]
        large = case in (C.CASES[3], C.CASES[5])
        assert plan["tile"] == ("large" if large else "small"), case
        assert plan["k_tiles"] == -(-r * r * cin // 128)
        assert plan["mfma"] == ("bf16" if r * r * cin < 128 else "fp8")
        assert plan["m_tiles"] == -(-m // plan["bm"])
    assert ops.conv_fp8_plan((2, 20, 20, 128), (128, 1, 1, 128), 1, 0,
                             2)["grid"] == 2
    with pytest.raises(RuntimeError):
        ops.conv_fp8_plan((1, 8, 8, 24), (16, 3, 3, 24), 1, 1)
