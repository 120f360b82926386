"""GPU: conv_fp8_kernel and quantize_fp8_kernel (csrc/conv_fp8.hip) and a
quantised toy ResNet through StageExecutor.

The exact gate is torch.equal on the bytes: every fp32 intermediate of its
data is exact, so the expected output is one RNE rounding of a known value,
with ties, saturation at +-448 and e4m3 subnormals in it (asserted on the CPU
in test_conv_fp8.py, on the same data). It is also what establishes the MFMA
operand and accumulator layout the kernel's header states. Random data is
held to the derived per-element bound of fp8_checks.py."""

import pytest
import torch

import fp8_checks as C
from defer_amd import ops, quant
from defer_amd.graph import GraphModel
from defer_amd.parallel.pipeline import StageExecutor

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FP8 = C.FP8
VARIANTS = [(res, out) for res in (False, True) for out in ("fp8", "bf16")]

# max-norm relative logit error of the CPU quantised toy ResNet against the
# CPU fp32 one on this file's seeded input: measured 0.02975. The GPU may not
# be further from the CPU quantised graph than that graph is from fp32.
E_Q = 0.0298


def _run(case, x, w, scale, bias, act, res, res_scale, out_scale):
    return ops.conv2d_bn_act_fp8(
        x.to(DEV), w.to(DEV), scale.to(DEV), bias.to(DEV), case[6], case[7],
        act, None if res is None else res.to(DEV), res_scale, out_scale,
        max_blocks=C.MAX_BLOCKS.get(case, 0)).cpu()


@pytest.mark.parametrize("case", C.CASES)
@pytest.mark.parametrize("act", C.ACTS)
def test_exact(case, act):
    x, w, res, scale, bias = C.make_inputs(case, exact=True)
    if case == C.CASES[5]:
        plan = ops.conv_fp8_plan(
            case[:4], (case[4], case[5], case[5], case[3]), case[6], case[7])
        assert plan["tile"] == "large" and plan["grid"] == 4
    for has_res, out in VARIANTS:
        r = res if has_res else None
        t, _ = C.expected(case, x, w, scale, bias, act, r, C.EXACT_RES_SCALE)
        out_scale = C.EXACT_OUT_SCALE if out == "fp8" else None
        got = _run(case, x, w, scale, bias, act, r, C.EXACT_RES_SCALE,
                   out_scale)
        if out == "fp8":
            want = (t / out_scale).float().clamp(-448.0, 448.0).to(FP8)
            assert got.dtype == FP8
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
        else:
            assert torch.equal(got, t.float().to(torch.bfloat16))


@pytest.mark.parametrize("case", C.CASES)
@pytest.mark.parametrize("act", C.ACTS)
def test_random_inside_bound(case, act):
    """Measured on the MI355X, the accumulation error left after the output
    rounding term, in units of 2^-24 mag, of 1.5 (K + 7) allowed: K = 48 (the
    bf16 MFMA on widened bytes) under 1 of 82.5; K = 128 159.4 of 202.5 and
    K = 144 105.5 of 226.5 on the fp8 MFMA, which does not sum its 128
    products like an fp32 chain (docs/STATE.md, "fp8 MFMA accumulation")."""
    x, w, res, scale, bias = C.make_inputs(case, exact=False)
    for has_res, out in VARIANTS:
        r = res if has_res else None
        t, mag = C.expected(case, x, w, scale, bias, act, r, 0.75)
        out_scale = 0.01 if out == "fp8" else None
        got = _run(case, x, w, scale, bias, act, r, 0.75, out_scale)
        C.check_bound(case, got, t, mag, out_scale)


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32))
def test_quantize_bytes(dtype):
    """Byte-equal to the torch expression: overshoots past +-448, ties,
    subnormals; max_blocks=1 makes the one workgroup stride 3 times."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3 * 256 * 16, generator=g) * 40.0
    x[:8] = torch.tensor([1e4, -1e4, 929.0, -897.0, 2.0 ** -8, -2.0 ** -9,
                          3 * 2.0 ** -10, 17.0 * 2])  # 2 * 17 / 2: a tie at 17
    x = x.to(dtype)
    inv = 1.0 / 2.0
    want = (x.float() * inv).clamp(-448, 448).to(FP8)
    assert bool((want.float().abs() == 448).any())
    assert bool(((want.float() != 0) & (want.float().abs() < 2.0 ** -6)).any())
    for max_blocks in (0, 1):
        got = ops.quantize_fp8(x.to(DEV), 2.0, max_blocks=max_blocks).cpu()
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


def test_gpu_refusals():
    case = C.CASES[0]
    x, w, _, scale, bias = (t.to(DEV) for t in C.make_inputs(case, True))
    with pytest.raises(ValueError):
        ops.conv2d_bn_act_fp8(x, w, scale.cpu(), bias, 1, 1)
    with pytest.raises(RuntimeError):       # a misaligned data pointer
        xm = torch.zeros(x.numel() + 16, dtype=torch.uint8, device=DEV)[
            8:8 + x.numel()].view(FP8).view(x.shape)
        ops.conv2d_bn_act_fp8(xm, w, scale, bias, 1, 1)


def test_toy_resnet_executor():
    g = C.toy_resnet()
    torch.manual_seed(1)
    x = torch.randn(2, 32, 32, 3)
    q = quant.quantize_graph(g, [x])
    with torch.no_grad():
        y_cpu = GraphModel(q)(x).float()
    xb = x.to(DEV, torch.bfloat16)
    eager = StageExecutor(GraphModel(q), DEV, torch.bfloat16).run(xb)
    assert eager.dtype == torch.bfloat16 and eager.shape == (2, 16)
    err = (eager.float().cpu() - y_cpu).abs().max() / y_cpu.abs().max()
    print("toy ResNet, GPU vs CPU quantised, max-norm relative:", float(err))
    assert float(err) <= E_Q
    graphed = StageExecutor(GraphModel(q), DEV, torch.bfloat16,
                            use_graph=True)
    for _ in range(3):
        assert torch.equal(graphed.run(xb), eager)
    assert graphed.use_graph, "capture fell back to eager"
