"""CPU tests of the checkers in ops_checks.py, which the GPU tests of the
pooling, elementwise, concat and softmax kernels assert with
(test_ops_edges_gpu.py): every checker passes on `defer_amd.ops.reference`
at the small shapes of the GPU file, in bf16 and fp32, and fails on a
deliberately wrong implementation written here. Also the refusals that the
CPU branch of `defer_amd.ops` shares with the bindings."""

import math

import pytest
import torch
import torch.nn.functional as F

import defer_amd.ops as ops
import ops_checks as C
from defer_amd.ops import reference as ref

BF16 = torch.bfloat16
both = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)


def trunc_bf16(y):
    """fp32 -> bf16 by dropping the low 16 bits: the rounding a kernel gets
    from a shift instead of a convert."""
    bits = y.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(BF16)


def fails(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


# ---- the reference stays inside every bound ----

@both
@pytest.mark.parametrize("shape", C.ELEMENTWISE_SHAPES, ids=["n8", "nhwc"])
def test_reference_passes_elementwise(shape, dtype):
    a = C.randn(shape, dtype, 1)
    b = C.randn(shape, dtype, 2)
    assert C.check_relu(a, ref.relu(a)) == 0.0
    x6 = C.relu6_data(shape, dtype, 3)
    assert (x6 == 0).any() and (x6 == 6).any()
    assert ((x6 > 0) & (x6 < 1e-30)).any() and ((x6 > 6) & (x6 < 6.1)).any()
    assert ((x6 < 6) & (x6 > 5.9)).any() and ((x6 < 0) & (x6 > -1e-30)).any()
    C.check_relu6(x6, ref.relu6(x6))
    for act in ("relu", "none"):
        C.check_add_act(a, b, act, ref.add_act(a, b, act))


@both
@pytest.mark.parametrize("act", ["none", "relu"])
def test_reference_passes_batchnorm(act, dtype):
    x = C.randn(C.BN_SHAPE, dtype, 4)
    scale = torch.rand(72) + 0.5
    bias = torch.randn(72)
    r = C.check_batchnorm_apply(x, scale, bias, act,
                                ref.batchnorm_apply(x, scale, bias, act))
    assert 0 < r <= 1


@both
@pytest.mark.parametrize("case", C.POOL_CASES, ids=C.POOL_IDS)
def test_reference_passes_pools(case, dtype):
    shape, (k, s, p) = case
    x = C.randn(shape, dtype, 5)
    C.check_maxpool2d(x, k, s, p, ref.maxpool2d(x, k, s, p))
    r = C.check_avgpool2d(x, k, s, p, ref.avgpool2d(x, k, s, p))
    assert r <= 1


@both
@pytest.mark.parametrize("kind", C.MAXPOOL_SPECIALS)
def test_reference_passes_maxpool_specials(kind, dtype):
    x = C.maxpool_special(kind, dtype)
    for k, s, p in C.POOL_GEOMS:
        y = ref.maxpool2d(x, k, s, p)
        C.check_maxpool2d(x, k, s, p, y)
        if kind == "neg_inf_image":
            assert (y[0] == -math.inf).all()
        if kind == "huge_negative":
            assert (y[1] == math.inf).any() and (y[1] < -1e38).any()


@both
def test_reference_passes_gap(dtype):
    for shape in C.GAP_SHAPES[dtype]:
        x = C.randn(shape, dtype, 6)
        assert C.check_global_avg_pool(x, ref.global_avg_pool(x)) <= 1


@both
def test_reference_passes_concat(dtype):
    for lead, c1, c2 in C.CAT2_CASES:
        xs = [C.randn(lead + (c1,), dtype, 7), C.randn(lead + (c2,), dtype, 8)]
        C.check_concat_channels(xs, ref.concat_channels(xs))
    xs = [C.randn((2, 7, 7, c), dtype, 9 + c) for c in (8, 24, 64)]
    C.check_concat_channels(xs, ref.concat_channels(xs))
    xs = [C.randn((2, 3, 5, c), BF16, 9 + c) for c in (12, 4)]
    C.check_concat_channels(xs, ref.concat_channels(xs))


@both
@pytest.mark.parametrize("case", C.SOFTMAX_CASES,
                         ids=[f"{r}x{c}" for r, c, _ in C.SOFTMAX_CASES])
def test_reference_passes_softmax(case, dtype):
    rows, cols, scale = case
    x = C.randn((rows, cols), dtype, 10, scale)
    r, rs = C.check_softmax(x, ref.softmax(x))
    assert r <= 1 and rs <= 1


@both
@pytest.mark.parametrize("kind", C.SOFTMAX_SPECIALS)
def test_reference_passes_softmax_specials(kind, dtype):
    x = C.softmax_special(kind, dtype)
    y = ref.softmax(x)
    C.check_softmax(x, y)
    if kind == "all_huge_negative":
        assert torch.equal(y[1], torch.full((100,), 0.01).to(dtype))


# ---- a wrong implementation fails its checker ----

def test_truncation_fails_batchnorm_avgpool_gap_softmax():
    x = C.randn(C.BN_SHAPE, BF16, 4)
    scale = torch.rand(72) + 0.5
    bias = torch.randn(72)
    for act in ("none", "relu"):
        y = x.float() * scale + bias
        y = torch.relu(y) if act == "relu" else y
        assert C.check_batchnorm_apply(x, scale, bias, act, y.to(BF16)) <= 1
        fails(C.check_batchnorm_apply, x, scale, bias, act, trunc_bf16(y))

    xc = x.float().permute(0, 3, 1, 2)
    for k, s, p in C.POOL_GEOMS:
        y = F.avg_pool2d(xc, k, s, p, count_include_pad=False)
        fails(C.check_avgpool2d, x, k, s, p,
              trunc_bf16(y.permute(0, 2, 3, 1)))

    g = C.randn((3, 7, 7, 2056), BF16, 6)
    fails(C.check_global_avg_pool, g, trunc_bf16(g.float().mean(dim=(1, 2))))

    for rows, cols, sc in C.SOFTMAX_CASES:
        if cols == 1:
            continue                 # p = 1 exactly under any rounding
        z = C.randn((rows, cols), BF16, 10, sc)
        fails(C.check_softmax, z, trunc_bf16(F.softmax(z.float(), dim=-1)))


def test_silent_bf16_downcast_fails_the_fp32_checkers():
    x = C.randn(C.BN_SHAPE, torch.float32, 4)
    scale = torch.rand(72) + 0.5
    bias = torch.randn(72)
    lossy = x.to(BF16).float()
    fails(C.check_batchnorm_apply, x, scale, bias, "none",
          ref.batchnorm_apply(lossy, scale, bias))
    fails(C.check_avgpool2d, x, 2, 2, 0, ref.avgpool2d(lossy, 2, 2, 0))
    fails(C.check_global_avg_pool, x, ref.global_avg_pool(lossy))
    z = 4 * torch.randn(5, 1000)
    fails(C.check_softmax, z, ref.softmax(z.to(BF16).float()))
    fails(C.check_relu, x, ref.relu(lossy))


@both
def test_count_include_pad_fails_avgpool(dtype):
    x = C.randn((2, 9, 11, 8), dtype, 5)
    for k, s, p in [(3, 2, 1), (3, 1, 1)]:
        y = F.avg_pool2d(x.float().permute(0, 3, 1, 2), k, s, p,
                         count_include_pad=True)
        fails(C.check_avgpool2d, x, k, s, p,
              y.permute(0, 2, 3, 1).to(dtype))


@both
def test_zero_padded_maxpool_fails_on_negative_data(dtype):
    x = C.maxpool_special("negative", dtype)
    xp = F.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1))
    y = F.max_pool2d(xp, 3, 2, 0).permute(0, 2, 3, 1).to(dtype)
    fails(C.check_maxpool2d, x, 3, 2, 1, y)


@both
@pytest.mark.parametrize("kind", ["neg_inf_image", "huge_negative"])
def test_maxpool_started_at_minus_1e30_fails(kind, dtype):
    x = C.maxpool_special(kind, dtype)
    for k, s, p in C.POOL_GEOMS:
        y = ref.maxpool2d(x, k, s, p).float()
        wrong = torch.maximum(y, torch.tensor(-1e30)).to(dtype)
        fails(C.check_maxpool2d, x, k, s, p, wrong)


@both
def test_wrong_divisor_fails_gap(dtype):
    for shape in C.GAP_SHAPES[dtype]:
        x = C.randn(shape, dtype, 6)
        hw = shape[1] * shape[2]
        y = (x.float().sum(dim=(1, 2)) / (hw + 1)).to(dtype)
        fails(C.check_global_avg_pool, x, y)


@both
def test_swapped_inputs_fail_concat(dtype):
    for lead, c1, c2 in C.CAT2_CASES:
        a = C.randn(lead + (c1,), dtype, 7)
        b = C.randn(lead + (c2,), dtype, 8)
        fails(C.check_concat_channels, [a, b], torch.cat([b, a], dim=-1))
    a = C.randn((2, 3, 3, 8), dtype, 7)      # equal widths: shape alone
    b = C.randn((2, 3, 3, 8), dtype, 8)      # cannot tell
    fails(C.check_concat_channels, [a, b], torch.cat([b, a], dim=-1))


@both
def test_softmax_without_max_subtraction_fails_near_80(dtype):
    x = (84 + 2 * torch.randn(3, 1000)).to(dtype)
    C.check_softmax(x, ref.softmax(x))
    e = torch.exp(x.float())                 # sums past fp32's largest
    fails(C.check_softmax, x, (e / e.sum(dim=-1, keepdim=True)).to(dtype))


def test_softmax_started_at_minus_1e30_fails():
    """The old start value of the running maximum: a row below it gives
    exp(x + 1e30) = 0 everywhere, s = 0 and NaN."""
    x = C.softmax_special("all_huge_negative", BF16)
    m = torch.maximum(x.float().max(dim=-1, keepdim=True).values,
                      torch.tensor(-1e30))
    e = torch.exp(x.float() - m)
    fails(C.check_softmax, x, (e / e.sum(dim=-1, keepdim=True)).to(BF16))


def test_wrong_clamp_and_missing_relu_fail():
    """An add_act that rounds a + b to bf16 before its ReLU is no control:
    round-to-nearest is monotone and keeps 0, so it commutes with
    max(., 0) and that implementation is bit-identical to the reference.
    The add_act controls here are a missing ReLU and a truncated sum."""
    x = C.relu6_data((2, 9, 11, 72), BF16, 3)
    fails(C.check_relu6, x, torch.clamp(x, 0.0, 6.03125))  # next bf16 up
    fails(C.check_relu6, x, torch.relu(x))
    fails(C.check_relu, x, x)
    a, b = C.randn((8,), BF16, 1), C.randn((8,), BF16, 2)
    fails(C.check_add_act, a, b, "relu", ref.add_act(a, b, "none"))
    fails(C.check_add_act, a, b, "none", trunc_bf16(a.float() + b.float()))


def test_sign_of_zero_is_not_pinned():
    x = torch.tensor([-0.0, 0.0, -1.0, 2.0] * 2, dtype=BF16)
    C.check_relu(x, torch.relu(x) * -1 * -1)
    C.check_relu(x, torch.tensor([0.0, -0.0, -0.0, 2.0] * 2, dtype=BF16))


def test_checkers_refuse_dtype_and_shape_changes():
    x = C.randn((1, 4, 4, 8), BF16, 1)
    fails(C.check_relu, x, ref.relu(x).float())
    fails(C.check_global_avg_pool, x, ref.global_avg_pool(x).float())
    fails(C.check_avgpool2d, x, 2, 2, 0, ref.avgpool2d(x, 2, 1, 0))


# ---- refusals of the CPU branch, the same as the bindings' ----

@both
@pytest.mark.parametrize("op", [ops.maxpool2d, ops.avgpool2d],
                         ids=["max", "avg"])
def test_cpu_pools_refuse_what_the_bindings_refuse(op, dtype):
    x = C.randn((1, 4, 4, 8), dtype, 1)
    with pytest.raises(RuntimeError, match="stride must be >= 1"):
        op(x, 2, 0, 0)
    with pytest.raises(RuntimeError, match="kernel must be >= 1"):
        op(x, 0, 1, 0)
    with pytest.raises(RuntimeError, match=r"pad must be in \[0, kernel / 2"):
        op(x, 3, 2, 2)
    with pytest.raises(RuntimeError, match=r"pad must be in \[0, kernel / 2"):
        op(x, 2, 2, -1)
    with pytest.raises(RuntimeError, match="smaller than the window"):
        op(C.randn((1, 2, 4, 8), dtype, 1), 3, 1, 0)
    with pytest.raises(RuntimeError, match="NHWC"):
        op(C.randn((4, 8), dtype, 1), 2, 2, 0)
    assert op(x, 3, 2, 1).shape == (1, 2, 2, 8)


@both
def test_cpu_batchnorm_softmax_gap_refusals(dtype):
    x = C.randn((1, 4, 4, 16), dtype, 1)
    ok = torch.ones(16)
    with pytest.raises(RuntimeError, match="length C"):
        ops.batchnorm_apply(x, torch.ones(8), ok)
    with pytest.raises(RuntimeError, match="length C"):
        ops.batchnorm_apply(x, ok, torch.ones(8))
    assert ops.batchnorm_apply(x, ok, ok).shape == x.shape
    with pytest.raises(RuntimeError, match="softmax of nothing"):
        ops.softmax(torch.empty(0, 8, dtype=dtype))
    with pytest.raises(RuntimeError, match="softmax of nothing"):
        ops.softmax(torch.empty(2, 0, dtype=dtype))
    with pytest.raises(RuntimeError, match="empty spatial extent"):
        ops.global_avg_pool(torch.empty(1, 0, 3, 8, dtype=dtype))
