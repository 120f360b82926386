"""CPU tests of the checkers in conv_checks.py, which the GPU tests of the
bf16 conv kernels assert with (test_conv_rows_gpu.py), in the convention of
test_ops_checks.py: the exact check and the bound check pass on
`defer_amd.ops.reference` at small shapes, each fails on a deliberately
wrong implementation written here, and the premises of the exact check raise
when they do not hold."""

import pytest
import torch

import conv_checks as C
from defer_amd.ops import reference as ref

BF16 = torch.bfloat16

# (x shape NHWC, Cout, R, stride, pad): 3x3 s1 and s2, a 1x1 (its residual
# is part of every case), the 7x7 stem on 3 channels, a Cout that is no
# multiple of 8
SHAPES = {
    "3x3s1": ((2, 9, 11, 16), 24, 3, 1, 1),
    "3x3s2": ((2, 11, 13, 16), 24, 3, 2, 1),
    "1x1": ((1, 9, 14, 256), 40, 1, 1, 0),
    "7x7cin3": ((2, 20, 22, 3), 16, 7, 2, 3),
    "cout20": ((2, 9, 11, 16), 20, 3, 1, 1),
}
shapes = pytest.mark.parametrize("name", list(SHAPES))
PAIRS = [(a, r) for a in C.ACTS for r in (False, True)]


def trunc_bf16(y):
    """fp32 -> bf16 by dropping the low 16 bits: the rounding a kernel gets
    from a shift instead of a convert."""
    bits = y.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(BF16)


def rnd(y):
    return y.float().to(BF16).double()


def act64(v, act):
    if act == "gelu":
        return torch.nn.functional.gelu(v)
    if act == "hardswish":
        return v * (v + 3).clamp(0, 6) / 6
    return ref.apply_act(v, act)


def conv_with(case, act, has_res, wrong=None):
    """The conv of a case in float64 with one planted error (None = none),
    rounded to bf16 once at the end."""
    w = case.w.double()
    r = case.r
    if wrong == "last_k":
        w = w.clone()
        w[:, r - 1, r - 1, -1] = 0
    c = C.conv_nhwc(case.x, w, case.stride, case.pad)
    if wrong == "tap":
        # the last tap of output pixel (0, 0) of image 0: in bounds for
        # every shape here (r - 1 - pad >= 0)
        i = r - 1 - case.pad
        assert i >= 0
        c[0, 0, 0] -= (case.x[0, i, i].double()
                       @ case.w[:, r - 1, r - 1].double().t())
    scale, bias = case.scale.double(), case.bias.double()
    if wrong == "next_scale":
        scale = scale.roll(-1)
    if wrong == "next_bias":
        bias = bias.roll(-1)
    v = c * scale
    if wrong == "round_before_bias":
        v = rnd(v)
    v = v + bias
    if wrong == "round_before_res":
        v = rnd(v)
    if has_res and wrong != "no_res":
        v = v + case.res.double()
    if wrong == "act_on_rounded":
        v = rnd(v)
    y = act64(v, "relu" if wrong == "no_clamp6" and act == "relu6" else act)
    return trunc_bf16(y) if wrong == "trunc" else y.float().to(BF16)


def ref_conv(case, act, has_res):
    return ref.conv2d_bn_act(case.x, case.w, case.scale, case.bias,
                             case.stride, case.pad, act,
                             case.res if has_res else None)


def fails(check, *args):
    with pytest.raises(AssertionError) as e:
        check(*args)
    assert not isinstance(e.value, C.PremiseError)
    return str(e.value)


# ---- the reference passes ----

@shapes
def test_reference_passes_the_exact_check(name):
    case = C.exact_case(*SHAPES[name])
    for act, has_res in PAIRS:
        C.check_exact(case, act, has_res, ref_conv(case, act, has_res))
        # and so does the float64 formulation the planted errors start from
        C.check_exact(case, act, has_res, conv_with(case, act, has_res))
    # relu6 is 0 / 3 / 6 and hardswish v or 0
    assert set(C.expected(case, "relu6").unique().tolist()) == {0.0, 3.0, 6.0}
    v = case.v[0]
    assert torch.equal(C.expected(case, "hardswish"),
                       v.clamp(min=0).float().to(BF16))


@shapes
def test_reference_passes_the_bound_check(name):
    case = C.float_case(*SHAPES[name])
    for act, has_res in PAIRS:
        r = C.check_bound(case, act, has_res, ref_conv(case, act, has_res))
        assert 0 < r <= 1
    # the u_b term dominates: mag stays within a small multiple of |t|
    t, mag = C.truth(case, "none", True), case.mag[1]
    assert (1.5 * (case.K + 7) * C.U * mag).max() < C.U_B * t.abs().median()


def test_reference_passes_the_gelu_checks():
    case = C.gelu_case(70, 72, 48)
    r = C.check_bound(case, "gelu", False,
                      ref.linear_gelu(case.x, case.w, case.bias))
    assert 0 < r <= 1
    case = C.float_case((1, 9, 14, 64), 40, 1, 1, 0)
    v32 = ref.conv2d_bn_act(case.x.float(), case.w.float(), case.scale,
                            case.bias, 1, 0, "none")
    r = C.check_bound(case, "gelu", False, ref._gelu_f32(v32).to(BF16))
    assert 0 < r <= 1


def test_linear_case_is_exact_on_the_reference():
    for m, k, n in [(40, 2048, 72), (30, 200, 40)]:
        case = C.linear_case(m, k, n)
        C.check_exact(case, "none", False,
                      ref.linear(case.x, case.w, case.bias))
        fails(C.check_exact, case, "none", False,
              trunc_bf16(case.v[0]))


# ---- a wrong implementation fails the exact check ----

# planted error -> the (act, residual) pairs it is visible under
EXACT_ERRORS = {
    "trunc": [("none", False), ("relu", True), ("hardswish", False)],
    "round_before_res": [("none", True), ("relu", True), ("hardswish", True)],
    "round_before_bias": [("none", False), ("relu", True),
                          ("hardswish", False)],
    "next_scale": [("none", False), ("relu", True), ("relu6", False),
                   ("hardswish", True)],
    "next_bias": [("none", False), ("relu", True), ("relu6", False),
                  ("hardswish", True)],
    "no_res": [("none", True), ("relu", True), ("relu6", True),
               ("hardswish", True)],
    "no_clamp6": [("relu6", False), ("relu6", True)],
    "tap": [("none", False), ("none", True)],
    "last_k": [("none", False), ("relu", True), ("hardswish", False)],
}


@shapes
@pytest.mark.parametrize("wrong", list(EXACT_ERRORS))
def test_planted_error_fails_the_exact_check(wrong, name):
    case = C.exact_case(*SHAPES[name])
    for act, has_res in EXACT_ERRORS[wrong]:
        msg = fails(C.check_exact, case, act, has_res,
                    conv_with(case, act, has_res, wrong), name, (64, 64))
        assert "first at (row, column)" in msg and "tile (m, n)" in msg
    if wrong == "tap":      # one pixel: row 0 of the [M, Cout] output only
        assert "first at (row, column) (0, " in msg


def test_exact_check_refuses_dtype_and_shape_changes():
    case = C.exact_case(*SHAPES["3x3s1"])
    good = ref_conv(case, "none", False)
    fails(C.check_exact, case, "none", False, good.float())
    fails(C.check_exact, case, "none", False, good[:, :-1])
    nan = good.clone()
    nan[0, 0, 0, 0] = float("nan")
    fails(C.check_exact, case, "none", False, nan)


# ---- a wrong implementation fails the bound check ----

# K = 72, 64 and 72 (Cout 20: no multiple of 8)
SHALLOW = [((2, 9, 11, 8), 24, 3, 1, 1), ((1, 9, 14, 64), 40, 1, 1, 0),
           ((2, 9, 11, 8), 20, 3, 1, 1)]


@pytest.mark.parametrize("xs,cout,r,stride,pad", SHALLOW,
                         ids=["3x3", "1x1", "cout20"])
def test_activation_of_a_rounded_value_fails_the_bound_check(xs, cout, r,
                                                             stride, pad):
    case = C.float_case(xs, cout, r, stride, pad)
    assert case.K <= 128
    for act in ("hardswish", "gelu"):
        for has_res in ((False, True) if act == "hardswish" else (False,)):
            good = conv_with(case, act, has_res)
            assert C.check_bound(case, act, has_res, good) <= 1
            fails(C.check_bound, case, act, has_res,
                  conv_with(case, act, has_res, "act_on_rounded"))
    # truncation and a NaN fail it too
    fails(C.check_bound, case, "none", True,
          conv_with(case, "none", True, "trunc"))
    nan = conv_with(case, "relu", False).clone()
    nan.view(-1)[-1] = float("nan")
    fails(C.check_bound, case, "relu", False, nan)


# ---- the premises raise ----

def _small(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (2, 9, 11, 16), generator=g).float()
    w = torch.randint(-2, 3, (24, 3, 3, 16), generator=g).float()
    case = C.exact_case(*SHAPES["3x3s1"])
    return x, w, case.scale.clone(), case.bias.clone(), case.res.float()


def test_premises_hold_for_the_small_data():
    C.premises(*_small(), 1, 1)


def test_premises_raise_when_violated():
    x, w, scale, bias, res = _small()
    # products of signs: nearly every |v| stays below 256, a bf16 number
    with pytest.raises(C.PremiseError, match="no bf16 numbers"):
        C.premises(x.sign(), w.sign(), scale, bias.clamp(-12, 12),
                   torch.zeros_like(res), 1, 1)
    s = scale.clone()
    s[5] = 2.0
    with pytest.raises(C.PremiseError, match="no multiple of 3"):
        C.premises(x, w, s, bias, res, 1, 1)
    with pytest.raises(C.PremiseError, match="non-multiples of 3"):
        C.premises(x, w, scale, bias + 1, res, 1, 1)
    with pytest.raises(C.PremiseError, match="not all of"):
        C.premises(x, w, torch.full_like(scale, 3.0), bias, res, 1, 1)
    # Cout 70: the last n-tile of 64 holds 6 channels, all of one scale
    s = torch.tensor(C.SCALES).repeat(24)[:70].clone()
    s[-6:] = 3.0
    with pytest.raises(C.PremiseError, match="partial n-tile of 64"):
        C.premises(x, w[:1, :1, :1].repeat(70, 1, 1, 1), s, torch.zeros(70),
                   torch.zeros(2, 9, 11, 70), 1, 0)
    with pytest.raises(C.PremiseError, match="bf16 numbers"):
        C.premises(x + 2.0 ** -9, w, scale, bias, res, 1, 1)
    with pytest.raises(C.PremiseError, match="2\\^24"):
        C.premises(x, w, scale, bias * 2.0 ** 16, res, 1, 1)
    # all of one sign: v <= -3 never occurs
    with pytest.raises(C.PremiseError, match="misses one of"):
        C.premises(x.abs(), w.abs() * 3, None, bias.abs(), res.abs(), 1, 1)
    # 2^24 + 1: fp32 loses the sum that float64 keeps
    xw = torch.tensor([4096.0, 1, 0, 0, 0, 0, 0, 0]).view(1, 1, 1, 8)
    with pytest.raises(C.PremiseError, match="differs from the float64"):
        C.premises(xw, xw, None, torch.zeros(1), torch.zeros(1, 1, 1, 1),
                   1, 0)
