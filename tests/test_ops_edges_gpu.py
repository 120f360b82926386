"""GPU numerics of the pooling, elementwise, concat and softmax kernels
(csrc/pool.hip, csrc/elementwise.hip and their fp32 twins in
csrc/ops_f32.hip) at their edges, asserted per element with the derived
bounds of ops_checks.py (u = 2^-24, u_b = 2^-8; nothing measured):

* small shapes: border windows, one output pixel, odd sizes, a second
  channel block with one live lane, softmax rows narrower than, equal to and
  one past a wave, row counts that do not fill the last block;
* the start value of the running maximum (windows and rows below -1e30 and
  of -inf);
* launches with more lanes of work than the 2048 x 256 grid, so the second
  trip of every grid-stride loop is compared with something;
* the bindings' refusals.

Each test prints `envelope <op> <dtype> <err/bound>`; the figures of one run
are in profiles/numerics_envelope_bf16_ops.txt.
"""

import math

import pytest
import torch

import defer_amd.ops as ops
import ops_checks as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
both = pytest.mark.parametrize("dtype", C.DTYPES, ids=C.DTYPE_IDS)


def _name(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def _note(op, dtype, ratio):
    print(f"envelope {op} {_name(dtype)} {ratio:.4f}")


def _g(t):
    return t.to(DEV)


# ---- small edges ----

@both
@pytest.mark.parametrize("case", C.POOL_CASES, ids=C.POOL_IDS)
def test_pools_small(case, dtype):
    shape, (k, s, p) = case
    x = C.randn(shape, dtype, 5)
    C.check_maxpool2d(x, k, s, p, ops.maxpool2d(_g(x), k, s, p))
    _note("avgpool2d", dtype,
          C.check_avgpool2d(x, k, s, p, ops.avgpool2d(_g(x), k, s, p)))


@both
@pytest.mark.parametrize("kind", C.MAXPOOL_SPECIALS)
def test_maxpool_running_maximum_start(kind, dtype):
    x = C.maxpool_special(kind, dtype)
    for k, s, p in C.POOL_GEOMS:
        y = ops.maxpool2d(_g(x), k, s, p)
        C.check_maxpool2d(x, k, s, p, y)
        if kind == "neg_inf_image":
            assert (y[0] == -math.inf).all()


@both
def test_global_avg_pool_blocks(dtype):
    for shape in C.GAP_SHAPES[dtype]:
        x = C.randn(shape, dtype, 6)
        _note("global_avg_pool", dtype,
              C.check_global_avg_pool(x, ops.global_avg_pool(_g(x))))


@both
@pytest.mark.parametrize("case", C.CAT2_CASES,
                         ids=[f"{a}+{b}" for _, a, b in C.CAT2_CASES])
def test_concat_two_inputs_kernel(case, dtype):
    lead, c1, c2 = case
    xs = [C.randn(lead + (c1,), dtype, 7), C.randn(lead + (c2,), dtype, 8)]
    C.check_concat_channels(xs, ops.concat_channels([_g(t) for t in xs]))


@both
def test_concat_three_inputs(dtype):
    xs = [C.randn((2, 7, 7, c), dtype, 9 + c) for c in (8, 24, 64)]
    C.check_concat_channels(xs, ops.concat_channels([_g(t) for t in xs]))


def test_concat_two_inputs_copy_branch_24_byte_pitch():
    """C = 12 + 4 in bf16: 12 % 8 != 0, so the 2-D copies run."""
    xs = [C.randn((2, 3, 5, c), BF16, 9 + c) for c in (12, 4)]
    C.check_concat_channels(xs, ops.concat_channels([_g(t) for t in xs]))


@both
@pytest.mark.parametrize("case", C.SOFTMAX_CASES,
                         ids=[f"{r}x{c}" for r, c, _ in C.SOFTMAX_CASES])
def test_softmax_small(case, dtype):
    rows, cols, scale = case
    x = C.randn((rows, cols), dtype, 10, scale)
    r, rs = C.check_softmax(x, ops.softmax(_g(x)))
    _note("softmax", dtype, r)
    _note("softmax_rowsum", dtype, rs)


@both
@pytest.mark.parametrize("kind", C.SOFTMAX_SPECIALS)
def test_softmax_running_maximum_start(kind, dtype):
    x = C.softmax_special(kind, dtype)
    y = ops.softmax(_g(x))
    C.check_softmax(x, y)
    if kind == "all_huge_negative":
        assert torch.equal(y[1].cpu(), torch.full((100,), 0.01).to(dtype))


@both
@pytest.mark.parametrize("act", ["none", "relu"])
def test_batchnorm_small(act, dtype):
    x = C.randn(C.BN_SHAPE, dtype, 4)
    scale = torch.rand(72) + 0.5
    bias = torch.randn(72)
    y = ops.batchnorm_apply(_g(x), _g(scale), _g(bias), act)
    _note("batchnorm_apply", dtype,
          C.check_batchnorm_apply(x, scale, bias, act, y))


@both
@pytest.mark.parametrize("shape", C.ELEMENTWISE_SHAPES, ids=["n8", "nhwc"])
def test_elementwise_small(shape, dtype):
    a = C.randn(shape, dtype, 1)
    b = C.randn(shape, dtype, 2)
    C.check_relu(a, ops.relu(_g(a)))
    x6 = C.relu6_data(shape, dtype, 3)
    C.check_relu6(x6, ops.relu6(_g(x6)))
    for act in ("relu", "none"):
        C.check_add_act(a, b, act, ops.add_act(_g(a), _g(b), act))


# ---- the second trip of the grid-stride loops ----

def _crosses(n_lanes):
    """More work than the largest grid has lanes, and a last block that is
    not full."""
    assert n_lanes > C.GRID_CAP_LANES and n_lanes % 256 != 0, n_lanes


def _elementwise_numel(dtype):
    n = (8 if dtype == BF16 else 4) * 524549
    _crosses(C.lanes(n, dtype))
    return n


@both
def test_relu_relu6_loop(dtype):
    n = _elementwise_numel(dtype)
    x = C.randn((n,), dtype, 21, 4.0)
    C.check_relu(x, ops.relu(_g(x)))
    x6 = C.relu6_data((n,), dtype, 22)
    C.check_relu6(x6, ops.relu6(_g(x6)))


@both
def test_add_act_loop(dtype):
    n = _elementwise_numel(dtype)
    a = C.randn((n,), dtype, 23)
    b = C.randn((n,), dtype, 24)
    for act in ("relu", "none"):
        C.check_add_act(a, b, act, ops.add_act(_g(a), _g(b), act))


@both
def test_batchnorm_loop(dtype):
    shape = (58300, 72) if dtype == BF16 else (29150, 72)
    _crosses(C.lanes(shape[0] * shape[1], dtype))
    x = C.randn(shape, dtype, 25)
    scale = torch.rand(72) + 0.5
    bias = torch.randn(72)
    y = ops.batchnorm_apply(_g(x), _g(scale), _g(bias), "relu")
    _note("batchnorm_apply", dtype,
          C.check_batchnorm_apply(x, scale, bias, "relu", y))


def _pool_lanes(shape, k, s, p, dtype):
    n, h, w, c = shape
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    return C.lanes(n * oh * ow * c, dtype)


@both
def test_pools_2x2_loop(dtype):
    shape = (1, 514, 514, 64 if dtype == BF16 else 32)
    _crosses(_pool_lanes(shape, 2, 2, 0, dtype))
    x = C.randn(shape, dtype, 26)
    xg = _g(x)
    C.check_maxpool2d(x, 2, 2, 0, ops.maxpool2d(xg, 2, 2, 0))
    _note("avgpool2d", dtype,
          C.check_avgpool2d(x, 2, 2, 0, ops.avgpool2d(xg, 2, 2, 0)))


def test_maxpool_3x3_loop():
    shape = (1, 513, 513, 64)
    _crosses(_pool_lanes(shape, 3, 2, 1, BF16))
    x = C.randn(shape, BF16, 27)
    C.check_maxpool2d(x, 3, 2, 1, ops.maxpool2d(_g(x), 3, 2, 1))


@both
@pytest.mark.parametrize("hw", [(96, 96), (95, 97)], ids=["96x96", "95x97"])
def test_concat_loop(hw, dtype):
    """96 x 96 gives 552,960 lanes, which crosses the grid but is 2160 full
    blocks; 95 x 97 (552,900 lanes) also leaves the last block part full."""
    c1, c2 = (256, 224) if dtype == BF16 else (128, 112)
    n_lanes = C.lanes(hw[0] * hw[1] * (c1 + c2), dtype)
    if hw == (96, 96):
        assert n_lanes == 552960 > C.GRID_CAP_LANES
    else:
        _crosses(n_lanes)
    xs = [C.randn((1,) + hw + (c,), dtype, 28 + c) for c in (c1, c2)]
    C.check_concat_channels(xs, ops.concat_channels([_g(t) for t in xs]))


# ---- refusals ----

def test_batchnorm_bf16_refuses_cpu_or_short_scale():
    x = torch.zeros(1, 4, 4, 16, device=DEV, dtype=BF16)
    ok = torch.ones(16, device=DEV)
    for scale, bias in [(torch.ones(16), ok), (ok, torch.ones(16)),
                        (torch.ones(8, device=DEV), ok),
                        (ok, torch.ones(8, device=DEV))]:
        with pytest.raises(RuntimeError, match="GPU tensors of length C"):
            ops.batchnorm_apply(x, scale, bias)


@both
def test_softmax_and_gap_refuse_empty(dtype):
    with pytest.raises(RuntimeError, match="softmax of nothing"):
        ops.softmax(torch.empty(0, 8, device=DEV, dtype=dtype))
    with pytest.raises(RuntimeError, match="softmax of nothing"):
        ops.softmax(torch.empty(2, 0, device=DEV, dtype=dtype))
    with pytest.raises(RuntimeError, match="empty spatial extent"):
        ops.global_avg_pool(torch.empty(1, 0, 3, 8, device=DEV, dtype=dtype))


@both
@pytest.mark.parametrize("op", [ops.maxpool2d, ops.avgpool2d],
                         ids=["max", "avg"])
def test_pools_refuse_bad_geometry(op, dtype):
    x = torch.zeros(1, 4, 4, 8, device=DEV, dtype=dtype)
    with pytest.raises(RuntimeError, match="stride must be >= 1"):
        op(x, 2, 0, 0)
    with pytest.raises(RuntimeError, match=r"pad must be in \[0, kernel / 2"):
        op(x, 3, 2, 2)
    with pytest.raises(RuntimeError, match="smaller than the window"):
        op(torch.zeros(1, 2, 4, 8, device=DEV, dtype=dtype), 3, 1, 0)
