"""GPU: every kernel of the bf16 conv dispatch table (csrc/conv.hip:
conv_rows x {none, relu, hardswish} x {residual, none}), of gelu_rows and of
conv_ws_kernel<ACT, RES>, launched at the smallest shape that plans it and
held bit for bit to conv_checks.expected on exact-integer data, plus one
(act, residual) pair per row on random floats held to the per-element bound
of conv_checks.check_bound. docs/TESTING.md has the construction.

The shapes are CASES of test_conv_dispatch_gpu.py (imported, not copied),
each the smallest that plans its row; before every call the plan is asked
again (ops.conv_plan), with and without a residual. The rows that only a
DEFER_CONV_VARIANT reaches run in a child process per letter
(tools/convrowscheck.py over conv_checks.FORCED_CASES), since the variable
is latched at first use."""

import os
import subprocess
import sys

import pytest
import torch

import conv_checks as C
import defer_amd.ops as ops
from test_conv_dispatch_gpu import CASES, planned_row

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_ACTS = ("none", "relu", "hardswish")     # ACT of a row's kernels
PAIRS = [(a, r) for a in KERNEL_ACTS for r in (False, True)]
IDS = [c[0].replace(", ", "-").replace(": ", "-") for c in CASES]

# the swin rows: Cin 3 -> 64 channels, 3x3, no residual (the binding sends a
# conv with a residual to the pad8 or stem path, see test_swin_rows).
# Stride 1 at 512 tiles of 8x16; stride 2 at the smallest square input of 4
# images that plans the row (OH = OW = 121: 16 x 8 tiles an image, just under
# the 18 % padding rule; asserted below).
SWIN = [
    ("swin: 3, 1", (4, 128, 128, 3), 64, 3, 1, 1),
    ("swin: 3, 2", (4, 241, 241, 3), 64, 3, 2, 1),
]
# conv_ws_kernel under mode=1: one 8x16 tile, and one pixel past a tile in
# both directions
WS = [(1, 8, 16, 64), (1, 9, 17, 64)]
# the GEMM-mode rows as [M, K] x [N, K]: what gelu_rows serves by default
GEMM = [(c[0], c[1][0] * c[1][1] * c[1][2], c[1][3], c[2])
        for c in CASES if "AMODE_GEMM" in c[0]]
# ops.linear: K 2048 / N 1000 (columns clamped in the last n-tile of 64) and
# a K that is no multiple of 64
LINEAR = [(200, 2048, 1000), (70, 200, 72)]


def _dev(t):
    return None if t is None else t.to(DEV)


_on_dev = {}


def _args(case):
    """A case's tensors on the device, moved once."""
    if id(case) not in _on_dev:
        _on_dev[id(case)] = (case, tuple(
            _dev(t) for t in (case.x, case.w, case.scale, case.bias,
                              case.res)))
    return _on_dev[id(case)][1]


def _conv(case, act, has_res, **kw):
    x, w, scale, bias, res = _args(case)
    return ops.conv2d_bn_act(x, w, scale, bias, stride=case.stride,
                             padding=case.pad, act=act,
                             residual=res if has_res else None, **kw)


def _tile(geom, has_res):
    _, xs, cout, r, stride, pad = geom
    p = ops.conv_plan(xs, (cout, r, r, xs[3]), stride, pad, has_res)
    return (p["BM"], p["BN"]) if p["family"] == "igemm" else None


def _row_of(plan):
    return f"{plan['family']}: {plan['template_args'].split(', ', 1)[1]}"


def _out_bytes(geom):
    _, xs, cout, r, stride, pad = geom
    oh, ow = C.out_hw(xs, r, stride, pad)
    return xs[0] * oh * ow * cout * 2


# ------------------------------------------------------------------ coverage
SWIN_RES_ALIAS = ("conv_swin_kernel has no RES parameter: the residual "
                  "column of a swin row holds the same three kernels, and "
                  "the binding plans no swin row for a conv with a residual")


def test_every_kernel_of_the_tables_is_launched():
    """rows x acts x residual of what the tests below launch equals the
    table, but for the named exclusion."""
    import defer_amd._hip_ops as hip

    table = {(row, a, r) for row in hip.conv_table_rows()
             for a in KERNEL_ACTS for r in (False, True)}
    assert len(table) == 192 + 12
    excluded = {(row, a, True): SWIN_RES_ALIAS for row, *_ in SWIN
                for a in KERNEL_ACTS}
    launched = {(c[0], a, r) for c in CASES for a, r in PAIRS}
    assert len(CASES) == 26 and len(launched) == 26 * 6
    launched |= {(c[0], a, False) for c in SWIN for a in KERNEL_ACTS}
    forced = {(c[0], a, r) for cases in C.FORCED_CASES.values()
              for c in cases for a, r in PAIRS}
    assert len(forced) == 6 * 6 and not forced & launched
    launched |= forced
    assert launched == table - set(excluded)
    assert len([k for k in launched if not k[0].startswith("swin")]) == 192
    # gelu_rows: one instantiation per GEMM-mode row of the table
    gelu = {row for row in hip.conv_table_rows() if "AMODE_GEMM" in row}
    assert len(gelu) == 10
    assert ({g[0] for g in GEMM}
            | {g[0] for gs in C.FORCED_GELU.values() for g in gs}) == gelu
    assert len(GEMM) == 8
    # conv_ws_kernel<ACT, RES>: test_conv_ws_kernels runs PAIRS
    assert len(PAIRS) == 6


# ------------------------------------------- the 26 default-reachable rows
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_row_exact_integers(i):
    """All six kernels of the row, and relu6 (the relu kernel with act_hi
    6), torch.equal to the one rounding of the exact value."""
    geom = CASES[i]
    row = geom[0]
    assert _out_bytes(geom) <= 16 << 20
    case = C.exact_case(*geom[1:])
    runs = PAIRS + [("relu6", bool(i % 2))]
    for act, has_res in runs:
        assert planned_row(geom, has_res) == row
        got = _conv(case, act, has_res)
        C.check_exact(case, act, has_res, got, row, _tile(geom, has_res))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_row_random_floats(i):
    """One (act, residual) pair per row, rotating over the six, held to the
    per-element bound."""
    geom = CASES[i]
    row = geom[0]
    act, has_res = PAIRS[i % 6]
    case = C.float_case(*geom[1:])
    assert planned_row(geom, has_res) == row
    got = _conv(case, act, has_res)
    worst = C.check_bound(case, act, has_res, got, row)
    print(f"{row} | {act} res={has_res}: worst err/bound {worst:.3f}")


# ---------------------------------------------------------- the swin rows
def _swin_plan(xs, stride, has_res):
    return ops.conv_plan(xs, (64, 3, 3, 3), stride, 1, has_res)


def test_swin_stride2_shape_is_the_smallest():
    for side in range(200, 241):
        assert _swin_plan((4, side, side, 3), 2, False)["path"] != "swin"


@pytest.mark.parametrize("i", range(len(SWIN)), ids=["s1", "s2"])
def test_swin_rows(i):
    geom = SWIN[i]
    row, xs, cout, r, stride, pad = geom
    assert _out_bytes(geom) <= 16 << 20
    plan = _swin_plan(xs, stride, False)
    # a swin row's template arguments carry no residual flag
    assert plan["path"] == "swin" and f"swin: {plan['template_args']}" == row
    assert plan["grid_x"] == 512
    case = C.exact_case(*geom[1:])
    for act in KERNEL_ACTS + ("relu6",):
        C.check_exact(case, act, False, _conv(case, act, False), row)
    # a residual never reaches conv_swin_kernel: prepare_conv asks for
    # !has_res, so the same conv with a residual plans an implicit-GEMM row
    # (pad8 at stride 1, stem at stride 2), and is exact there too
    plan = _swin_plan(xs, stride, True)
    assert plan["path"] == ("pad8", "stem")[i] and plan["family"] == "igemm"
    for act in ("relu", "hardswish"):
        C.check_exact(case, act, True, _conv(case, act, True),
                      f"{row} with a residual ({plan['path']})",
                      (plan["BM"], plan["BN"]))


# ------------------------------------------------------------ conv_ws_kernel
@pytest.mark.parametrize("xs", WS, ids=["8x16", "9x17"])
def test_conv_ws_kernels(xs):
    case = C.exact_case(xs, 64, 3, 1, 1)
    for act, has_res in PAIRS + [("relu6", True)]:
        plan = ops.conv_plan(xs, (64, 3, 3, 64), 1, 1, has_res, mode=1)
        assert plan["family"] == "ws"
        before = ops.conv_ws_stats()["launches"]
        got = _conv(case, act, has_res, mode=1)
        torch.cuda.synchronize()
        assert ops.conv_ws_stats()["launches"] == before + 1
        C.check_exact(case, act, has_res, got, f"conv_ws {xs}")
        # and the row the policy picks for this shape gives the same bits
        assert torch.equal(_conv(case, act, has_res, mode=2), got)


# ----------------------------------------------------------------- gelu_rows
@pytest.mark.parametrize("row,m,k,n", GEMM, ids=[
    g[0].replace(", ", "-").replace(": ", "-") for g in GEMM])
def test_gelu_rows(row, m, k, n):
    plan = ops.conv_plan((m, k), (n, k))
    assert _row_of(plan) == row
    case = C.gelu_case(m, k, n)
    got = ops.linear_gelu(_dev(case.x), _dev(case.w), _dev(case.bias)).cpu()
    worst = C.check_bound(case, "gelu", False, got, f"linear_gelu {row}")
    print(f"{row} | gelu: worst err/bound {worst:.3f}")
    # rows of x that are all zero, where the bias is 0: exactly 0
    zero = got[::5][:, case.bias == 0]
    assert zero.numel() and not zero.any()
    # erf(8 / sqrt(2)) is 1 in fp32: a pre-activation >= 8 comes back as
    # itself, rounded once
    big = case.v[0] >= 8
    assert torch.equal(got[big], case.v[0][big].float().to(torch.bfloat16))


# ---------------------------------------------------------------- ops.linear
@pytest.mark.parametrize("m,k,n", LINEAR, ids=["k2048n1000", "k200n72"])
def test_linear_exact_integers(m, k, n):
    plan = ops.conv_plan((m, k), (n, k))
    assert plan["family"] == "igemm" and n % plan["BN"]    # clamped columns
    case = C.linear_case(m, k, n)
    got = ops.linear(_dev(case.x), _dev(case.w), _dev(case.bias))
    C.check_exact(case, "none", False, got, f"linear {m}x{k}x{n}",
                  (plan["BM"], plan["BN"]))


# ------------------------------------- the rows behind DEFER_CONV_VARIANT
@pytest.mark.parametrize("letter", sorted(C.FORCED_CASES))
def test_forced_variant_rows(letter):
    """The variable is latched at first use: one fresh child per letter. A
    child that finds a mismatch names the row and exits non-zero; one that
    dies or runs out of time fails the test as well."""
    env = dict(os.environ, DEFER_CONV_VARIANT=letter)
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "tools", "convrowscheck.py"),
         letter],
        capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
