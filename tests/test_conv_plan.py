"""Conv kernel selection (csrc/conv_plan.h), checked without a GPU.

ops.conv_plan runs the geometry step of conv2d_bn_act and plan_conv and
nothing else, so the policy and the dispatch table are tested here on the
built extension alone.
"""

import itertools
import json
import os
import subprocess
import sys

import pytest

pytest.importorskip("defer_amd._hip_ops")

import defer_amd._hip_ops as hip  # noqa: E402
import defer_amd.ops as ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("", "l", "s", "w", "W")


def _golden():
    """tests/data/conv_plans.json: "kinds" lists each distinct
    "path|family|template_args"; a shape is [x, w, stride, pad, res, mode,
    max_blocks, groups] with trailing zeros left out (a linear layer [x, w,
    groups]) and a group [variant letters ("-" = unset, 0 = all five), kind,
    grid_x, grid_y, {further fields}].
    Returns (call, {variant: expected plan fields}) per shape."""
    with open(os.path.join(ROOT, "tests", "data", "conv_plans.json")) as f:
        data = json.load(f)
    out = []
    for *call, groups in data["shapes"]:
        plans = {}
        for letters, kind, gx, gy, *extra in groups:
            path, family, args = data["kinds"][kind].split("|")
            want = dict(path=path, family=family, template_args=args,
                        grid_x=gx, grid_y=gy, **(extra[0] if extra else {}))
            for v in letters or "-lswW":
                plans["" if v == "-" else v] = want
        out.append((call, plans))
    return out


def _plan(call, variant):
    x, w, stride, pad, res, mode, max_blocks = (
        call + ([1, 0] if len(call) == 2 else []) + [0, 0, 0])[:7]
    return ops.conv_plan(x, w, stride, pad, bool(res), mode=mode,
                         max_blocks=max_blocks, variant=variant)


def _row(plan):
    """The dispatch-table row a plan lands on (conv_ws has no table)."""
    if plan["family"] == "ws":
        return None
    args = plan["template_args"]
    if plan["family"] != "swin":
        args = args.split(", ", 1)[1]          # drop HAS_RES
    return f"{plan['family']}: {args}"


def test_golden_plans_match_parent():
    """Every record was logged by the launchers of the commit before the
    split (launches replaced by a log line, driven from a host program over
    the shape list): the kernel's template arguments after ACT and its grid,
    per shape and DEFER_CONV_VARIANT letter."""
    golden = _golden()
    assert len(golden) > 600
    bad = []
    for call, plans in golden:
        assert sorted(plans) == sorted(VARIANTS)
        for variant, want in plans.items():
            got = _plan(call, variant)
            have = {k: got[k] for k in want}
            if have != want:
                bad.append((call, variant, want, have))
    assert not bad, f"{len(bad)} plans differ, first: {bad[0]}"


def test_latched_variant_is_the_default():
    call = [[32, 56, 56, 128], [128, 3, 3, 128], 1, 1, 0, 0, 0]
    latched = os.environ.get("DEFER_CONV_VARIANT", "")
    assert _plan(call, None) == _plan(call, latched)


def test_table_is_complete_and_has_no_unreachable_row():
    """A coarse sweep never asks for a kernel the table lacks, and every
    row of the table is planned by a shape of the sweep or of the golden
    list."""
    rows = list(hip.conv_table_rows())
    assert len(rows) == len(set(rows))
    planned = set()
    for call, _ in _golden():
        for variant in VARIANTS:
            planned.add(_row(_plan(call, variant)))
    chans = (3, 8, 64, 128, 256, 512, 1000, 2048)
    for cin, cout, r, stride, h, nb, res, variant in itertools.product(
            chans, chans, (1, 3, 7), (1, 2), (7, 14, 28, 56, 112, 224),
            (1, 8, 256), (False, True), VARIANTS):
        # raises "no kernel for this plan" when the table has no row
        plan = ops.conv_plan((nb, h, h, cin), (cout, r, r, cin), stride,
                             r // 2, res, mode=0, variant=variant)
        planned.add(_row(plan))
    planned.discard(None)
    assert planned <= set(rows)
    assert not set(rows) - planned, sorted(set(rows) - planned)


def test_igemm_table_holds_the_reachable_instantiations_only():
    igemm = [r for r in hip.conv_table_rows() if r.startswith("igemm: ")]
    assert len(igemm) == 30                    # x 4 (act, res) = 120 kernels
    for r in igemm:
        amode, bp, bm, bn, da, db, wps = r[len("igemm: "):].split(", ")
        if bp == "true":
            assert amode in ("AMODE_GEMM", "AMODE_CONV") and bn == "64"
        if (da, db) == ("4", "2"):
            assert bp == "true"
        if wps != "2":
            assert (bm, bn) == ("64", "64")
            assert wps == ("4" if bp == "true" else "3")


@pytest.mark.parametrize("name", ["DEFER_CONV_WS", "DEFER_CONV_CHAIN",
                                  "DEFER_CHAIN_PROJ", "DEFER_STEM_POOL"])
def test_bad_env_mode_error_text(name):
    env = dict(os.environ, **{name: "1"})
    r = subprocess.run([sys.executable, "-c", "import defer_amd.ops"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode != 0
    assert (f"ValueError: {name}='1': expected unset, '0' or 'force'"
            in r.stderr)
