#!/usr/bin/env python3
"""Exact-integer check of the conv rows that only a DEFER_CONV_VARIANT
reaches (the legacy depths, the legacy 128x128 STEM gather, the TH 4 window)
and of the two legacy rows of gelu_rows.

    python tools/convrowscheck.py l
    python tools/convrowscheck.py w

The variable is latched at first use, so each letter needs a process of its
own: tests/test_conv_rows_gpu.py starts this once per letter. The shapes are
conv_checks.FORCED_CASES / FORCED_GELU of tests/conv_checks.py; each must
plan its row under the latched variant, and all six (act, residual) kernels
of a row must be torch.equal to conv_checks.expected. Exits non-zero on the
first mismatch and names the row."""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if len(sys.argv) != 2 or sys.argv[1] not in ("l", "w"):
    sys.exit("usage: convrowscheck.py l|w")
LETTER = sys.argv[1]
os.environ["DEFER_CONV_VARIANT"] = LETTER

import conv_checks as C  # noqa: E402
import defer_amd.ops as ops  # noqa: E402

DEV = "cuda:0"
ACTS = ("none", "relu", "hardswish")


def row_of(plan):
    return f"{plan['family']}: {plan['template_args'].split(', ', 1)[1]}"


def main():
    for row, xs, cout, r, stride, pad in C.FORCED_CASES[LETTER]:
        case = C.exact_case(xs, cout, r, stride, pad)
        x, w, scale, bias, res = (t.to(DEV) for t in (
            case.x, case.w, case.scale, case.bias, case.res))
        for act in ACTS:
            for has_res in (False, True):
                # variant=None: the value this process latched
                plan = ops.conv_plan(xs, (cout, r, r, xs[3]), stride, pad,
                                     has_res)
                if row_of(plan) != row:
                    sys.exit(f"FAIL {row}: {xs} plans {row_of(plan)} under "
                             f"DEFER_CONV_VARIANT={LETTER}")
                got = ops.conv2d_bn_act(x, w, scale, bias, stride=stride,
                                        padding=pad, act=act,
                                        residual=res if has_res else None)
                tile = ((plan["BM"], plan["BN"])
                        if plan["family"] == "igemm" else None)
                try:
                    C.check_exact(case, act, has_res, got, row, tile)
                except AssertionError as e:
                    sys.exit(f"FAIL {row}: {e}")
        print(f"{row}: 6 kernels exact", flush=True)
    for row, m, k, n in C.FORCED_GELU[LETTER]:
        plan = ops.conv_plan((m, k), (n, k))
        if row_of(plan) != row:
            sys.exit(f"FAIL gelu {row}: [{m}, {k}] x [{n}, {k}] plans "
                     f"{row_of(plan)} under DEFER_CONV_VARIANT={LETTER}")
        case = C.gelu_case(m, k, n)
        got = ops.linear_gelu(case.x.to(DEV), case.w.to(DEV),
                              case.bias.to(DEV)).cpu()
        try:
            worst = C.check_bound(case, "gelu", False, got, f"gelu {row}")
        except AssertionError as e:
            sys.exit(f"FAIL gelu {row}: {e}")
        if got[::5][:, case.bias == 0].any():
            sys.exit(f"FAIL gelu {row}: a zero row with bias 0 is not 0")
        print(f"gelu {row}: worst err/bound {worst:.3f}", flush=True)


if __name__ == "__main__":
    main()
