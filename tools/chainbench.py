#!/usr/bin/env python3
"""Per-shape A/B of the chained expand->reduce kernel (csrc/chain.hip).

For each ResNet bottleneck-boundary pair class (add_k -> res*_conv1) it
times ops.conv1x1_chain with mode=1 (fused kernel) against mode=2 (the
two conv launches) using device events, at batch 256 (the 1-GPU bench)
and batch 64 (the multi-stage micro-batch). A class belongs in the
launcher's policy table only if fused beats two-launch by more than the
spread of the repeats.

The last class, "L1 proj+64-256-64", is ops.conv1x1_chain_proj: mode=1 (the
chain kernel that makes the res2_0 projection shortcut itself) against
mode=2 (the projection launch plus the chain launch).
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

import defer_amd.ops as ops

PAIR_CLASSES = [
    # (name, HW, K1, N1, N2, pairs per ResNet50 step)
    ("L1 64-256-64", 56, 64, 256, 64, 2),
    ("L1 64-256-128", 56, 64, 256, 128, 1),
    ("L2 128-512-128", 28, 128, 512, 128, 3),
    ("L2 128-512-256", 28, 128, 512, 256, 1),
    ("L3 256-1024-256", 14, 256, 1024, 256, 5),
    ("L3 256-1024-512", 14, 256, 1024, 512, 1),
    ("L4 512-2048-512", 7, 512, 2048, 512, 2),
]


def time_mode(args, mode, iters, max_blocks=0, bm=None):
    for _ in range(5):
        ops.conv1x1_chain(*args, mode=mode, max_blocks=max_blocks, bm=bm)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(True)
    t1 = torch.cuda.Event(True)
    t0.record()
    for _ in range(iters):
        ops.conv1x1_chain(*args, mode=mode, max_blocks=max_blocks, bm=bm)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def bench_class(name, HW, K1, N1, N2, count, B, iters, repeats,
                max_blocks=0, fused_only=False, bm=None):
    dev = "cuda:0"
    bf = torch.bfloat16
    x = torch.randn(B, HW, HW, K1, device=dev, dtype=bf)
    res = torch.randn(B, HW, HW, N1, device=dev, dtype=bf)
    w3 = torch.randn(N1, 1, 1, K1, device=dev, dtype=bf) * 0.05
    w1 = torch.randn(N2, 1, 1, N1, device=dev, dtype=bf) * 0.05
    s3 = torch.rand(N1, device=dev) + 0.5
    b3 = torch.randn(N1, device=dev) * 0.1
    s1 = torch.rand(N2, device=dev) + 0.5
    b1 = torch.randn(N2, device=dev) * 0.1
    args = (x, w3, s3, b3, res, "relu", w1, s1, b1, "relu")
    y1, a1 = ops.conv1x1_chain(*args, mode=1, max_blocks=max_blocks, bm=bm)
    tile = ops.conv1x1_chain_stats()["bm"]
    y2, a2 = ops.conv1x1_chain(*args, mode=2)
    same = bool(torch.equal(y1, y2) and torch.equal(a1, a2))
    # alternate the modes so drift hits both alike
    fused, two = [], []
    for _ in range(repeats):
        fused.append(time_mode(args, 1, iters, max_blocks, bm))
        if not fused_only:
            two.append(time_mode(args, 2, iters))
    M = B * HW * HW
    # bytes the fused kernel must move: x, res in; y, a2 out
    gb = M * (K1 + 2 * N1 + N2) * 2 / 1e9
    return dict(name=name, batch=B, M=M, pairs=count, bitwise=same,
                max_blocks=max_blocks, tile_rows=tile,
                fused_us=[round(v, 1) for v in fused],
                two_us=[round(v, 1) for v in two],
                fused_tbps=round(gb / (min(fused) * 1e-6) / 1e3, 2))


PROJ_CLASS = ("L1 proj+64-256-64", 56, 64, 256, 64, 1)


def bench_proj(name, HW, K1, N1, N2, count, B, iters, repeats,
               max_blocks=0, fused_only=False):
    """ops.conv1x1_chain_proj: mode=1 (the shortcut made inside the chain
    kernel) against mode=2 (the projection launch plus the chain launch)."""
    dev = "cuda:0"
    bf = torch.bfloat16
    x = torch.randn(B, HW, HW, K1, device=dev, dtype=bf)
    xp = torch.randn(B, HW, HW, 64, device=dev, dtype=bf)
    w3 = torch.randn(N1, 1, 1, K1, device=dev, dtype=bf) * 0.05
    wp = torch.randn(N1, 1, 1, 64, device=dev, dtype=bf) * 0.05
    w1 = torch.randn(N2, 1, 1, N1, device=dev, dtype=bf) * 0.05
    s3, sp = (torch.rand(N1, device=dev) + 0.5 for _ in range(2))
    b3, bp = (torch.randn(N1, device=dev) * 0.1 for _ in range(2))
    s1 = torch.rand(N2, device=dev) + 0.5
    b1 = torch.randn(N2, device=dev) * 0.1
    args = (x, w3, s3, b3, xp, wp, sp, bp, "relu", w1, s1, b1, "relu")

    def run(mode, mb=0):
        return ops.conv1x1_chain_proj(*args, mode=mode, max_blocks=mb)

    def time_it(mode, mb=0):
        for _ in range(5):
            run(mode, mb)
        torch.cuda.synchronize()
        t0 = torch.cuda.Event(True)
        t1 = torch.cuda.Event(True)
        t0.record()
        for _ in range(iters):
            run(mode, mb)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / iters

    n0 = ops.chain_proj_stats()["launches"]
    y1, a1 = run(1, max_blocks)
    assert ops.chain_proj_stats()["launches"] == n0 + 1
    y2, a2 = run(2)
    same = bool(torch.equal(y1, y2) and torch.equal(a1, a2))
    fused, two = [], []
    for _ in range(repeats):
        fused.append(time_it(1, max_blocks))
        if not fused_only:
            two.append(time_it(2))
    M = B * HW * HW
    # bytes the fused kernel must move: x, xp in; y, a2 out
    gb = M * (K1 + 64 + N1 + N2) * 2 / 1e9
    return dict(name=name, batch=B, M=M, pairs=count, bitwise=same,
                max_blocks=max_blocks,
                fused_us=[round(v, 1) for v in fused],
                two_us=[round(v, 1) for v in two],
                fused_tbps=round(gb / (min(fused) * 1e-6) / 1e3, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 64])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--classes", nargs="+", default=None, metavar="K1-N1-N2",
                    help="only the classes whose name contains one of these")
    ap.add_argument("--max-blocks", type=int, nargs="+", default=[0],
                    help="persistent-grid caps to time the fused kernel at "
                         "(0 = the launcher's own grid)")
    ap.add_argument("--bm", type=int, nargs="+", default=[None],
                    choices=[0, 64, 128],
                    help="rows of a fused tile to time (0 = the launcher's "
                         "policy; default: DEFER_CHAIN_BM128); the projected "
                         "class has one form and ignores it")
    ap.add_argument("--fused-only", action="store_true",
                    help="time only the fused kernel (counter runs: one "
                         "kernel name in the profile)")
    args = ap.parse_args()
    classes = [c for c in PAIR_CLASSES + [PROJ_CLASS]
               if args.classes is None
               or any(k in c[0] for k in args.classes)]
    rows = []
    for B in args.batches:
        for c, mb, bm in [(c, mb, bm) for c in classes
                          for mb in args.max_blocks for bm in args.bm]:
            if c is PROJ_CLASS:
                r = bench_proj(*c, B, args.iters, args.repeats, mb,
                               args.fused_only)
            else:
                r = bench_class(*c, B, args.iters, args.repeats, mb,
                                args.fused_only, bm)
            rows.append(r)
            f, t = r["fused_us"], r["two_us"] or [float("nan")]
            verdict = ("WIN" if max(f) < min(t)
                       else "loss" if min(f) > max(t) else "noise")
            print(f"b{B:<4d} {r['name']:18s} M={r['M']:7d} mb={mb:<4d}"
                  f"bm={r.get('tile_rows', 64):<4d}"
                  f"fused {min(f):7.1f}..{max(f):7.1f} us  "
                  f"two {min(t):7.1f}..{max(t):7.1f} us  "
                  f"{r['fused_tbps']:5.2f} TB/s  bitwise={r['bitwise']}  "
                  f"{verdict}", flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
