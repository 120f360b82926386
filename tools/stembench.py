#!/usr/bin/env python3
"""A/B of the fused stem conv + max-pool kernel (csrc/stem_pool.hip).

Times ops.conv_bn_act_maxpool with mode=1 (the fused kernel) against
mode=2 (pad + stem conv + maxpool, the path it replaces) on the 224x224
ResNet/DenseNet stem using device events, at batch 256 (the 1-GPU bench)
and batch 64 (the multi-stage micro-batch). The fused kernel belongs in
the policy only if it beats the launches it replaces by more than the
spread of the repeats at both batch sizes.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

import defer_amd.ops as ops

STEM = (2, 3, "relu", 3, 2, 1)   # stride, pad, act, pool k/s/p


def time_mode(args, mode, iters):
    for _ in range(5):
        ops.conv_bn_act_maxpool(*args, *STEM, mode=mode)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(True)
    t1 = torch.cuda.Event(True)
    t0.record()
    for _ in range(iters):
        ops.conv_bn_act_maxpool(*args, *STEM, mode=mode)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def bench_batch(B, HW, iters, repeats):
    dev = "cuda:0"
    bf = torch.bfloat16
    x = torch.randn(B, HW, HW, 3, device=dev, dtype=bf)
    w = torch.randn(64, 7, 7, 3, device=dev, dtype=bf) * 0.1
    scale = torch.rand(64, device=dev) + 0.5
    bias = torch.randn(64, device=dev) * 0.1
    args = (x, w, scale, bias)
    y1 = ops.conv_bn_act_maxpool(*args, *STEM, mode=1)
    y2 = ops.conv_bn_act_maxpool(*args, *STEM, mode=2)
    same = bool(torch.equal(y1, y2))
    # alternate the modes so drift hits both alike
    fused, two = [], []
    for _ in range(repeats):
        fused.append(time_mode(args, 1, iters))
        two.append(time_mode(args, 2, iters))
    # bytes the result needs: the raw input in, the pooled tensor out
    gb = (x.numel() + y1.numel()) * 2 / 1e9
    return dict(batch=B, hw=HW, bitwise=same, needed_mb=round(gb * 1e3, 1),
                fused_us=[round(v, 1) for v in fused],
                two_us=[round(v, 1) for v in two],
                fused_tbps=round(gb / (min(fused) * 1e-6) / 1e3, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 64])
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    rows = []
    for B in args.batches:
        r = bench_batch(B, args.hw, args.iters, args.repeats)
        rows.append(r)
        f, t = r["fused_us"], r["two_us"]
        verdict = ("WIN" if max(f) < min(t)
                   else "loss" if min(f) > max(t) else "noise")
        print(f"b{B:<4d} {args.hw}x{args.hw} "
              f"fused {min(f):7.1f}..{max(f):7.1f} us  "
              f"two {min(t):7.1f}..{max(t):7.1f} us  "
              f"{r['fused_tbps']:5.2f} TB/s of {r['needed_mb']} MB  "
              f"bitwise={r['bitwise']}  {verdict}", flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
