#!/usr/bin/env python3
"""A/B of the weight-stationary 3x3 window kernel (csrc/conv_ws.hip).

Times ops.conv2d_bn_act with mode=1 (the new kernel) against mode=2 (the
window / implicit-GEMM paths it replaces) on the 64 -> 64 channel 3x3/s1/p1
classes, using device events: ResNet layer1 (56x56) at batch 256, 64, 8
and 1, and VGG19 block1_conv2 (224x224) at its bench batch. The policy
takes the new kernel for a class only where it beats the old path by more
than the spread of the repeats.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

import defer_amd.ops as ops

CLASSES = [
    # name, batch, H = W
    ("layer1", 256, 56),
    ("layer1", 64, 56),
    ("layer1", 8, 56),
    ("layer1", 1, 56),
    ("vgg_b1c2", 256, 224),
]


def time_mode(args, mode, iters, max_blocks):
    kw = dict(stride=1, padding=1, act="relu", mode=mode,
              max_blocks=max_blocks if mode == 1 else 0)
    for _ in range(5):
        ops.conv2d_bn_act(*args, **kw)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(True)
    t1 = torch.cuda.Event(True)
    t0.record()
    for _ in range(iters):
        ops.conv2d_bn_act(*args, **kw)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def bench_class(name, B, HW, iters, repeats, max_blocks):
    dev = "cuda:0"
    bf = torch.bfloat16
    x = torch.randn(B, HW, HW, 64, device=dev, dtype=bf)
    w = torch.randn(64, 3, 3, 64, device=dev, dtype=bf) * 0.05
    scale = torch.rand(64, device=dev) + 0.5
    bias = torch.randn(64, device=dev) * 0.1
    args = (x, w, scale, bias)
    y1 = ops.conv2d_bn_act(*args, stride=1, padding=1, act="relu", mode=1,
                           max_blocks=max_blocks)
    y2 = ops.conv2d_bn_act(*args, stride=1, padding=1, act="relu", mode=2)
    same = bool(torch.equal(y1, y2))
    st = ops.conv_ws_stats()
    # alternate the modes so drift hits both alike
    new, old = [], []
    for _ in range(repeats):
        new.append(time_mode(args, 1, iters, max_blocks))
        old.append(time_mode(args, 2, iters, max_blocks))
    # what the result needs: activations in and out, the weights once
    gb = (x.numel() + y1.numel() + w.numel()) * 2 / 1e9
    gflop = 2.0 * B * HW * HW * 64 * 576 / 1e9
    return dict(name=name, batch=B, hw=HW, equal=same,
                blocks=st["blocks"], tiles_per_block=st["tiles_per_block"],
                needed_mb=round(gb * 1e3, 1),
                new_us=[round(v, 1) for v in new],
                old_us=[round(v, 1) for v in old],
                new_tf=round(gflop / min(new) * 1e3, 1),
                old_tf=round(gflop / min(old) * 1e3, 1),
                new_tbps=round(gb / (min(new) * 1e-6) / 1e3, 2),
                old_tbps=round(gb / (min(old) * 1e-6) / 1e3, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-blocks", type=int, default=0,
                    help="grid cap of the new kernel (0 = its policy)")
    ap.add_argument("--only", default=None,
                    help="run one class, e.g. layer1:256")
    args = ap.parse_args()
    rows = []
    for name, B, HW in CLASSES:
        if args.only and args.only != f"{name}:{B}":
            continue
        r = bench_class(name, B, HW, args.iters, args.repeats,
                        args.max_blocks)
        rows.append(r)
        n, o = r["new_us"], r["old_us"]
        verdict = ("WIN" if max(n) < min(o)
                   else "loss" if min(n) > max(o) else "noise")
        print(f"{name:9s} b{B:<4d} {HW}x{HW} "
              f"new {min(n):7.1f}..{max(n):7.1f} us {r['new_tf']:6.1f} TF "
              f"{r['new_tbps']:5.2f} TB/s  "
              f"old {min(o):7.1f}..{max(o):7.1f} us {r['old_tf']:6.1f} TF "
              f"{r['old_tbps']:5.2f} TB/s  of {r['needed_mb']} MB  "
              f"grid {r['blocks']}x{r['tiles_per_block']}  "
              f"equal={r['equal']}  {verdict}", flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
