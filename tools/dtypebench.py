#!/usr/bin/env python3
"""Whole-model single-GPU throughput per compute dtype (bf16 vs fp32).

bench.py measures the flagship bf16 pipeline; this tool answers "what
does PipelineConfig(dtype="fp32") cost" for one model on one GPU:

    python tools/dtypebench.py --model resnet50 --batch 64 256 \
        --dtype fp32 bf16 --seconds 4

For each (dtype, batch) it warms up for --warmup-seconds of sustained
forwards (clocks and caches settle, every shape has launched), then
times whole forwards between two device events until the timed region
is at least --seconds long, and prints one JSON line per configuration.
Needs a GPU; there is no CPU fallback.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from defer_amd.graph import GraphModel
from defer_amd.models import MODELS
from defer_amd.parallel.pipeline import StageExecutor

DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def bench(model_name, dtype_name, batch, seconds, warmup_seconds, size):
    dev = "cuda:0"
    dtype = DTYPES[dtype_name]
    torch.manual_seed(0)
    model = MODELS[model_name]()
    ex = StageExecutor(GraphModel(model.graph), dev, dtype, use_graph=False)
    x = torch.randn(batch, size, size, 3, device=dev, dtype=dtype)

    def forwards(n):
        for _ in range(n):
            y = ex.run(x)
        return y

    # sustained warm-up, sized by wall clock around a device synchronize
    forwards(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_warm = 0
    while time.perf_counter() - t0 < warmup_seconds:
        forwards(2)
        torch.cuda.synchronize()
        n_warm += 2
    per_fwd = (time.perf_counter() - t0) / max(n_warm, 1)

    # one timed region of >= `seconds`, device events at both ends
    steps = max(4, int(seconds / per_fwd) + 1)
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    y = forwards(steps)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    assert torch.isfinite(y.float()).all(), "non-finite output"
    return dict(model=model_name, dtype=dtype_name, batch=batch,
                input=size, steps=steps, timed_s=round(ms / 1e3, 3),
                warmup_forwards=n_warm + 2,
                ms_per_forward=round(ms / steps, 3),
                images_per_sec=round(batch * steps / (ms / 1e3), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet50", choices=sorted(MODELS))
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--dtype", nargs="+", default=["fp32", "bf16"],
                    choices=sorted(DTYPES))
    ap.add_argument("--seconds", type=float, default=4.0,
                    help="minimum length of the timed region")
    ap.add_argument("--warmup-seconds", type=float, default=2.0)
    ap.add_argument("--input", type=int, default=224,
                    help="square input size")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dtypebench needs a GPU")
    for dt in args.dtype:
        for b in args.batch:
            r = bench(args.model, dt, b, args.seconds, args.warmup_seconds,
                      args.input)
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
