#!/usr/bin/env python3
"""Codec throughput on MI355X: encode/decode GB/s per boundary shape.

    codecbench.py                        fixed-rate ZFP + fp8 on randn
    codecbench.py --case lossless        the lossless wire on real ResNet50
                                         boundary activations (+ zfp rate 8
                                         and fp8 on the same tensors)
    codecbench.py --case lossless-ratio  its ratios from the numpy spec, on
                                         the CPU
"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch
from defer_amd.ops import codec
import defer_amd._hip_ops as hip

SHAPES = [  # ResNet50 boundary activations at batch 64 (bf16)
    ("add_2 56x56x256", (64, 56, 56, 256)),
    ("add_8 28x28x512", (64, 28, 28, 512)),
    ("add_12 14x14x1024", (64, 14, 14, 1024)),
    ("add_16 7x7x2048", (64, 7, 7, 2048)),
]

def bench(shape, rate, iters=30):
    x = torch.randn(*shape, device="cuda", dtype=torch.bfloat16)
    w = codec.zfp_encode(x, rate)
    y = codec.zfp_decode(w, shape, rate, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    t0, t1, t2 = (torch.cuda.Event(True) for _ in range(3))
    t0.record()
    for _ in range(iters):
        codec.zfp_encode(x, rate, out=w)
    t1.record()
    for _ in range(iters):
        y = codec.zfp_decode(w, shape, rate, dtype=torch.bfloat16)
    t2.record()
    torch.cuda.synchronize()
    enc_us = t0.elapsed_time(t1) * 1e3 / iters
    dec_us = t1.elapsed_time(t2) * 1e3 / iters
    # phase bisection: transform-only / serialize-only encodes
    ph = {}
    for phase in (1, 2, 4, 5):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        for _ in range(iters):
            hip.zfp_encode(x, rate, w, phase)
        b.record()
        torch.cuda.synchronize()
        ph[phase] = a.elapsed_time(b) * 1e3 / iters
    mb = x.numel() * 2 / 1e6
    return enc_us, dec_us, mb, w.numel() / 1e6, ph

def bench_fp8(shape, iters=50):
    x = torch.randn(*shape, device="cuda", dtype=torch.bfloat16)
    n = x.numel()
    w = torch.empty(n + 4, dtype=torch.uint8, device="cuda")
    hip.fp8_encode(x, w)
    y = hip.fp8_decode(w, list(shape))
    torch.cuda.synchronize()
    t0, t1, t2 = (torch.cuda.Event(True) for _ in range(3))
    t0.record()
    for _ in range(iters):
        hip.fp8_encode(x, w)
    t1.record()
    for _ in range(iters):
        y = hip.fp8_decode(w, list(shape))
    t2.record()
    torch.cuda.synchronize()
    enc = t0.elapsed_time(t1) * 1e3 / iters
    dec = t1.elapsed_time(t2) * 1e3 / iters
    mb = n * 2 / 1e6
    print(f"fp8  {str(shape):20s}: enc {enc:7.1f} us ({mb/enc*1e3:6.0f} GB/s) "
          f"dec {dec:7.1f} us ({mb/dec*1e3:6.0f} GB/s)  {mb:.0f}->{(n+4)/1e6:.0f} MB")


def zfp_case():
    for name, shape in SHAPES:
        bench_fp8(shape)
    for name, shape in SHAPES:
        for rate in (4, 8):
            e, d, mb, wmb, ph = bench(shape, rate)
            print(f"{name:20s} rate{rate:2d}: enc {e:7.1f} us ({mb/e*1e3:6.0f} GB/s) "
                  f"dec {d:7.1f} us ({mb/d*1e3:6.0f} GB/s)  {mb:.0f}->{wmb:.0f} MB"
                  f"  [p1 {ph[1]:.1f}us p2 {ph[2]:.1f}us stage {ph[4]:.1f}us lift {ph[5]:.1f}us]")


# ---- lossless case: REAL boundary activations (the ratio is made of ReLU
# zeros and clustered exponents; randn has neither) -------------------------
LOSSLESS_CUTS = ["add_2", "add_4", "add_8", "add_14"]
XGMI_GBPS = 153.0   # one xGMI link, the project's hop figure


def boundary_activations(cuts, batch, device, dtype, seed=0):
    """ResNet50 (random init, `seed`) forward on randn input; returns
    [(cut name, activation at that cut)] in `dtype` on `device`."""
    from defer_amd.models import resnet50
    from defer_amd.parallel.partitioner import partition_model
    from defer_amd.parallel.pipeline import StageExecutor

    torch.manual_seed(seed)
    model = resnet50()
    x = torch.randn(batch, 224, 224, 3).to(device=device, dtype=dtype)
    acts = []
    for name, stage in zip(cuts, partition_model(model, cuts)):
        x = StageExecutor(stage, device, dtype).run(x)
        acts.append((name, x))
    return acts


def _timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us


def lossless_case(batch, iters):
    """Per boundary and dtype: lossless ratio + encode/decode GB/s over raw
    bytes, zfp rate 8 and fp8 on the same tensor, and the hop arithmetic
    raw/153 GB/s vs encode + wire/153 GB/s + decode."""
    print(f"# ResNet50 boundaries, batch {batch}, random init seed 0, "
          f"{torch.cuda.get_device_name(0)}; GB/s are over RAW bytes; "
          f"hop times at {XGMI_GBPS:.0f} GB/s per xGMI link")
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        for name, x in boundary_activations(LOSSLESS_CUTS, batch, "cuda",
                                            dtype):
            x = x.contiguous()
            shape = tuple(x.shape)
            raw = x.numel() * x.element_size()
            bits = 16 if dtype == torch.bfloat16 else 32
            zeros = (x == 0).float().mean().item()
            out = torch.empty(int(hip.pack_wire_bytes_max(x.numel(), bits)),
                              dtype=torch.uint8, device="cuda")
            scratch = torch.empty(
                int(hip.pack_scratch_bytes(x.numel(), bits)),
                dtype=torch.uint8, device="cuda")
            size = torch.zeros(1, dtype=torch.long, device="cuda")
            enc = _timed(lambda: hip.pack_encode_into(x, scratch, out, size),
                         iters)
            wire = out[:int(size.item())]
            dec = _timed(lambda: hip.pack_decode(wire, list(shape),
                                                 bits == 16), iters)
            y = hip.pack_decode(wire, list(shape), bits == 16)
            idt = torch.int16 if bits == 16 else torch.int32
            assert torch.equal(y.view(idt), x.view(idt)), "round trip"
            wb = wire.numel()
            raw_us = raw / (XGMI_GBPS * 1e3)
            hop_us = enc + wb / (XGMI_GBPS * 1e3) + dec
            print(f"{name:7s} {tag} {str(shape):20s} zeros {zeros*100:4.1f}%  "
                  f"lossless {raw/wb:5.2f}x  enc {enc:8.1f} us "
                  f"({raw/enc/1e3:6.0f} GB/s)  dec {dec:8.1f} us "
                  f"({raw/dec/1e3:6.0f} GB/s)  hop raw {raw_us:8.1f} us vs "
                  f"lossless {hop_us:8.1f} us "
                  f"({'shorter' if hop_us < raw_us else 'LONGER'})")
            w = codec.zfp_encode(x, 8)
            ze = _timed(lambda: codec.zfp_encode(x, 8, out=w), iters)
            zd = _timed(lambda: codec.zfp_decode(w, shape, 8, dtype=dtype),
                        iters)
            print(f"{'':7s} {tag} {'':20s} zfp rate 8 {raw/w.numel():5.2f}x"
                  f" (lossy)  enc {ze:8.1f} us ({raw/ze/1e3:6.0f} GB/s)  "
                  f"dec {zd:8.1f} us ({raw/zd/1e3:6.0f} GB/s)")
            if dtype == torch.bfloat16:      # the fp8 kernels take bf16
                fw = torch.empty(x.numel() + 4, dtype=torch.uint8,
                                 device="cuda")
                fe = _timed(lambda: hip.fp8_encode(x, fw), iters)
                fd = _timed(lambda: hip.fp8_decode(fw, list(shape)), iters)
                print(f"{'':7s} {tag} {'':20s} fp8        "
                      f"{raw/fw.numel():5.2f}x (lossy)  enc {fe:8.1f} us "
                      f"({raw/fe/1e3:6.0f} GB/s)  dec {fd:8.1f} us "
                      f"({raw/fd/1e3:6.0f} GB/s)")


def ratio_case(batch):
    """No GPU: per-boundary lossless ratios from the numpy spec, fp32 CPU
    forward (and the same values rounded to bf16)."""
    import numpy as np
    from defer_amd.ops import pack_ref

    print(f"# lossless wire ratio per ResNet50 boundary: numpy spec "
          f"(defer_amd/ops/pack_ref.py), CPU fp32 forward, random init "
          f"seed 0, randn input, batch {batch}")
    print(f"{'boundary':9s} {'shape':20s} {'zeros':>6s} {'bf16':>7s} "
          f"{'fp32':>7s}")
    cuts = ["pool1"] + LOSSLESS_CUTS
    for name, x in boundary_activations(cuts, batch, "cpu", torch.float32):
        x = x.contiguous()
        b16 = x.bfloat16().view(torch.int16).numpy().view(np.uint16)
        r16 = b16.size * 2 / pack_ref.encoded_bytes(b16)
        r32 = x.numel() * 4 / pack_ref.encoded_bytes(x.numpy())
        z = (x == 0).float().mean().item()
        print(f"{name:9s} {str(tuple(x.shape)):20s} {z*100:5.1f}% "
              f"{r16:6.2f}x {r32:6.2f}x")


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="zfp",
                    choices=["zfp", "lossless", "lossless-ratio"],
                    help="zfp: fixed-rate ZFP + fp8 on randn (default); "
                         "lossless: the lossless wire on real ResNet50 "
                         "boundaries; lossless-ratio: its ratios from the "
                         "numpy spec, no GPU")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    if args.case == "zfp":
        zfp_case()
    elif args.case == "lossless":
        lossless_case(args.batch or 64, args.iters)
    else:
        ratio_case(args.batch or 4)
