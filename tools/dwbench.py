"""Measurements for the depthwise conv kernel (csrc/dwconv.hip) and
MobileNetV2, on one GPU.

    python tools/dwbench.py kernel [--batches 64,256] [--out FILE]
    python tools/dwbench.py kernel --geoms v3_5x5 [...]
    python tools/dwbench.py model  [--batches 64,256] [--out FILE]

`kernel` runs the ten depthwise geometries of MobileNetV2 (224x224 input),
bf16 and fp32, and times per geometry, alternating in one process:

  dw      ops.dwconv2d_bn_act (3x3, folded BN, ReLU6); GB/s over the bytes
          it needs: input + output + weights
  dw'     the same call again: the run-to-run spread of a repeated contender
  pool    ops.maxpool2d(3, stride, 1) on the same tensor, the project's
          streaming yardstick with the same footprint
  island  what a lowered model ran before the kernel existed: ops.to_nchw,
          torch's depthwise conv + BatchNorm + ReLU6 in NCHW, ops.to_nhwc

`--geoms v3_5x5` runs the 5x5 depthwise geometries of MobileNetV3-Large
instead (its seven 5x5 layers have four distinct geometries), with the
activation each has there.

`model` measures img/s of MobileNetV2 in bf16 through StageExecutor: the
zoo's mobilenet_v2() (NHWC input), a torchvision-style torch module lowered
onto it (NCHW input), and the same module lowered with the depthwise and
ReLU6 patterns disabled, so those layers stay TorchIslands between two
layout conversions (the path before this kernel).

Method (the conventions of tools/lowerbench.py): device events around a
window of back-to-back calls that ends in a synchronise; every contender is
warmed first; the contenders alternate over 5 rounds in one process and the
median round is reported with the min-max spread. In `kernel` mode every
contender walks a ring of distinct input tensors whose inputs and outputs
together exceed 1 GiB, four times the 256 MiB Infinity Cache.
"""

import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import defer_amd.lower as lower_mod  # noqa: E402
from defer_amd import ops  # noqa: E402
from defer_amd.graph import GraphModel  # noqa: E402
from defer_amd.lower import lower_torch, lowering_report  # noqa: E402
from defer_amd.models import mobilenet_v2  # noqa: E402
from defer_amd.models.mobilenet import MOBILENET_V2_TABLE  # noqa: E402
from defer_amd.parallel.pipeline import StageExecutor  # noqa: E402

DEV = "cuda:0"
RING_BYTES = 1 << 30

# (H = W of the input, C, stride): the depthwise layers of MobileNetV2
GEOMETRIES = [(112, 32, 1), (112, 96, 2), (56, 144, 1), (56, 144, 2),
              (28, 192, 1), (28, 192, 2), (14, 384, 1), (14, 576, 1),
              (14, 576, 2), (7, 960, 1)]
# (H = W, C, stride, act) of the 5x5 depthwise layers of MobileNetV3-Large:
# blocks 3; 4 and 5; 12; 13 and 14
GEOMETRIES_V3_5X5 = [(56, 72, 2, "relu"), (28, 120, 1, "relu"),
                     (14, 672, 2, "hardswish"), (7, 960, 1, "hardswish")]
_TORCH_ACTS = {"relu6": nn.ReLU6, "relu": nn.ReLU, "hardswish": nn.Hardswish}


def _window_ms(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _alternate(fns, rounds=5, min_window_s=0.1):
    """Per-call ms of each fn: median over `rounds` alternating windows,
    with (min, max)."""
    iters = []
    for fn in fns:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        one = _window_ms(fn, 5)
        iters.append(max(10, int(min_window_s * 1e3 / max(one, 1e-3))))
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            ms[i].append(_window_ms(fn, iters[i]))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def _header(min_window_s=0.1):
    return [f"device: {torch.cuda.get_device_name(0)}, torch "
            f"{torch.__version__}",
            "method: device events around windows of back-to-back calls "
            f"(>= {min_window_s} s, ending in a",
            "synchronise), contenders warmed and alternated over 5 rounds in "
            "one process; median",
            "round, (min-max) in brackets. One session; launch gaps are "
            "inside the figures.", ""]


# ------------------------------------------------------------------ kernel
def bench_kernel(batches, out, geoms="v2"):
    if geoms == "v2":
        R, todo = 3, [g + ("relu6",) for g in GEOMETRIES]
        what = ["Depthwise 3x3 conv + BN + ReLU6 (csrc/dwconv.hip), the ten "
                "depthwise geometries of", "MobileNetV2."]
    else:
        R, todo = 5, GEOMETRIES_V3_5X5
        what = ["Depthwise 5x5 conv + BN + ReLU or hardswish "
                "(csrc/dwconv.hip), the 5x5 depthwise",
                "geometries of MobileNetV3-Large."]
    P = R // 2
    lines = what + [
        "dw GB/s = (input + output + weight bytes) / time, 1 GB = 1e9 B; "
        "dw' is the same call",
        "as a second contender (run-to-run spread); pool = "
        "ops.maxpool2d(3, s, 1) on the same",
        "tensor; island = ops.to_nchw + torch depthwise conv + BN + the "
        "activation in NCHW +",
        "ops.to_nhwc. Rings of distinct inputs, inputs + outputs > 1 GiB "
        "per contender."] + _header()
    lines.append(f"{'dtype':<6}{'N':>4} {'HxWxC/s':<14}{'dw ms':>9}"
                 f"{'dw GB/s':>20}{'dw2 ms':>9}{'pool ms':>9}"
                 f"{'island ms':>11}{'isl/dw':>8}{'dw/pool':>9}")
    worst = {}
    for dt, dname in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        esz = 2 if dt == torch.bfloat16 else 4
        for nb in batches:
            for H, C, st, act in todo:
                OH = (H + 2 * P - R) // st + 1
                in_b = nb * H * H * C * esz
                out_b = nb * OH * OH * C * esz
                need = in_b + out_b + R * R * C * esz
                nbuf = max(2, -(-RING_BYTES // (in_b + out_b)))
                xs = [torch.randn(nb, H, H, C, device=DEV).to(dt)
                      for _ in range(nbuf)]
                w = (torch.randn(R, R, C, device=DEV) / R).to(dt)
                scale = torch.rand(C, device=DEV) + 0.5
                bias = torch.randn(C, device=DEV) * 0.1
                conv = nn.Conv2d(C, C, R, st, P, groups=C, bias=False)
                bn = nn.BatchNorm2d(C)
                island = nn.Sequential(conv, bn,
                                       _TORCH_ACTS[act](inplace=True))
                island = island.eval().to(DEV, dt)
                with torch.no_grad():
                    conv.weight.copy_(w.permute(2, 0, 1).unsqueeze(1))
                    bn.weight.copy_(scale)
                    bn.bias.copy_(bias)
                turn = [0, 0, 0, 0]

                def nxt(i):
                    turn[i] = (turn[i] + 1) % nbuf
                    return xs[turn[i]]

                def dw(i=0):
                    return ops.dwconv2d_bn_act(nxt(i), w, scale, bias, st, P,
                                               act)

                def dw2():
                    return dw(1)

                def pool():
                    return ops.maxpool2d(nxt(2), 3, st, 1)

                def isl():
                    return ops.to_nhwc(island(ops.to_nchw(nxt(3))))

                # the island computes the same function
                a, b = dw().float(), isl().float()     # both on xs[1]
                rel = ((a - b).abs().max() / b.abs().max()).item()
                assert rel < (0.02 if dt == torch.bfloat16 else 1e-4), rel
                (d, dlo, dhi), (d2, _, _), (p, _, _), (s, _, _) = \
                    _alternate([dw, dw2, pool, isl])

                def gbs(ms):
                    return need / (ms * 1e-3) / 1e9

                lines.append(
                    f"{dname:<6}{nb:>4} {f'{H}x{H}x{C}/s{st}':<14}{d:>9.4f}"
                    f"{f'{gbs(d):.0f} ({gbs(dhi):.0f}-{gbs(dlo):.0f})':>20}"
                    f"{d2:>9.4f}{p:>9.4f}{s:>11.4f}{s / d:>8.2f}"
                    f"{d / p:>9.2f}")
                print(lines[-1], flush=True)
                k = (dname, nb)
                worst[k] = max(worst.get(k, 0.0), abs(d2 - d) / d)
                del xs, island
    lines.append("")
    for (dname, nb), v in worst.items():
        lines.append(f"largest |dw2 - dw| / dw, {dname} batch {nb}: "
                     f"{100 * v:.1f}%")
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        Path(out).write_text(text)


# ------------------------------------------------------------------- model
class _CNA(nn.Sequential):
    def __init__(self, cin, cout, k=3, stride=1, groups=1):
        super().__init__(
            nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups,
                      bias=False),
            nn.BatchNorm2d(cout), nn.ReLU6(inplace=True))


class _InvertedResidual(nn.Module):
    def __init__(self, inp, oup, stride, t):
        super().__init__()
        hidden = inp * t
        self.use_res_connect = stride == 1 and inp == oup
        layers = [] if t == 1 else [_CNA(inp, hidden, 1)]
        layers += [_CNA(hidden, hidden, 3, stride, hidden),
                   nn.Conv2d(hidden, oup, 1, bias=False),
                   nn.BatchNorm2d(oup)]
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.conv(x) if self.use_res_connect else self.conv(x)


class TorchMobileNetV2(nn.Module):
    """MobileNetV2 the way torchvision writes it (NCHW, ReLU6(inplace=True),
    F.adaptive_avg_pool2d + torch.flatten)."""

    def __init__(self, classes=1000):
        super().__init__()
        feats, cin = [_CNA(3, 32, 3, 2)], 32
        for t, c, n, s in MOBILENET_V2_TABLE:
            for i in range(n):
                feats.append(_InvertedResidual(cin, c, s if i == 0 else 1, t))
                cin = c
        feats.append(_CNA(cin, 1280, 1))
        self.features = nn.Sequential(*feats)
        self.classifier = nn.Sequential(nn.Dropout(0.2),
                                        nn.Linear(1280, classes))

    def forward(self, x):
        x = F.adaptive_avg_pool2d(self.features(x), (1, 1))
        return torch.softmax(self.classifier(torch.flatten(x, 1)), dim=1)


def _lower_with_islands(net, shape):
    """lower_torch with the depthwise and ReLU6 patterns switched off, for
    this measurement only: the depthwise convs and the ReLU6s stay
    TorchIslands, as they did before the kernel existed."""
    saved = lower_mod._DW_KERNELS, lower_mod._Lowering.is_relu6
    lower_mod._DW_KERNELS = ()
    lower_mod._Lowering.is_relu6 = lambda self, n, of: False
    try:
        return lower_torch(net, shape)
    finally:
        lower_mod._DW_KERNELS, lower_mod._Lowering.is_relu6 = saved


def _kinds(ex):
    counts = {}
    for n in ex.model.graph.nodes:
        k = type(n.layer).__name__
        counts[k] = counts.get(k, 0) + 1
    return counts


def bench_model(batches, out):
    lines = ["MobileNetV2 bf16, 224x224, one GPU, StageExecutor defaults "
             "(fuse=True, chain=True, no hipGraph)."] + _header(0.3)
    for nb in batches:
        torch.manual_seed(0)
        net = TorchMobileNetV2().eval()
        shape = (nb, 3, 224, 224)
        g_low = lower_torch(net, shape, strict=True)
        g_isl = _lower_with_islands(net, shape)
        kept = [r for _, r in lowering_report(g_isl) if r != "lowered"]
        zoo = StageExecutor(GraphModel(mobilenet_v2().graph), DEV,
                            torch.bfloat16)
        low = StageExecutor(GraphModel(g_low), DEV, torch.bfloat16)
        isl = StageExecutor(GraphModel(g_isl), DEV, torch.bfloat16)
        x = torch.randn(*shape, device=DEV, dtype=torch.bfloat16)
        xz = x.permute(0, 2, 3, 1).contiguous()
        a, b = low.run(x).float(), isl.run(x).float()
        assert (a - b).abs().max().item() < 0.05, "island path differs"
        res = _alternate([lambda: zoo.run(xz), lambda: low.run(x),
                          lambda: isl.run(x), lambda: low.run(x)],
                         min_window_s=0.3)

        def ips(ms):
            return nb / (ms * 1e-3)

        for tag, (m, lo, hi) in zip(
                ("zoo mobilenet_v2() (NHWC input)",
                 "torch module, lowered (NCHW input)",
                 "torch module, dw + ReLU6 as islands",
                 "torch module, lowered, again"), res):
            lines.append(f"batch {nb:>3}  {tag:<38}{ips(m):9.0f} img/s "
                         f"({ips(hi):.0f}-{ips(lo):.0f}), {m:.3f} ms")
        lines.append(f"batch {nb:>3}  islands in the island graph: "
                     f"{len(kept)}; lowered / island speed: "
                     f"{res[2][0] / res[1][0]:.2f}x")
        lines.append(f"batch {nb:>3}  lowered stage graph: {_kinds(low)}")
        lines.append(f"batch {nb:>3}  island stage graph:  {_kinds(isl)}")
        lines.append("")
        print("\n".join(lines[-8:]), flush=True)
        del zoo, low, isl
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        Path(out).write_text(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("what", choices=["kernel", "model"])
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--geoms", choices=["v2", "v3_5x5"], default="v2",
                    help="kernel mode: MobileNetV2's 3x3 geometries or "
                         "MobileNetV3-Large's 5x5 ones")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dwbench measures on the GPU; none found")
    batches = [int(b) for b in args.batches.split(",")]
    with torch.no_grad():
        if args.what == "kernel":
            bench_kernel(batches, args.out, args.geoms)
        else:
            bench_model(batches, args.out)


if __name__ == "__main__":
    main()
