"""Measurements for the grouped 3x3 conv kernel (csrc/gconv.hip) and
ResNeXt50, on one GPU.

    python tools/gconvbench.py kernel [--batches 64,256] [--out FILE]
    python tools/gconvbench.py model  [--batches 64,256] [--out FILE]

`kernel` runs the seven grouped-conv geometries of ResNeXt50 32x4d (224x224
input), bf16 and fp32, and times per geometry, alternating in one process:

  gc      ops.gconv2d_bn_act (folded BN, ReLU); TB/s over the bytes it
          needs: input + output + weights
  gc'     the same call again: the run-to-run spread of a repeated contender
  island  what a lowered model ran before the kernel existed: ops.to_nchw,
          torch's grouped conv + BatchNorm + ReLU in NCHW, ops.to_nhwc
  dense   ops.conv2d_bn_act with the weights densified to C x C (zeros
          outside the groups), the only other route on the HIP path
  pool    ops.maxpool2d(3, stride, 1) on the same tensor, the project's
          streaming yardstick with the same footprint

`model` measures img/s of ResNeXt50 32x4d in bf16 through StageExecutor: the
zoo's resnext50_32x4d() (NHWC input), a torchvision-style torch module
lowered onto it (NCHW input), and the same module lowered with the grouped
pattern disabled, so its 16 grouped convs stay TorchIslands between two
layout conversions (the path before this kernel).

Method: tools/dwbench.py's (device events around windows of back-to-back
calls, contenders warmed and alternated over 5 rounds, median with min-max;
in `kernel` mode rings of distinct inputs whose inputs and outputs together
exceed 1 GiB).
"""

import argparse
import sys
from pathlib import Path

import torch
import torch.nn as nn

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import defer_amd.lower as lower_mod  # noqa: E402
from defer_amd import ops  # noqa: E402
from defer_amd.graph import GraphModel  # noqa: E402
from defer_amd.lower import lower_torch, lowering_report  # noqa: E402
from defer_amd.models import resnext50_32x4d  # noqa: E402
from defer_amd.parallel.pipeline import StageExecutor  # noqa: E402
from dwbench import DEV, RING_BYTES, _alternate, _header, _kinds  # noqa: E402

GROUPS = 32
# (H = W of the input, C, stride): the conv2 layers of ResNeXt50 32x4d
GEOMETRIES = [(56, 128, 1), (56, 256, 2), (28, 256, 1), (28, 512, 2),
              (14, 512, 1), (14, 1024, 2), (7, 1024, 1)]


# ------------------------------------------------------------------ kernel
def bench_kernel(batches, out):
    lines = [
        "Grouped 3x3 conv + BN + ReLU (csrc/gconv.hip), 32 groups, the seven "
        "conv2 geometries of", "ResNeXt50 32x4d.",
        "gc TB/s = (input + output + weight bytes) / time, 1 TB = 1e12 B; "
        "gc' is the same call",
        "as a second contender (run-to-run spread); island = ops.to_nchw + "
        "torch grouped conv +",
        "BN + ReLU in NCHW + ops.to_nhwc; dense = ops.conv2d_bn_act with C x "
        "C weights; pool =",
        "ops.maxpool2d(3, s, 1) on the same tensor. Rings of distinct inputs, "
        "inputs + outputs",
        "> 1 GiB per contender."] + _header()
    lines.append(f"{'dtype':<6}{'N':>4} {'HxWxC/s':<14}{'gc ms':>9}"
                 f"{'gc TB/s':>20}{'gc2 ms':>9}{'island ms':>11}"
                 f"{'dense ms':>10}{'pool ms':>9}{'isl/gc':>8}{'dns/gc':>8}"
                 f"{'gc/pool':>9}")
    worst = {}
    for dt, dname in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        esz = 2 if dt == torch.bfloat16 else 4
        for nb in batches:
            for H, C, st in GEOMETRIES:
                cg = C // GROUPS
                OH = (H + 2 - 3) // st + 1
                in_b = nb * H * H * C * esz
                out_b = nb * OH * OH * C * esz
                need = in_b + out_b + 9 * cg * C * esz
                nbuf = max(2, -(-RING_BYTES // (in_b + out_b)))
                xs = [torch.randn(nb, H, H, C, device=DEV).to(dt)
                      for _ in range(nbuf)]
                w = (torch.randn(C, 3, 3, cg, device=DEV)
                     / (3 * cg ** 0.5)).to(dt)
                wd = torch.zeros(C, 3, 3, C, device=DEV, dtype=dt)
                for k in range(0, C, cg):
                    wd[k:k + cg, :, :, k:k + cg] = w[k:k + cg]
                scale = torch.rand(C, device=DEV) + 0.5
                bias = torch.randn(C, device=DEV) * 0.1
                conv = nn.Conv2d(C, C, 3, st, 1, groups=GROUPS, bias=False)
                bn = nn.BatchNorm2d(C)
                island = nn.Sequential(conv, bn, nn.ReLU(inplace=True))
                island = island.eval().to(DEV, dt)
                with torch.no_grad():
                    conv.weight.copy_(w.permute(0, 3, 1, 2))
                    bn.weight.copy_(scale)
                    bn.bias.copy_(bias)
                turn = [0] * 5

                def nxt(i):
                    turn[i] = (turn[i] + 1) % nbuf
                    return xs[turn[i]]

                def gc(i=0):
                    return ops.gconv2d_bn_act(nxt(i), w, scale, bias, st, 1,
                                              "relu")

                def gc2():
                    return gc(1)

                def isl():
                    return ops.to_nhwc(island(ops.to_nchw(nxt(2))))

                def dense():
                    return ops.conv2d_bn_act(nxt(3), wd, scale, bias, st, 1,
                                             "relu")

                def pool():
                    return ops.maxpool2d(nxt(4), 3, st, 1)

                # all three compute the same function (each on xs[1])
                a, b, c = gc().float(), isl().float(), dense().float()
                tol = 0.02 if dt == torch.bfloat16 else 1e-4
                for other in (b, c):
                    rel = ((a - other).abs().max() / other.abs().max()).item()
                    assert rel < tol, rel
                (g, glo, ghi), (g2, _, _), (s, _, _), (d, _, _), (p, _, _) = \
                    _alternate([gc, gc2, isl, dense, pool])

                def tbs(ms):
                    return need / (ms * 1e-3) / 1e12

                lines.append(
                    f"{dname:<6}{nb:>4} {f'{H}x{H}x{C}/s{st}':<14}{g:>9.4f}"
                    f"{f'{tbs(g):.2f} ({tbs(ghi):.2f}-{tbs(glo):.2f})':>20}"
                    f"{g2:>9.4f}{s:>11.4f}{d:>10.4f}{p:>9.4f}{s / g:>8.2f}"
                    f"{d / g:>8.2f}{g / p:>9.2f}")
                print(lines[-1], flush=True)
                k = (dname, nb)
                worst[k] = max(worst.get(k, 0.0), abs(g2 - g) / g)
                del xs, island, wd
    lines.append("")
    for (dname, nb), v in worst.items():
        lines.append(f"largest |gc2 - gc| / gc, {dname} batch {nb}: "
                     f"{100 * v:.1f}%")
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        Path(out).write_text(text)


# ------------------------------------------------------------------- model
class _Bottleneck(nn.Module):
    def __init__(self, cin, planes, stride):
        super().__init__()
        width, cout = planes * 4 // 64 * GROUPS, planes * 4
        self.body = nn.Sequential(
            nn.Conv2d(cin, width, 1, bias=False), nn.BatchNorm2d(width),
            nn.ReLU(inplace=True),
            nn.Conv2d(width, width, 3, stride, 1, groups=GROUPS, bias=False),
            nn.BatchNorm2d(width), nn.ReLU(inplace=True),
            nn.Conv2d(width, cout, 1, bias=False), nn.BatchNorm2d(cout))
        self.down = None
        if stride != 1 or cin != cout:
            self.down = nn.Sequential(
                nn.Conv2d(cin, cout, 1, stride, bias=False),
                nn.BatchNorm2d(cout))

    def forward(self, x):
        return torch.relu(
            self.body(x) + (x if self.down is None else self.down(x)))


class TorchResNeXt50(nn.Module):
    """ResNeXt50 32x4d the way torchvision writes it (NCHW)."""

    def __init__(self, classes=1000):
        super().__init__()
        layers = [nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64),
                  nn.ReLU(inplace=True), nn.MaxPool2d(3, 2, 1)]
        cin = 64
        for planes, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2),
                                       (512, 3, 2)):
            for b in range(blocks):
                layers.append(_Bottleneck(cin, planes,
                                          stride if b == 0 else 1))
                cin = planes * 4
        self.features = nn.Sequential(*layers)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(cin, classes)

    def forward(self, x):
        x = torch.flatten(self.pool(self.features(x)), 1)
        return torch.softmax(self.fc(x), dim=1)


def _lower_with_islands(net, shape):
    """lower_torch with the grouped pattern switched off, for this
    measurement only: the grouped convs stay TorchIslands, as they did
    before the kernel existed."""
    saved = lower_mod._GC_GROUP_CHANNELS
    lower_mod._GC_GROUP_CHANNELS = ()
    try:
        return lower_torch(net, shape)
    finally:
        lower_mod._GC_GROUP_CHANNELS = saved


def bench_model(batches, out):
    lines = ["ResNeXt50 32x4d bf16, 224x224, one GPU, StageExecutor defaults "
             "(fuse=True, chain=True, no hipGraph)."] + _header(0.3)
    for nb in batches:
        torch.manual_seed(0)
        net = TorchResNeXt50().eval()
        shape = (nb, 3, 224, 224)
        g_low = lower_torch(net, shape, strict=True)
        g_isl = _lower_with_islands(net, shape)
        kept = [r for _, r in lowering_report(g_isl) if r != "lowered"]
        zoo = StageExecutor(GraphModel(resnext50_32x4d().graph), DEV,
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
                ("zoo resnext50_32x4d() (NHWC input)",
                 "torch module, lowered (NCHW input)",
                 "torch module, grouped convs as islands",
                 "torch module, lowered, again"), res):
            lines.append(f"batch {nb:>3}  {tag:<40}{ips(m):9.0f} img/s "
                         f"({ips(hi):.0f}-{ips(lo):.0f}), {m:.3f} ms")
        lines.append(f"batch {nb:>3}  islands in the island graph: "
                     f"{len(kept)}; lowered / island speed: "
                     f"{res[2][0] / res[1][0]:.2f}x")
        lines.append(f"batch {nb:>3}  zoo stage graph:     {_kinds(zoo)}")
        lines.append(f"batch {nb:>3}  lowered stage graph: {_kinds(low)}")
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gconvbench measures on the GPU; none found")
    batches = [int(b) for b in args.batches.split(",")]
    with torch.no_grad():
        if args.what == "kernel":
            bench_kernel(batches, args.out)
        else:
            bench_model(batches, args.out)


if __name__ == "__main__":
    main()
