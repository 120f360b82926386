"""Measurements for the torch lowering path (defer_amd.lower), on one GPU.

    python tools/lowerbench.py layout   [--out FILE]
    python tools/lowerbench.py resnet50 [--batch 64] [--out FILE]

`layout` times ops.to_nhwc / ops.to_nchw (csrc/layout.hip) against
PyTorch's x.permute(...).contiguous().to(dtype) on the same tensors and
reports GB/s over bytes read plus bytes written.

`resnet50` lowers a ResNet50 written as a plain torch module (torchvision
style: NCHW, one shared self.relu per block, `out += identity`) and runs
it beside the zoo's resnet50 through the same StageExecutor, bf16.

Method (both): device events around a window of back-to-back calls that
ends in a synchronise; every shape is warmed first; the window is sized
to at least 0.2 s; the two contenders alternate over 5 rounds in one
process and the median round is reported with the min-max spread.
"""

import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn as nn

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from defer_amd import ops  # noqa: E402
from defer_amd.graph import GraphModel  # noqa: E402
from defer_amd.lower import lower_torch, lowering_report  # noqa: E402
from defer_amd.models import resnet50  # noqa: E402
from defer_amd.parallel.pipeline import StageExecutor  # noqa: E402

DEV = "cuda:0"


def _window_ms(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _alternate(fns, rounds=5, min_window_s=0.2):
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


# ------------------------------------------------------------------ layout
RING_BYTES = 1 << 30       # inputs + outputs a ring of tensors must exceed

LAYOUT_SHAPES = [
    ((256, 3, 224, 224), torch.float32, torch.bfloat16),
    ((256, 64, 56, 56), torch.bfloat16, torch.bfloat16),
    ((256, 2048, 7, 7), torch.bfloat16, torch.bfloat16),
]


def bench_layout(out):
    lines = [
        "NCHW <-> NHWC conversion: ops.to_nhwc / ops.to_nchw "
        "(csrc/layout.hip) against",
        "x.permute(...).contiguous().to(dtype) of PyTorch on the same "
        "tensors.",
        f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
        "method: device events around a window of back-to-back calls "
        "(>= 0.2 s, ends in a",
        "synchronise), every shape warmed first, the two contenders "
        "alternating over 5 rounds in",
        "one process; median round, (min-max) in brackets. GB/s = (bytes "
        "read + bytes written) /",
        "time, 1 GB = 1e9 B. One session; not a kernel-trace figure (launch "
        "gaps are inside).",
        "Each contender walks a ring of distinct input tensors whose "
        "inputs and outputs together",
        "exceed 1 GiB, four times the 256 MiB Infinity Cache, so no call "
        "finds its input cached",
        "(outputs are fresh allocations that the caching allocator may "
        "hand back).",
        "",
        f"{'NCHW shape':<18}{'dtypes':<14}{'dir':<9}{'HIP ms':>9}"
        f"{'HIP GB/s':>22}{'torch ms':>10}{'torch GB/s':>22}",
    ]
    name = {torch.float32: "fp32", torch.bfloat16: "bf16"}
    for shape, src, dst in LAYOUT_SHAPES:
        n = 1
        for d in shape:
            n *= d
        nbytes = n * (torch.finfo(src).bits + torch.finfo(dst).bits) // 8
        nbuf = max(2, -(-RING_BYTES // nbytes))
        xs = [torch.randn(*shape, device=DEV).to(src) for _ in range(nbuf)]
        xhs = [x.permute(0, 2, 3, 1).contiguous() for x in xs]
        for tag, op, ring, perm in (("to_nhwc", ops.to_nhwc, xs,
                                     (0, 2, 3, 1)),
                                    ("to_nchw", ops.to_nchw, xhs,
                                     (0, 3, 1, 2))):
            want = ring[0].permute(*perm).contiguous().to(dst)
            assert torch.equal(op(ring[0], dst), want)
            turn = [0, 0]

            def hip(ring=ring, op=op):
                turn[0] = (turn[0] + 1) % nbuf
                return op(ring[turn[0]], dst)

            def eager(ring=ring, perm=perm):
                turn[1] = (turn[1] + 1) % nbuf
                return ring[turn[1]].permute(*perm).contiguous().to(dst)

            (h, hlo, hhi), (t, tlo, thi) = _alternate([hip, eager])

            def gbs(ms):
                return nbytes / (ms * 1e-3) / 1e9

            lines.append(
                f"{'x'.join(map(str, shape)):<18}"
                f"{name[src] + '->' + name[dst]:<14}{tag:<9}{h:>9.4f}"
                f"{f'{gbs(h):.0f} ({gbs(hhi):.0f}-{gbs(hlo):.0f})':>22}"
                f"{t:>10.4f}"
                f"{f'{gbs(t):.0f} ({gbs(thi):.0f}-{gbs(tlo):.0f})':>22}")
        del xs, xhs
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        Path(out).write_text(text)


# ---------------------------------------------------------------- resnet50
class Bottleneck(nn.Module):
    def __init__(self, cin, width, stride):
        super().__init__()
        cout = width * 4
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(
                nn.Conv2d(cin, cout, 1, stride, bias=False),
                nn.BatchNorm2d(cout))

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


class TorchResNet50(nn.Module):
    def __init__(self, classes=1000):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        blocks, cin = [], 64
        for i, (n, width) in enumerate(zip((3, 4, 6, 3),
                                           (64, 128, 256, 512))):
            for b in range(n):
                blocks.append(Bottleneck(cin, width,
                                         2 if b == 0 and i > 0 else 1))
                cin = width * 4
        self.layers = nn.Sequential(*blocks)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(cin, classes)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.avgpool(self.layers(x))
        return torch.softmax(self.fc(torch.flatten(x, 1)), dim=1)


def _fired(ex):
    counts = {}
    for n in ex.model.graph.nodes:
        k = type(n.layer).__name__
        counts[k] = counts.get(k, 0) + 1
    return counts


def bench_resnet50(batch, out):
    torch.manual_seed(0)
    net = TorchResNet50().eval()
    graph = lower_torch(net, (batch, 3, 224, 224))
    kept = [(n, r) for n, r in lowering_report(graph) if r != "lowered"]
    low = StageExecutor(GraphModel(graph), DEV, torch.bfloat16)
    zoo = StageExecutor(GraphModel(resnet50().graph), DEV, torch.bfloat16)
    xl = torch.randn(batch, 3, 224, 224, device=DEV, dtype=torch.bfloat16)
    xz = xl.permute(0, 2, 3, 1).contiguous()
    (l, llo, lhi), (z, zlo, zhi) = _alternate(
        [lambda: low.run(xl), lambda: zoo.run(xz)])

    def ips(ms):
        return batch / (ms * 1e-3)

    lines = [
        f"ResNet50 bf16, batch {batch}, one GPU, StageExecutor defaults "
        "(fuse=True, chain=True, no hipGraph);",
        f"device: {torch.cuda.get_device_name(0)}; same timing method as "
        "`layout` (see the module docstring).",
        f"zoo resnet50 (NHWC input):            {ips(z):9.0f} img/s "
        f"({ips(zhi):.0f}-{ips(zlo):.0f}), {z:.3f} ms",
        f"plain torch ResNet50, lowered (NCHW): {ips(l):9.0f} img/s "
        f"({ips(lhi):.0f}-{ips(llo):.0f}), {l:.3f} ms",
        f"nodes kept as torch code: {kept}",
        f"zoo stage graph after the passes:     {_fired(zoo)}",
        f"lowered stage graph after the passes: {_fired(low)}",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        Path(out).write_text(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("what", choices=["layout", "resnet50"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lowerbench measures on the GPU; none found")
    with torch.no_grad():
        if args.what == "layout":
            bench_layout(args.out)
        else:
            bench_resnet50(args.batch, args.out)


if __name__ == "__main__":
    main()
