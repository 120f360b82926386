"""Measurements for the squeeze-excite kernels (csrc/se.hip) and
MobileNetV3-Large, on one GPU.

    python tools/sebench.py kernel [--batches 64,256] [--out FILE]
    python tools/sebench.py model  [--batches 64,256] [--out FILE]

`kernel` runs the squeeze-excite geometries of MobileNetV3-Large (224x224
input; its eight blocks have six distinct geometries), bf16 and fp32, and
times per geometry, alternating in one process:

  se      ops.squeeze_excite (both launches); TB/s over the bytes it needs:
          x read twice and y written once
  se'     the same call again: the run-to-run spread of a repeated contender
  gate    ops.se_gate alone (pool and both FCs, one read of x)
  scale   ops.channel_scale alone (one read of x, one write of y)
  relu6   ops.relu6 on the same tensor: it moves the bytes of the scale pass
          and is the streaming yardstick
  island  what a lowered model ran before the kernels existed: ops.to_nchw,
          torch's pool / conv / relu / conv / hardsigmoid / mul in NCHW,
          ops.to_nhwc
  comp    the composition of the ops that existed: ops.global_avg_pool,
          ops.linear twice, and the relu, hardsigmoid and broadcast multiply
          in torch (NHWC)

scale/relu6 is the scale pass against the yardstick; gate/read is the gate
pass against one read of x at the rate relu6 reaches (half its time).

`model` measures img/s of MobileNetV3-Large in bf16 through StageExecutor:
the zoo's mobilenet_v3_large() (NHWC input), a torchvision-style torch
module lowered onto it (NCHW input), and the same module lowered with the
squeeze-excite and hardswish patterns disabled, so those layers stay
TorchIslands between two layout conversions (the path before these kernels).

Method: that of tools/dwbench.py, whose helpers this uses.
"""

import argparse
import sys
from pathlib import Path

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import defer_amd.lower as lower_mod  # noqa: E402
from defer_amd import ops  # noqa: E402
from defer_amd.graph import GraphModel  # noqa: E402
from defer_amd.lower import lower_torch, lowering_report  # noqa: E402
from defer_amd.models import mobilenet_v3_large  # noqa: E402
from defer_amd.models.mobilenet import (MOBILENET_V3_LARGE_TABLE,  # noqa: E402
                                        make_divisible)
from defer_amd.parallel.pipeline import StageExecutor  # noqa: E402
from dwbench import DEV, RING_BYTES, _alternate, _header, _kinds  # noqa: E402

# (H = W, C, Cr): the squeeze-excite blocks of MobileNetV3-Large at 224x224
# (blocks 3; 4 and 5; 10; 11; 12; 13 and 14)
GEOMETRIES = [(28, 72, 24), (28, 120, 32), (14, 480, 120), (14, 672, 168),
              (7, 672, 168), (7, 960, 240)]


class _TorchSE(nn.Module):
    """torchvision.ops.misc.SqueezeExcitation."""

    def __init__(self, c, cr):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(c, cr, 1)
        self.fc2 = nn.Conv2d(cr, c, 1)
        self.activation = nn.ReLU()
        self.scale_activation = nn.Hardsigmoid()

    def forward(self, x):
        s = self.fc2(self.activation(self.fc1(self.avgpool(x))))
        return self.scale_activation(s) * x


# ------------------------------------------------------------------ kernel
def bench_kernel(batches, out):
    lines = ["Squeeze-excite (csrc/se.hip), the squeeze-excite geometries of "
             "MobileNetV3-Large.",
             "se TB/s = 3 * (bytes of x) / time (x read twice, y written "
             "once), 1 TB = 1e12 B; se' is",
             "the same call as a second contender (run-to-run spread); gate "
             "and scale are the two",
             "launches apart; relu6 = ops.relu6 on the same tensor; island = "
             "ops.to_nchw + torch",
             "pool / conv / relu / conv / hardsigmoid / mul in NCHW + "
             "ops.to_nhwc; comp =",
             "ops.global_avg_pool + ops.linear twice, the rest in torch. "
             "gate/read = gate time over",
             "half the relu6 time (one read of x at relu6's rate). Rings of "
             "distinct inputs, inputs +",
             "outputs > 1 GiB per contender; times in ms."] + _header()
    lines.append(f"{'dtype':<6}{'N':>4} {'HxWxC/Cr':<15}{'se':>8}"
                 f"{'se TB/s':>19}{'se2':>8}{'gate':>8}{'scale':>8}"
                 f"{'relu6':>8}{'island':>8}{'comp':>8}{'isl/se':>7}"
                 f"{'comp/se':>8}{'scale/relu6':>12}{'gate/read':>10}")
    worst, verdicts = {}, []
    for dt, dname in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        esz = 2 if dt == torch.bfloat16 else 4
        for nb in batches:
            for H, C, Cr in GEOMETRIES:
                x_b = nb * H * H * C * esz
                nbuf = max(2, -(-RING_BYTES // (2 * x_b)))
                xs = [torch.randn(nb, H, H, C, device=DEV).to(dt)
                      for _ in range(nbuf)]
                island = _TorchSE(C, Cr).eval().to(DEV, dt)
                w1 = island.fc1.weight.detach().view(Cr, C).contiguous()
                w2 = island.fc2.weight.detach().view(C, Cr).contiguous()
                b1 = island.fc1.bias.detach().float().contiguous()
                b2 = island.fc2.bias.detach().float().contiguous()
                g0 = ops.se_gate(xs[0], w1, b1, w2, b2)
                turn = [0] * 7

                def nxt(i):
                    turn[i] = (turn[i] + 1) % nbuf
                    return xs[turn[i]]

                def se(i=0):
                    return ops.squeeze_excite(nxt(i), w1, b1, w2, b2)

                def se2():
                    return se(1)

                def gate():
                    return ops.se_gate(nxt(2), w1, b1, w2, b2)

                def scale():
                    return ops.channel_scale(nxt(3), g0)

                def relu6():
                    return ops.relu6(nxt(4))

                def isl():
                    return ops.to_nhwc(island(ops.to_nchw(nxt(5))))

                def comp():
                    x = nxt(6)
                    z = torch.relu(ops.linear(ops.global_avg_pool(x), w1, b1))
                    g = F.hardsigmoid(ops.linear(z, w2, b2))
                    return x * g[:, None, None, :]

                # the contenders compute the same function (all on xs[1])
                a = se().float()
                for other in (isl, comp):
                    turn[5] = turn[6] = 0
                    b = other().float()
                    rel = ((a - b).abs().max() / b.abs().max()).item()
                    assert rel < (0.02 if dt == torch.bfloat16 else 1e-4), rel
                res = _alternate([se, se2, gate, scale, relu6, isl, comp])
                (d, dlo, dhi), (d2, _, _) = res[0], res[1]
                gt, sc, r6, il, cp = (r[0] for r in res[2:])

                def tbs(ms):
                    return 3 * x_b / (ms * 1e-3) / 1e12

                lines.append(
                    f"{dname:<6}{nb:>4} {f'{H}x{H}x{C}/{Cr}':<15}{d:>8.4f}"
                    f"{f'{tbs(d):.2f} ({tbs(dhi):.2f}-{tbs(dlo):.2f})':>19}"
                    f"{d2:>8.4f}{gt:>8.4f}{sc:>8.4f}{r6:>8.4f}{il:>8.4f}"
                    f"{cp:>8.4f}{il / d:>7.2f}{cp / d:>8.2f}{sc / r6:>12.2f}"
                    f"{gt / (r6 / 2):>10.2f}")
                print(lines[-1], flush=True)
                k = (dname, nb)
                spread = abs(d2 - d) / d
                worst[k] = max(worst.get(k, 0.0), spread)
                verdicts.append((dname, nb, f"{H}x{H}x{C}", spread,
                                 il / d, cp / d, gt / (r6 / 2)))
                del xs, island
    lines.append("")
    for (dname, nb), v in worst.items():
        lines.append(f"largest |se2 - se| / se, {dname} batch {nb}: "
                     f"{100 * v:.1f}%")
    slow = [v for v in verdicts if min(v[4], v[5]) <= 1 + v[3]]
    lines.append("squeeze_excite faster than both compositions by more than "
                 "the spread of the repeated contender: "
                 + ("every geometry and dtype" if not slow else
                    "NOT for " + ", ".join(f"{d} N={n} {g}"
                                           for d, n, g, *_ in slow)))
    over = [v for v in verdicts if v[1] == min(batches) and v[6] > 2]
    lines.append(f"gate pass more than 2x one read of x at batch "
                 f"{min(batches)}: "
                 + (", ".join(f"{d} {g} ({r:.1f}x)"
                              for d, _, g, _, _, _, r in over) or "none"))
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        Path(out).write_text(text)


# ------------------------------------------------------------------- model
class _CNA(nn.Sequential):
    def __init__(self, cin, cout, k=3, stride=1, groups=1, act=nn.Hardswish):
        layers = [nn.Conv2d(cin, cout, k, stride, (k - 1) // 2,
                            groups=groups, bias=False),
                  nn.BatchNorm2d(cout)]
        if act is not None:
            layers.append(act(inplace=True))
        super().__init__(*layers)


class _InvertedResidual(nn.Module):
    def __init__(self, inp, kernel, hidden, oup, se, act, stride):
        super().__init__()
        self.use_res_connect = stride == 1 and inp == oup
        layers = [] if hidden == inp else [_CNA(inp, hidden, 1, act=act)]
        layers.append(_CNA(hidden, hidden, kernel, stride, hidden, act))
        if se:
            layers.append(_TorchSE(hidden, make_divisible(hidden / 4)))
        layers.append(_CNA(hidden, oup, 1, act=None))
        self.block = nn.Sequential(*layers)

    def forward(self, x):
        y = self.block(x)
        if self.use_res_connect:
            y += x
        return y


class TorchMobileNetV3Large(nn.Module):
    """MobileNetV3-Large the way torchvision writes it (NCHW, in-place
    Hardswish, SqueezeExcitation, avgpool + flatten + Linear + Hardswish)."""

    def __init__(self, classes=1000):
        super().__init__()
        feats, cin = [_CNA(3, 16, 3, 2)], 16
        for k, hidden, c, se, act, s in MOBILENET_V3_LARGE_TABLE:
            feats.append(_InvertedResidual(
                cin, k, hidden, c, se,
                nn.Hardswish if act == "hardswish" else nn.ReLU, s))
            cin = c
        feats.append(_CNA(cin, 960, 1))
        self.features = nn.Sequential(*feats)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(
            nn.Linear(960, 1280), nn.Hardswish(inplace=True),
            nn.Dropout(0.2, inplace=True), nn.Linear(1280, classes))

    def forward(self, x):
        x = torch.flatten(self.avgpool(self.features(x)), 1)
        return torch.softmax(self.classifier(x), dim=1)


def _lower_with_islands(net, shape):
    """lower_torch with the squeeze-excite and hardswish patterns switched
    off, for this measurement only: those layers stay TorchIslands, as they
    did before the kernels existed."""
    cls = lower_mod._Lowering
    saved = cls.is_hardswish, cls.is_pool_to_1x1
    cls.is_hardswish = lambda self, n, of: False
    cls.is_pool_to_1x1 = lambda self, n: False
    try:
        return lower_torch(net, shape)
    finally:
        cls.is_hardswish, cls.is_pool_to_1x1 = saved


def _kinds_of(graph):
    counts = {}
    for n in graph.nodes:
        k = type(n.layer).__name__
        counts[k] = counts.get(k, 0) + 1
    return counts


def bench_model(batches, out):
    lines = ["MobileNetV3-Large bf16, 224x224, one GPU, StageExecutor "
             "defaults (fuse=True, chain=True, no hipGraph)."] + _header(0.3)
    for nb in batches:
        torch.manual_seed(0)
        net = TorchMobileNetV3Large().eval()
        shape = (nb, 3, 224, 224)
        g_low = lower_torch(net, shape, strict=True)
        g_isl = _lower_with_islands(net, shape)
        kept = [r for _, r in lowering_report(g_isl) if r != "lowered"]
        # 21 hardswishes and 8 x (pool, hardsigmoid, mul): if the patterns
        # switched off above are renamed, this is no longer the old path
        assert len(kept) == 45 and not _kinds_of(g_low).get("TorchIsland"), \
            (len(kept), _kinds_of(g_low))
        zoo = StageExecutor(GraphModel(mobilenet_v3_large().graph), DEV,
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
                ("zoo mobilenet_v3_large() (NHWC input)",
                 "torch module, lowered (NCHW input)",
                 "torch module, SE + hardswish as islands",
                 "torch module, lowered, again"), res):
            lines.append(f"batch {nb:>3}  {tag:<42}{ips(m):9.0f} img/s "
                         f"({ips(hi):.0f}-{ips(lo):.0f}), {m:.3f} ms")
        spread = abs(res[3][0] - res[1][0]) / res[1][0]
        ratio = res[2][0] / res[1][0]
        lines.append(f"batch {nb:>3}  islands in the island graph: "
                     f"{len(kept)}; lowered / island speed: {ratio:.2f}x; "
                     f"spread of the repeated contender {100 * spread:.1f}%: "
                     + ("faster by more than the spread"
                        if ratio > 1 + spread else "NOT faster by more than "
                        "the spread"))
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sebench measures on the GPU; none found")
    batches = [int(b) for b in args.batches.split(",")]
    with torch.no_grad():
        if args.what == "kernel":
            bench_kernel(batches, args.out)
        else:
            bench_model(batches, args.out)


if __name__ == "__main__":
    main()
