"""Measurements for the ConvNeXt kernels (csrc/dwconv7.hip,
csrc/layernorm.hip, the GELU epilogues of csrc/conv.hip) and convnext_tiny(),
on one GPU.

    python tools/convnextbench.py kernel [--batches 64,256] [--out FILE]
    python tools/convnextbench.py model  [--batches 64,256] [--out FILE]

`kernel` runs the four block geometries of ConvNeXt-Tiny at 224x224, bf16
and fp32, and times per geometry, alternating in one process:

  dw      ops.dwconv7x7; TB/s over one read of x and one write of y
  dw'     the same call again: the run-to-run spread of a repeated contender
  isl     the island: ops.to_nchw, torch's depthwise conv, ops.to_nhwc
  pool    ops.maxpool2d(3, 1, 1) on the same tensor, the streaming yardstick
  ln      ops.layernorm_channels (ln' again)
  relu6   ops.relu6 on the same tensor, the yardstick of one pass
  tln     torch's F.layer_norm on the NHWC tensor
  lg      ops.linear_gelu, C -> 4C (lg' again)
  cg      ops.conv2d_bn_act(act="none") as a 1x1 conv, then torch's GELU

`model` measures img/s of convnext_tiny() in bf16 through StageExecutor
against the same graph with the three new layers swapped for those torch
compositions, and prints the stage graph.

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

from defer_amd import ops  # noqa: E402
from defer_amd.graph import GraphModel, GraphNode, LayerGraph  # noqa: E402
from defer_amd.models import convnext_tiny  # noqa: E402
from defer_amd.models.layers import (DepthwiseConv7x7, LayerNormC,  # noqa: E402
                                     PointwiseGelu)
from defer_amd.parallel.pipeline import StageExecutor  # noqa: E402
from dwbench import DEV, RING_BYTES, _alternate, _header, _kinds  # noqa: E402

# (H = W, C) of the blocks of the four stages at 224x224
GEOMETRIES = [(56, 96), (28, 192), (14, 384), (7, 768)]


def _dw_island(x, w, bias):
    """w is [C, 1, 7, 7], torch's layout, in x's dtype."""
    y = F.conv2d(ops.to_nchw(x), w, bias.to(x.dtype), padding=3,
                 groups=x.shape[-1])
    return ops.to_nhwc(y)


def _ln_torch(x, weight, bias, eps=1e-6):
    return F.layer_norm(x, (x.shape[-1],), weight.to(x.dtype),
                        bias.to(x.dtype), eps)


def _gelu_composed(x, w, bias):
    w4 = w.view(w.shape[0], 1, 1, w.shape[1])
    return F.gelu(ops.conv2d_bn_act(x, w4, None, bias, 1, 0, "none"))


# ------------------------------------------------------------------ kernel
def bench_kernel(batches, out):
    lines = ["ConvNeXt-Tiny block geometries at 224x224. dw = ops.dwconv7x7, "
             "isl = ops.to_nchw + torch",
             "depthwise conv + ops.to_nhwc, pool = ops.maxpool2d(3, 1, 1); ln "
             "= ops.layernorm_channels,",
             "relu6 = ops.relu6, tln = F.layer_norm on the NHWC tensor; lg = "
             "ops.linear_gelu C -> 4C,",
             "cg = ops.conv2d_bn_act(1x1, none) + F.gelu. x' is x again (the "
             "run-to-run spread). dw TB/s",
             "= 2 * (bytes of x) / time. Rings of distinct inputs, inputs + "
             "outputs > 1 GiB; times in ms."] + _header()
    lines.append(f"{'dtype':<6}{'N':>4} {'HxWxC':<11}{'dw':>8}{'dw TB/s':>9}"
                 f"{'dw2':>8}{'isl':>8}{'pool':>8}{'ln':>8}{'ln2':>8}"
                 f"{'relu6':>8}{'tln':>8}{'lg':>8}{'lg2':>8}{'cg':>8}"
                 f"{'isl/dw':>7}{'dw/pool':>8}{'ln/relu6':>9}{'tln/ln':>7}"
                 f"{'cg/lg':>6}")
    losses = []
    for dt, dname in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        esz = 2 if dt == torch.bfloat16 else 4
        for nb in batches:
            for H, C in GEOMETRIES:
                x_b = nb * H * H * C * esz
                nbuf = max(2, -(-RING_BYTES // (2 * x_b)))
                xs = [torch.randn(nb, H, H, C, device=DEV).to(dt)
                      for _ in range(nbuf)]
                w = (torch.randn(7, 7, C, device=DEV) / 7).to(dt)
                wt = w.permute(2, 0, 1).unsqueeze(1).contiguous()
                b = torch.randn(C, device=DEV)
                g = torch.rand(C, device=DEV) + 0.5
                wl = (torch.randn(4 * C, C, device=DEV) * C ** -0.5).to(dt)
                bl = torch.randn(4 * C, device=DEV)
                turn = [0] * 12

                def nxt(i):
                    turn[i] = (turn[i] + 1) % nbuf
                    return xs[turn[i]]

                fns = [lambda: ops.dwconv7x7(nxt(0), w, b),
                       lambda: ops.dwconv7x7(nxt(1), w, b),
                       lambda: _dw_island(nxt(2), wt, b),
                       lambda: ops.maxpool2d(nxt(3), 3, 1, 1),
                       lambda: ops.layernorm_channels(nxt(4), g, b),
                       lambda: ops.layernorm_channels(nxt(5), g, b),
                       lambda: ops.relu6(nxt(6)),
                       lambda: _ln_torch(nxt(7), g, b),
                       lambda: ops.linear_gelu(nxt(8), wl, bl),
                       lambda: ops.linear_gelu(nxt(9), wl, bl),
                       lambda: _gelu_composed(nxt(10), wl, bl)]
                # the contenders of a pair compute the same function
                tol = 0.02 if dt == torch.bfloat16 else 1e-4
                for i, j in ((0, 2), (4, 7), (8, 10)):
                    turn[i] = turn[j] = 0
                    a, c = fns[i]().float(), fns[j]().float()
                    rel = ((a - c).abs().max() / c.abs().max()).item()
                    assert rel < tol, (i, j, rel)
                res = _alternate(fns)
                dw, dw2, isl, pool, ln, ln2, r6, tln, lg, lg2, cg = (
                    r[0] for r in res)
                lines.append(
                    f"{dname:<6}{nb:>4} {f'{H}x{H}x{C}':<11}{dw:>8.4f}"
                    f"{2 * x_b / (dw * 1e-3) / 1e12:>9.2f}{dw2:>8.4f}"
                    f"{isl:>8.4f}{pool:>8.4f}{ln:>8.4f}{ln2:>8.4f}{r6:>8.4f}"
                    f"{tln:>8.4f}{lg:>8.4f}{lg2:>8.4f}{cg:>8.4f}"
                    f"{isl / dw:>7.2f}{dw / pool:>8.2f}{ln / r6:>9.2f}"
                    f"{tln / ln:>7.2f}{cg / lg:>6.2f}")
                print(lines[-1], flush=True)
                for op, t, t2, other in (("dwconv7x7", dw, dw2, isl),
                                         ("layernorm_channels", ln, ln2, tln),
                                         ("linear_gelu", lg, lg2, cg)):
                    if other / t <= 1 + abs(t2 - t) / t:
                        losses.append(f"{op} {dname} N={nb} {H}x{H}x{C}")
                del xs
    lines += ["", "each new op faster than its island by more than the "
              "spread of its repeated contender: "
              + ("every row" if not losses else "NOT for " +
                 ", ".join(losses))]
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        Path(out).write_text(text)


# ------------------------------------------------------------------- model
class _Island(nn.Module):
    """A new layer run as the torch composition it replaces; .inner is the
    layer, so StageExecutor casts its parameters as usual."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        m = self.inner
        if isinstance(m, DepthwiseConv7x7):
            w = m.weight.to(x.dtype).permute(2, 0, 1).unsqueeze(1)
            return _dw_island(x, w, m.bias)
        if isinstance(m, LayerNormC):
            return _ln_torch(x, m.weight, m.bias, m.eps)
        return _gelu_composed(x, m.weight.to(x.dtype), m.bias)


def _with_islands(model):
    new = (DepthwiseConv7x7, LayerNormC, PointwiseGelu)
    nodes = [GraphNode(n.name, _Island(n.layer) if isinstance(n.layer, new)
                       else n.layer, list(n.inputs), dict(n.kwargs))
             for n in model.graph.nodes]
    return GraphModel(LayerGraph(nodes, output=model.graph.output),
                      name=model.model_name)


def bench_model(batches, out):
    lines = ["ConvNeXt-Tiny bf16, 224x224, one GPU, StageExecutor defaults "
             "(fuse=True, chain=True, no hipGraph). islands: every "
             "DepthwiseConv7x7, LayerNormC and PointwiseGelu run as the torch "
             "composition of `kernel` mode."] + _header(0.3)
    for nb in batches:
        torch.manual_seed(0)
        zoo = StageExecutor(convnext_tiny(), DEV, torch.bfloat16)
        torch.manual_seed(0)
        isl = StageExecutor(_with_islands(convnext_tiny()), DEV,
                            torch.bfloat16)
        x = torch.randn(nb, 224, 224, 3, device=DEV, dtype=torch.bfloat16)
        a, b = zoo.run(x).float(), isl.run(x).float()
        assert (a - b).abs().max().item() < 0.05, "island path differs"
        res = _alternate([lambda: zoo.run(x), lambda: isl.run(x),
                          lambda: zoo.run(x)], min_window_s=0.3)

        def ips(ms):
            return nb / (ms * 1e-3)

        for tag, (m, lo, hi) in zip(("convnext_tiny()", "with torch islands",
                                     "convnext_tiny(), again"), res):
            lines.append(f"batch {nb:>3}  {tag:<24}{ips(m):9.0f} img/s "
                         f"({ips(hi):.0f}-{ips(lo):.0f}), {m:.3f} ms")
        lines.append(f"batch {nb:>3}  islands / kernels time: "
                     f"{res[1][0] / res[0][0]:.2f}x")
        lines.append(f"batch {nb:>3}  stage graph: {_kinds(zoo)}")
        print("\n".join(lines[-5:]), flush=True)
        del isl
    lines += ["", "stage graph, stem to the end of the first block:"]
    for n in zoo.model.graph.nodes[:8]:
        lines.append(f"  {n.name:<52}{type(n.layer).__name__} <- {n.inputs}")
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
        sys.exit("convnextbench measures on the GPU; none found")
    batches = [int(b) for b in args.batches.split(",")]
    with torch.no_grad():
        if args.what == "kernel":
            bench_kernel(batches, args.out)
        else:
            bench_model(batches, args.out)


if __name__ == "__main__":
    main()
