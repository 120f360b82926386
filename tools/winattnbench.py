"""Measurements for the shifted-window attention kernel
(csrc/window_attention.hip) and Swin-T, on one GPU.

    python tools/winattnbench.py kernel [--batches 64,256] [--out FILE]
    python tools/winattnbench.py model  [--batches 64,256] [--out FILE]

`kernel` times, per Swin-T stage geometry (map side, heads), shift and batch,
alternating in one process:

  fused   ops.window_attention on a bf16 qkv [N, H, W, 3 * heads * 32]
  fused'  the same call again: the run-to-run spread of a repeated contender
  comp    the same computation composed in bf16 torch on the same GPU: roll,
          window partition, matmul, + bias + mask, softmax, matmul, reverse
          partition, roll back. The gathered bias [heads, T, T] and the mask
          are built once outside the timed region, in the composition's
          favour.

and prints the time, the achieved bytes/s against the traffic the fused
kernel needs (qkv read once, out written once) and the FLOP/s
(4 * T * T * 32 per head and window).

`model` runs swin_t() in bf16 and fp32 through StageExecutor, prints what
the default passes made of its graph, and measures img/s in bf16 against the
same graph with WindowAttention.forward swapped for the composition.

Method: that of tools/dwbench.py, whose helpers this uses.
"""

import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from defer_amd import ops  # noqa: E402
from defer_amd.graph import GraphModel  # noqa: E402
from defer_amd.models import swin_t  # noqa: E402
from defer_amd.models.layers import TorchIsland, WindowAttention  # noqa: E402
from defer_amd.ops.reference import _window_regions  # noqa: E402
from defer_amd.parallel.pipeline import StageExecutor  # noqa: E402
from dwbench import DEV, RING_BYTES, _alternate, _header, _kinds  # noqa: E402

# (map side, heads) of the four Swin-T stages at 224; window 7
STAGES = [(56, 3), (28, 6), (14, 12), (7, 24)]
WINDOW, D = 7, 32


def bias_and_mask(table, side, heads, w, s):
    """What the composition adds to the scores: bias [heads, T, T] and, for
    s > 0, mask [windows, 1, T, T]; both in table's dtype, on its device."""
    t = w * w
    i, j = torch.arange(t) // w, torch.arange(t) % w
    idx = (i[:, None] - i[None] + w - 1) * (2 * w - 1) + j[:, None] - j[None] \
        + w - 1
    bias = table[idx.to(table.device)].permute(2, 0, 1).contiguous()
    if s == 0:
        return bias, None
    reg = _window_regions(side, w, s)
    reg = reg[:, None] * 3 + reg[None]
    reg = reg.reshape(side // w, w, side // w, w).permute(0, 2, 1, 3)
    reg = reg.reshape(-1, t)
    mask = (reg[:, :, None] != reg[:, None, :]).to(table.dtype) * -100.0
    return bias, mask[:, None].to(table.device)


def composed(qkv, bias, mask, heads, w, s):
    """ops.window_attention as torch calls on the same tensor."""
    n, hh, ww, c3 = qkv.shape
    x = torch.roll(qkv, (-s, -s), (1, 2)) if s else qkv
    x = x.reshape(n, hh // w, w, ww // w, w, 3, heads, D)
    q, k, v = x.permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(
        3, -1, heads, w * w, D)                     # [N * windows, heads, T, D]
    score = torch.matmul(q, k.transpose(-1, -2)) * D ** -0.5 + bias
    if mask is not None:
        nw = mask.shape[0]
        score = (score.reshape(n, nw, heads, w * w, w * w) + mask).reshape(
            -1, heads, w * w, w * w)
    out = torch.matmul(torch.softmax(score, dim=-1), v)
    out = out.reshape(n, hh // w, ww // w, heads, w, w, D)
    out = out.permute(0, 1, 4, 2, 5, 3, 6).reshape(n, hh, ww, c3 // 3)
    return torch.roll(out, (s, s), (1, 2)) if s else out


def bench_kernel(batches, out):
    lines = ["Shifted-window attention (csrc/window_attention.hip), bf16, "
             "D = 32, window 7:",
             "the four stage geometries of Swin-T at 224x224 (map side, "
             "heads), shift 0 and 3.",
             "TB/s = (qkv read once + out written once) / time, 1 TB = 1e12 "
             "B; TFLOP/s = 4 * 49 * 49",
             "* 32 per head and window / time; fused2 is the same call as a "
             "second contender",
             "(run-to-run spread); comp = roll, partition, matmul, + bias + "
             "mask, softmax, matmul,",
             "reverse, roll in bf16 torch on the same qkv, bias and mask "
             "prepared outside the timing.",
             "Rings of distinct inputs, > 1 GiB per contender; times in ms."
             ] + _header()
    lines.append(f"{'N':>4}{'side':>5}{'heads':>6}{'shift':>6}{'fused':>9}"
                 f"{'TB/s':>19}{'TFLOP/s':>9}{'fused2':>9}{'comp':>9}"
                 f"{'comp/fused':>11}  verdict")
    for nb in batches:
        for side, h in STAGES:
            for s in (0, WINDOW // 2) if side > WINDOW else (0,):
                c = h * D
                nbytes = nb * side * side * 4 * c * 2
                flop = 4.0 * 49 * 32 * nb * side * side * h
                nbuf = max(2, -(-RING_BYTES // nbytes))
                xs = [torch.randn(nb, side, side, 3 * c, device=DEV).bfloat16()
                      for _ in range(nbuf)]
                table = (torch.randn(169, h, device=DEV) * 0.02).bfloat16()
                bias, mask = bias_and_mask(table, side, h, WINDOW, s)
                turn = [0] * 3

                def nxt(i):
                    turn[i] = (turn[i] + 1) % nbuf
                    return xs[turn[i]]

                a = ops.window_attention(xs[0], table, h, WINDOW, s).float()
                b = composed(xs[0], bias, mask, h, WINDOW, s).float()
                rel = ((a - b).abs().max() / b.abs().max()).item()
                assert rel < 0.02, rel
                del a, b
                res = _alternate(
                    [lambda: ops.window_attention(nxt(0), table, h, WINDOW, s),
                     lambda: ops.window_attention(nxt(1), table, h, WINDOW, s),
                     lambda: composed(nxt(2), bias, mask, h, WINDOW, s)])
                (f, flo, fhi), (f2, f2lo, f2hi), (cp, cplo, _) = res

                def tbs(ms):
                    return nbytes / (ms * 1e-3) / 1e12

                # wins when the composition's best window is slower than
                # the worst window of either fused contender
                wins = cplo > max(fhi, f2hi)
                lines.append(
                    f"{nb:>4}{side:>5}{h:>6}{s:>6}{f:>9.4f}"
                    f"{f'{tbs(f):.2f} ({tbs(fhi):.2f}-{tbs(flo):.2f})':>19}"
                    f"{flop / (f * 1e-3) / 1e12:>9.1f}{f2:>9.4f}{cp:>9.4f}"
                    f"{cp / f:>11.2f}  {'wins' if wins else 'LOSES'}")
                print(lines[-1], flush=True)
                del xs
    text = "\n".join(lines) + "\n"
    if out:
        Path(out).write_text(text)


def bench_model(batches, out):
    lines = ["Swin-T, 224x224, one GPU, StageExecutor defaults (fuse=True, "
             "no hipGraph)."] + _header(0.3)
    fused_forward = WindowAttention.forward
    prepared = {}

    def composed_forward(self, qkv):
        key = (id(self), qkv.dtype)
        if key not in prepared:
            prepared[key] = bias_and_mask(
                self.relative_position_bias_table.to(qkv.dtype), qkv.shape[1],
                self.heads, self.window, self.shift)
        return composed(qkv, *prepared[key], self.heads, self.window,
                        self.shift)

    def fresh():
        prepared.clear()
        torch.manual_seed(0)
        return GraphModel(swin_t().graph)

    for dt in (torch.bfloat16, torch.float32):
        ex = StageExecutor(fresh(), DEV, dt)
        y = ex.run(torch.randn(8, 224, 224, 3, device=DEV, dtype=dt)).float()
        assert not any(isinstance(n.layer, TorchIsland)
                       for n in ex.model.graph.nodes)
        assert ((y.sum(-1) - 1).abs() < 1e-2).all()
        lines.append(f"swin_t() {dt}: runs, rows sum to 1, no TorchIsland; "
                     f"stage graph: {_kinds(ex)}")
    lines += ["the first nodes after the default passes:"] + [
        f"  {n.name}: {type(n.layer).__name__} <- {', '.join(n.inputs)}"
        for n in ex.model.graph.nodes[2:12]] + [""]
    del ex
    for nb in batches:
        ex = StageExecutor(fresh(), DEV, torch.bfloat16)
        x = torch.randn(nb, 224, 224, 3, device=DEV, dtype=torch.bfloat16)

        def run_fused():
            WindowAttention.forward = fused_forward
            return ex.run(x)

        def run_comp():
            WindowAttention.forward = composed_forward
            try:
                return ex.run(x)
            finally:
                WindowAttention.forward = fused_forward

        d = (run_fused().float() - run_comp().float()).abs().max().item()
        assert d < 0.05, "composed path differs"
        res = _alternate([run_fused, run_comp, run_fused], min_window_s=0.3)
        for tag, (m, lo, hi) in zip(
                ("swin_t(), ops.window_attention",
                 "swin_t(), window attention composed in torch",
                 "swin_t(), ops.window_attention, again"), res):
            lines.append(f"batch {nb:>3}  {tag:<46}{nb / (m * 1e-3):9.0f} "
                         f"img/s ({nb / (hi * 1e-3):.0f}-"
                         f"{nb / (lo * 1e-3):.0f}), {m:.3f} ms")
        lines.append("")
        print("\n".join(lines[-4:]), flush=True)
        del ex
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
        sys.exit("winattnbench measures on the GPU; none found")
    batches = [int(b) for b in args.batches.split(",")]
    with torch.no_grad():
        if args.what == "kernel":
            bench_kernel(batches, args.out)
        else:
            bench_model(batches, args.out)


if __name__ == "__main__":
    main()
