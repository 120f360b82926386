"""Measurements for the fused attention kernel (csrc/attention.hip) and
ViT-B/16, on one GPU.

    python tools/attnbench.py kernel [--out FILE]
    python tools/attnbench.py model  [--batches 64,256] [--out FILE]

`kernel` times, per (N, T, heads) and alternating in one process:

  fused   ops.attention on a bf16 qkv [N, T, 3 * heads * 64]
  fused'  the same call again: the run-to-run spread of a repeated contender
  comp    the same computation composed in bf16 torch on the same GPU: two
          matmul and a softmax on the head-transposed views of qkv

and prints the time, the achieved bytes/s against the traffic the fused
kernel needs (qkv read once, out written once: the bound that binds) and the
FLOP/s (4 * N * heads * T * T * 64).

`model` measures img/s of vit_b16() in bf16 through StageExecutor, and the
same graph with Attention.forward swapped for the composition.

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
from defer_amd.models import vit_b16  # noqa: E402
from defer_amd.models.layers import Attention  # noqa: E402
from defer_amd.parallel.pipeline import StageExecutor  # noqa: E402
from dwbench import DEV, RING_BYTES, _alternate, _header  # noqa: E402

SHAPES = [(64, 197, 12), (256, 197, 12), (64, 197, 6), (16, 577, 12)]
D = 64


def composed(qkv, heads):
    """softmax(q k^T / 8) v in bf16 torch on views of qkv."""
    shape = qkv.shape
    t = shape[-2]
    q, k, v = (qkv.reshape(-1, t, 3, heads, D).permute(2, 0, 3, 1, 4))
    p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * 0.125, dim=-1)
    return torch.matmul(p, v).transpose(1, 2).reshape(*shape[:-1], heads * D)


def bench_kernel(out):
    lines = ["Fused attention (csrc/attention.hip), bf16, D = 64.",
             "TB/s = (qkv read once + out written once) / time, 1 TB = 1e12 "
             "B; TFLOP/s = 4 * N * heads",
             "* T * T * 64 / time; fused' is the same call as a second "
             "contender (run-to-run spread);",
             "comp = two torch.matmul and a torch.softmax in bf16 on the "
             "head-transposed views of",
             "the same qkv. Rings of distinct inputs, > 1 GiB per contender; "
             "times in ms."] + _header()
    lines.append(f"{'N':>4}{'T':>5}{'heads':>6}{'fused':>9}{'TB/s':>19}"
                 f"{'TFLOP/s':>9}{'fused2':>9}{'comp':>9}{'comp/fused':>11}")
    for nb, t, h in SHAPES:
        c = h * D
        nbytes = nb * t * 4 * c * 2
        flop = 4.0 * nb * h * t * t * D
        nbuf = max(2, -(-RING_BYTES // nbytes))
        xs = [torch.randn(nb, t, 3 * c, device=DEV).bfloat16()
              for _ in range(nbuf)]
        turn = [0] * 3

        def nxt(i):
            turn[i] = (turn[i] + 1) % nbuf
            return xs[turn[i]]

        a, b = ops.attention(xs[0], h).float(), composed(xs[0], h).float()
        rel = ((a - b).abs().max() / b.abs().max()).item()
        assert rel < 0.02, rel
        res = _alternate([lambda: ops.attention(nxt(0), h),
                          lambda: ops.attention(nxt(1), h),
                          lambda: composed(nxt(2), h)])
        (f, flo, fhi), (f2, _, _), (cp, _, _) = res

        def tbs(ms):
            return nbytes / (ms * 1e-3) / 1e12

        lines.append(
            f"{nb:>4}{t:>5}{h:>6}{f:>9.4f}"
            f"{f'{tbs(f):.2f} ({tbs(fhi):.2f}-{tbs(flo):.2f})':>19}"
            f"{flop / (f * 1e-3) / 1e12:>9.1f}{f2:>9.4f}{cp:>9.4f}"
            f"{cp / f:>11.2f}")
        print(lines[-1], flush=True)
        if (nb, t, h) == SHAPES[0]:
            verdict = ("fused is not slower than the composition at "
                       f"{SHAPES[0]}: " + ("yes" if f <= cp else "NO")
                       + f" ({f:.4f} ms against {cp:.4f} ms)")
        del xs
    lines += ["", verdict]
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        Path(out).write_text(text)


def bench_model(batches, out):
    lines = ["ViT-B/16 bf16, 224x224, one GPU, StageExecutor defaults "
             "(fuse=True, no hipGraph)."] + _header(0.3)
    fused_forward = Attention.forward
    for nb in batches:
        torch.manual_seed(0)
        ex = StageExecutor(GraphModel(vit_b16().graph), DEV, torch.bfloat16)
        x = torch.randn(nb, 224, 224, 3, device=DEV, dtype=torch.bfloat16)

        def run_fused():
            Attention.forward = fused_forward
            return ex.run(x)

        def run_comp():
            Attention.forward = lambda self, qkv: composed(qkv, self.heads)
            try:
                return ex.run(x)
            finally:
                Attention.forward = fused_forward

        d = (run_fused().float() - run_comp().float()).abs().max().item()
        assert d < 0.05, "composed path differs"
        res = _alternate([run_fused, run_comp, run_fused], min_window_s=0.3)
        for tag, (m, lo, hi) in zip(("vit_b16(), ops.attention",
                                     "vit_b16(), attention composed in torch",
                                     "vit_b16(), ops.attention, again"), res):
            lines.append(f"batch {nb:>3}  {tag:<40}{nb / (m * 1e-3):9.0f} "
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
        sys.exit("attnbench measures on the GPU; none found")
    with torch.no_grad():
        if args.what == "kernel":
            bench_kernel(args.out)
        else:
            bench_model([int(b) for b in args.batches.split(",")], args.out)


if __name__ == "__main__":
    main()
