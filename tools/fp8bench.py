"""Measurements for the fp8 (e4m3) conv path (csrc/conv_fp8.hip), on one GPU.

    python tools/fp8bench.py kernel [--batches 64,256] [--out FILE]
    python tools/fp8bench.py model  [--batches 64,256] [--out FILE]

`kernel` runs the distinct non-stem conv geometries of ResNet50 (224x224
input) and times per geometry, alternating in one process:

  fp8     ops.conv2d_bn_act_fp8, e4m3 in, e4m3 out, ReLU; TFLOP/s over
          2*M*K*Cout and TB/s over the bytes it needs: input + output +
          weights, one byte each
  fp8'    the same call again: the run-to-run spread of a repeated contender
  bf16    ops.conv2d_bn_act on bf16 tensors of the same shape (two bytes each)

A row where fp8 is slower than bf16 is marked LOSES.

`model` measures img/s of resnet50() through StageExecutor with defaults:
the bf16 graph, the graph quantised by defer_amd.quant (calibrated on a seeded
batch) and the quantised graph again, plus top-1 agreement and the cosine of
the outputs between the two on seeded inputs.

Method: tools/gconvbench.py's (device events around windows of back-to-back
calls, contenders warmed and alternated over 5 rounds, median with min-max; in
`kernel` mode rings of distinct inputs whose inputs and outputs together
exceed 1 GiB).
"""

import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from defer_amd import ops, quant  # noqa: E402
from defer_amd.graph import GraphModel  # noqa: E402
from defer_amd.models import resnet50  # noqa: E402
from defer_amd.parallel.pipeline import StageExecutor  # noqa: E402
from dwbench import DEV, RING_BYTES, _alternate, _header, _kinds  # noqa: E402

FP8 = torch.float8_e4m3fn


def resnet50_geometries():
    """Distinct (H, Cin, Cout, R, stride, pad) of the convs quantize_graph
    converts in resnet50(), in graph order, H = W of the conv's input."""
    geoms, size = [], {"input": 224}
    for n in resnet50().graph.nodes:
        lay, h = n.layer, size[n.inputs[0]]
        k = getattr(lay, "kernel", None)
        if k is None:                   # add, GAP, head: size unchanged
            size[n.name] = h
            continue
        size[n.name] = (h + 2 * lay.padding - k) // lay.stride + 1
        if hasattr(lay, "cin") and lay.cin % 16 == 0:
            g = (h, lay.cin, lay.cout, k, lay.stride, lay.padding)
            if g not in geoms:
                geoms.append(g)
    return geoms


# ------------------------------------------------------------------ kernel
def bench_kernel(batches, out):
    lines = [
        "conv + BN + ReLU on e4m3 (csrc/conv_fp8.hip) against the bf16 "
        "ops.conv2d_bn_act, the",
        "distinct non-stem conv geometries of ResNet50. TFLOP/s = 2*M*K*Cout "
        "/ time; TB/s =",
        "(input + output + weight bytes) / time, 1 TB = 1e12 B, one byte a "
        "value for fp8 and two",
        "for bf16; fp8' is the same call as a second contender (run-to-run "
        "spread). Rings of",
        "distinct inputs, inputs + outputs > 1 GiB per contender. LOSES = "
        "fp8 slower than bf16.",
        "tile*: K < 128, the e4m3 bytes widened onto the bf16 MFMA."
    ] + _header()
    lines.append(f"{'N':>4} {'HxH Cin->Cout kR/s':<24}{'tile':>6}"
                 f"{'fp8 ms':>9}{'fp8 TFLOP/s':>22}{'TB/s':>7}{'fp8b ms':>9}"
                 f"{'bf16 ms':>9}{'TFLOP/s':>9}{'TB/s':>7}{'bf16/fp8':>10}")
    worst, losses = {}, 0
    for nb in batches:
        for H, cin, cout, R, st, pad in resnet50_geometries():
            OH = (H + 2 * pad - R) // st + 1
            M, K = nb * OH * OH, R * R * cin
            flops = 2.0 * M * K * cout
            elems = nb * H * H * cin + M * cout + cout * K
            nbuf = max(2, -(-RING_BYTES // (nb * H * H * cin + M * cout)))
            xs = [torch.randn(nb, H, H, cin, device=DEV, dtype=torch.bfloat16)
                  for _ in range(nbuf)]
            xq = [ops.quantize_fp8(x, 4.0 / 448) for x in xs]
            w = (torch.randn(cout, R, R, cin, device=DEV) / K ** 0.5)
            w_scale = w.abs().amax(dim=(1, 2, 3)) / 448
            wq = (w / w_scale.view(-1, 1, 1, 1)).to(FP8)
            wb = w.to(torch.bfloat16)
            bn = torch.rand(cout, device=DEV) + 0.5
            bias = torch.randn(cout, device=DEV) * 0.1
            scale8 = bn * (4.0 / 448) * w_scale
            plan = ops.conv_fp8_plan((nb, H, H, cin), (cout, R, R, cin), st,
                                     pad)
            turn = [0] * 3

            def nxt(i, ring):
                turn[i] = (turn[i] + 1) % nbuf
                return ring[turn[i]]

            def f8(i=0):
                return ops.conv2d_bn_act_fp8(nxt(i, xq), wq, scale8, bias, st,
                                             pad, "relu", out_scale=8.0 / 448)

            def f8b():
                return f8(1)

            def b16():
                return ops.conv2d_bn_act(nxt(2, xs), wb, bn, bias, st, pad,
                                         "relu")

            # both compute the same function up to the quantisation
            a = f8().float() * (8.0 / 448)
            b = b16().float()
            rel = ((a - b).abs().max() / b.abs().max()).item()
            assert rel < 0.25, rel
            (f, flo, fhi), (f2, _, _), (h, _, _) = _alternate([f8, f8b, b16])

            def tf(ms):
                return flops / (ms * 1e-3) / 1e12

            lost = f > h
            losses += lost
            lines.append(
                f"{nb:>4} {f'{H}x{H} {cin}->{cout} k{R}/s{st}':<24}"
                f"{plan['tile'] + '*' * (plan['mfma'] == 'bf16'):>6}{f:>9.4f}"
                f"{f'{tf(f):.0f} ({tf(fhi):.0f}-{tf(flo):.0f})':>22}"
                f"{elems / (f * 1e-3) / 1e12:>7.2f}{f2:>9.4f}{h:>9.4f}"
                f"{tf(h):>9.0f}{2 * elems / (h * 1e-3) / 1e12:>7.2f}"
                f"{h / f:>10.2f}{'  LOSES' if lost else ''}")
            print(lines[-1], flush=True)
            worst[nb] = max(worst.get(nb, 0.0), abs(f2 - f) / f)
            del xs, xq
    lines.append("")
    for nb, v in worst.items():
        lines.append(f"largest |fp8' - fp8| / fp8, batch {nb}: {100 * v:.1f}%")
    lines.append(f"rows where fp8 LOSES: {losses}")
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        Path(out).write_text(text)


# ------------------------------------------------------------------- model
def bench_model(batches, out):
    lines = ["ResNet50 224x224, one GPU, StageExecutor defaults (fuse=True, "
             "chain=True, no hipGraph):",
             "the bf16 graph against the graph quantised by "
             "defer_amd.quant.quantize_graph."] + _header(0.3)
    for nb in batches:
        torch.manual_seed(0)
        model = resnet50()
        with torch.no_grad():
            gq = quant.quantize_graph(model.graph,
                                      [torch.randn(4, 224, 224, 3)])
        counts = {}
        for _, s in quant.report(gq):
            counts[s.split(":")[0]] = counts.get(s.split(":")[0], 0) + 1
        ref = StageExecutor(GraphModel(model.graph), DEV, torch.bfloat16)
        q8 = StageExecutor(GraphModel(gq), DEV, torch.bfloat16)
        x = torch.randn(nb, 224, 224, 3, device=DEV, dtype=torch.bfloat16)
        a, b = ref.run(x).float(), q8.run(x).float()
        top1 = (a.argmax(1) == b.argmax(1)).float().mean().item()
        cos = torch.nn.functional.cosine_similarity(a, b, dim=1).min().item()
        res = _alternate([lambda: ref.run(x), lambda: q8.run(x),
                          lambda: q8.run(x)], min_window_s=0.3)

        def ips(ms):
            return nb / (ms * 1e-3)

        for tag, (m, lo, hi) in zip(("bf16 resnet50()", "quantised (fp8)",
                                     "quantised (fp8), again"), res):
            lines.append(f"batch {nb:>3}  {tag:<26}{ips(m):9.0f} img/s "
                         f"({ips(hi):.0f}-{ips(lo):.0f}), {m:.3f} ms")
        lost = res[1][0] > res[0][0]
        lines.append(f"batch {nb:>3}  fp8 / bf16 speed: "
                     f"{res[0][0] / res[1][0]:.2f}x"
                     f"{'  LOSES' if lost else ''}; top-1 agreement "
                     f"{100 * top1:.1f}%, smallest output cosine {cos:.4f} "
                     "(random-init weights, seeded inputs)")
        lines.append(f"batch {nb:>3}  quant.report: {counts}")
        lines.append(f"batch {nb:>3}  quantised stage graph: {_kinds(q8)}")
        lines.append("")
        print("\n".join(lines[-7:]), flush=True)
        del ref, q8
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
        sys.exit("fp8bench measures on the GPU; none found")
    batches = [int(b) for b in args.batches.split(",")]
    with torch.no_grad():
        if args.what == "kernel":
            bench_kernel(batches, args.out)
        else:
            bench_model(batches, args.out)


if __name__ == "__main__":
    main()
