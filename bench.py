#!/usr/bin/env python3
"""Flagship benchmark: ResNet50 pipeline-partitioned inference throughput
(images/sec, whole node) — the reference's headline metric
(/root/reference/test/test.py:25-37: results counted over a window) on
MI355X at 1/2/4/8 stages.

Single GPU:   python bench.py --gpus 1 --steps 200 --warmup 20
Multi GPU:    python bench.py --gpus N ...          (self-spawns N ranks)
         or:  python -m torch.distributed.run --nnodes=1 --nproc-per-node N
                --master-addr 127.0.0.1 bench.py --gpus N ...

Rank r runs pipeline stage r; boundary activations relay over RCCL/xGMI
(optionally ZFP-compressed). Synthetic 224x224x3 data, random-init
weights (no network access for datasets), bf16 compute.

A "step" processes one global batch (--batch images). At world > 1 the
global batch is split into --micro-batch-sized pipeline items so the
chain stays full (the reference streams single images through its node
chain, test/test.py:20-23,47-49; micro-batches are the throughput-viable
version of that operating point).

A plain run sets up, warms up, times --steps steps and prints the result
line. With --full, a short serialized pass after the timed region also
measures true per-item end-to-end latency (feed at rank0 -> result back
at rank0, host-synchronized), reported as latency_ms (null otherwise).
--dump-outputs DIR writes the last timed step's outputs as DIR/output.npy.
"""

import argparse
import json
import os
import time

import torch


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=800,
                    help="timed steps; one step = one --batch global batch "
                         "(default sized so the timed region is >=5 s at "
                         "1 GPU: the driver's rocm-smi sampling can see "
                         "the GPU busy, and ms_per_step is robust to "
                         "clock ramp)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--model", default="resnet50",
                    choices=["resnet50", "resnet101", "resnet152",
                             "vgg19", "vgg19_gap", "densenet121"])
    ap.add_argument("--batch", type=int, default=256,
                    help="images per step (global batch; throughput "
                         "saturates ~128-256, profiles/README.md)")
    ap.add_argument("--micro-batch", type=int, default=0,
                    help="images per pipeline item; 0 = auto (=batch at "
                         "1 stage; 64 at >1 stage so 20 driver steps are "
                         ">=80 items and pipeline fill/drain stays <10%%)")
    ap.add_argument("--compression", default="none",
                    choices=["none", "fp8", "zfp", "zfp+lz4", "auto"])
    ap.add_argument("--zfp-bits", type=int, default=8)
    ap.add_argument("--cuts", default="auto",
                    help='"auto", "defer8", or comma-separated layer names')
    ap.add_argument("--graphs", action="store_true",
                    help="capture stage forwards in hipGraphs")
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"])
    ap.add_argument("--ring-depth", type=int, default=4)
    ap.add_argument("--dual-rail", dest="dual_rail", default=None,
                    action="store_true",
                    help="split each fixed-size hop across two xGMI "
                         "rails (direct + via an idle third GPU); "
                         "doubles effective hop bandwidth for "
                         "boundaries above one link's 153 GB/s. "
                         "Default: ON at world >= 4 (every hop dual, "
                         "the xGMI-topology-aware design point), OFF "
                         "below")
    ap.add_argument("--no-dual-rail", dest="dual_rail",
                    action="store_false")
    ap.add_argument("--no-return-results", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline "
                         "figure (the serialized latency pass)")
    ap.add_argument("--latency-items", type=int, default=32,
                    help="serialized items for the --full post-run "
                         "latency measurement (0 = skip)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the outputs of the last timed step as "
                         "DIR/output.npy (float32)")
    ap.add_argument("--calibration", default=None, metavar="JSON",
                    help="per-layer measured-cost file for auto cuts "
                         "(tools/calibrate.py); default: use the "
                         "in-tree profile for this model if present")
    ap.add_argument("--stats", action="store_true",
                    help="print per-stage stats to stderr (hipEvent "
                         "compute time, wire bytes)")
    ap.add_argument("--dump-partition", default=None, metavar="DIR",
                    help="write per-stage DOT/text partition dumps "
                         "(plot_model parity, reference node.py:39)")
    return ap.parse_args(argv)


def worker(args):
    # ONE-JSON-LINE stdout contract: native libs write banners straight
    # to fd 1 (gloo's rank banner; RCCL's version line under NCCL_DEBUG),
    # so park the real stdout and point fd 1 at stderr for the whole
    # run — the JSON line goes to the saved fd at the end.
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    from defer_amd.config import PipelineConfig
    from defer_amd.models import DEFER_8STAGE_CUTS, MODELS
    from defer_amd.parallel.pipeline import DistPipeline

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(
            f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus}; launch "
            f"with matching -nproc-per-node or let bench.py self-spawn")
    dist_mode = world > 1
    import torch.distributed as dist
    if dist_mode:
        backend = "nccl" if args.device == "cuda" else "gloo"
        if args.device == "cuda":
            ndev = torch.cuda.device_count()
            torch.cuda.set_device(local_rank % ndev)
        dist.init_process_group(backend)
    else:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29771")
        dist.init_process_group(
            "nccl" if args.device == "cuda" else "gloo", rank=0,
            world_size=1)

    torch.manual_seed(0)
    model = MODELS[args.model]()

    if args.cuts == "auto":
        cuts = None
    elif args.cuts == "defer8":
        cuts = DEFER_8STAGE_CUTS
    else:
        cuts = [c for c in args.cuts.split(",") if c]

    B = args.batch
    M = args.micro_batch
    if M <= 0:
        M = B if world == 1 else min(64, B)
    if B % M:
        raise SystemExit(f"--batch {B} not divisible by --micro-batch {M}")
    per_step = B // M
    if args.dual_rail is None:
        # default: dual-rail when EVERY hop can run dual (world >= 4);
        # the auto-partitioner's bandwidth credit follows via
        # comm.dual_bw_boost
        args.dual_rail = world >= 4 and args.compression != "zfp+lz4"

    cfg = PipelineConfig(
        partition_layers=cuts, num_stages=world, device=args.device,
        dtype="bf16" if args.device == "cuda" else "fp32",
        batch_size=M, use_hip_graphs=args.graphs,
        compression=args.compression, zfp_rate_bits=args.zfp_bits,
        ring_depth=args.ring_depth, dual_rail=args.dual_rail,
        backend="nccl" if args.device == "cuda" else "gloo",
        return_results=not args.no_return_results,
        log_stage_stats=args.stats,
        calibration_file=args.calibration,
        partition_dump_dir=args.dump_partition)

    dev = (torch.device("cuda",
                        local_rank % max(torch.cuda.device_count(), 1))
           if args.device == "cuda" else torch.device("cpu"))
    pipe = DistPipeline(model, cfg, (M, 224, 224, 3), device=dev)

    dtype = torch.bfloat16 if args.device == "cuda" else torch.float32
    # static synthetic input batches, pre-generated on device (the
    # reference feeds one preprocessed image repeatedly, test/test.py:20-23)
    n_inputs = 4
    inputs = [torch.randn(M, 224, 224, 3, device=dev, dtype=dtype)
              for _ in range(n_inputs)] if pipe.rank == 0 else None

    def feed(k):
        return inputs[k % n_inputs]

    sink = {}

    def collect(k, y):
        sink["last"] = (k, y.shape)

    # --dump-outputs: keep the items of the last timed step (the slot a
    # ring hands to collect is reused, so clone; one step's logits only)
    kept = {}
    first_kept = (args.steps - 1) * per_step

    def collect_kept(k, y):
        sink["last"] = (k, y.shape)
        if k >= first_kept:
            kept[k] = y.clone()

    def barrier_sync():
        dist.barrier()
        if args.device == "cuda":
            torch.cuda.synchronize()

    # establish the world communicator collectively BEFORE any p2p op
    # (lazy per-pair init ordering is then irrelevant on RCCL)
    barrier_sync()

    # ---- dual-rail stall watchdog around warmup+barrier. The dual-rail
    # relay is gloo-proven but its first-ever RCCL execution is the
    # round-end multi-GPU run itself; if an RCCL-specific stall shows up
    # there it would show up in the warmup, so every rank re-execs
    # itself single-rail (same argv + --no-dual-rail; fd 1 restored for
    # the one-JSON-line contract; env rendezvous state survives exec)
    # instead of hanging the whole scaling sweep.
    import sys as _sys
    import threading

    warm_done = threading.Event()
    wd_s = float(os.environ.get("DEFER_BENCH_WATCHDOG_S", "300"))
    arm = args.dual_rail and world > 2 and \
        (args.device == "cuda"
         or os.environ.get("DEFER_BENCH_TEST_STALL") == "1")

    def _watchdog():
        if not warm_done.wait(timeout=wd_s):
            print(f"[bench rank {rank}] dual-rail warmup stalled "
                  f">{wd_s:.0f}s; re-exec single-rail", flush=True)
            os.environ.pop("DEFER_BENCH_TEST_STALL", None)
            # fresh rendezvous on a derived port: under torchrun the
            # original store lives in the (still running) agent and a
            # second init on it would collide on rendezvous keys; the
            # re-exec'd rank 0 hosts the new store itself
            os.environ["MASTER_ADDR"] = "127.0.0.1"
            os.environ["MASTER_PORT"] = str(
                int(os.environ.get("MASTER_PORT", "29500")) + 17)
            # TORCHELASTIC_USE_AGENT_STORE=True would make every rank a
            # store CLIENT on the new port (nobody hosts) — drop the
            # torchrun-agent markers so rank 0 hosts the fresh store
            for k in list(os.environ):
                if k.startswith("TORCHELASTIC"):
                    os.environ.pop(k)
            os.dup2(real_stdout, 1)
            argv = [a for a in _sys.argv[1:]
                    if a not in ("--dual-rail", "--no-dual-rail")]
            os.execv(_sys.executable,
                     [_sys.executable, os.path.abspath(__file__)]
                     + argv + ["--no-dual-rail"])

    if arm:
        threading.Thread(target=_watchdog, daemon=True).start()
    if os.environ.get("DEFER_BENCH_TEST_STALL") == "1" and arm:
        time.sleep(wd_s * 3 + 10)   # simulate a hung warmup (tests)

    # ---- warmup (fills pipeline, triggers graph capture)
    pipe.run(max(args.warmup, 2) * per_step, feed=feed, collect=collect)
    barrier_sync()
    warm_done.set()
    pipe.reset_stats()

    # ---- timed region: exactly --steps global batches
    t0 = time.perf_counter()
    pipe.run(args.steps * per_step, feed=feed,
             collect=collect_kept if args.dump_outputs else collect)
    barrier_sync()
    t1 = time.perf_counter()

    elapsed = torch.tensor([t1 - t0], dtype=torch.float64,
                           device=dev if args.device == "cuda" else "cpu")
    if dist_mode:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)  # NCCL needs GPU
    elapsed = elapsed.cpu()
    el = elapsed.item()
    images = args.steps * B
    ips = images / el
    import copy

    timed_stats = copy.copy(pipe.stats)   # before the latency pass runs

    # ---- --dump-outputs: what the last timed step handed to collect, on
    # the rank that received it (rank 0, or the last rank under
    # --no-return-results), in item order
    if kept:
        import numpy as np

        y = torch.cat([kept[k] for k in sorted(kept)]).float().cpu().numpy()
        cap = (64 << 20) // 4
        if y.size > cap:   # fixed seeded sample of an oversized output
            idx = np.sort(np.random.default_rng(0).choice(
                y.size, cap, replace=False))
            y = y.reshape(-1)[idx]
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "output.npy"), y)

    # ---- --full, untimed: serialized per-item end-to-end latency (rank0
    # feed -> rank0 result, host-synced per item; the reference's batch-1
    # streaming protocol operating point, test/test.py:47-49)
    lat = None
    L = args.latency_items if args.full else 0
    if L > 0 and (world == 1 or not args.no_return_results):
        lat_ms = []
        t_feed = {}

        def lfeed(k):
            if args.device == "cuda":
                torch.cuda.synchronize()
            t_feed[k] = time.perf_counter()
            return inputs[k % n_inputs]

        def lcollect(k, y):
            if args.device == "cuda":
                torch.cuda.synchronize()
            lat_ms.append((time.perf_counter() - t_feed.pop(k)) * 1e3)

        pipe.run(L, feed=lfeed if pipe.rank == 0 else feed,
                 collect=lcollect if pipe.rank == 0 else collect)
        barrier_sync()
        if pipe.rank == 0 and lat_ms:
            srt = sorted(lat_ms)

            def pct(p):
                return round(srt[min(len(srt) - 1, int(p * len(srt)))], 3)

            lat = {"p50": pct(0.5), "p90": pct(0.9), "p99": pct(0.99),
                   "items": L, "micro_batch": M}

    if args.stats:
        import sys
        st = timed_stats
        cms = st.compute_ms / max(st.items, 1)
        busy = st.compute_ms / 1e3 / el * 100 if el > 0 else 0.0
        print(f"[stage {pipe.rank}] items={st.items} images={st.images} "
              f"compute={cms:.3f}ms/item (dev busy ~{busy:.0f}%) "
              f"wire_in={st.bytes_in/1e6:.1f}MB wire_out="
              f"{st.bytes_out/1e6:.1f}MB fwd={st.bytes_fwd/1e6:.1f}MB "
              f"({st.bytes_out/max(st.items,1)/1e6:.2f} MB/item)",
              file=sys.stderr)
    if pipe.rank == 0:
        out = {
            "metric": "images/sec (whole node) "
                      + {"resnet50": "ResNet50", "resnet101": "ResNet101",
                         "resnet152": "ResNet152", "vgg19": "VGG19",
                         "vgg19_gap": "VGG19-GAP",
                         "densenet121": "DenseNet121"}[args.model]
                      + " pipeline",
            "value": round(ips, 1),
            "unit": "images/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(el / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": cfg.dtype,
            "data": "synthetic",
            "latency_ms": lat,
            "config": {
                "model": args.model,
                "global_batch": B,
                "micro_batch": M,
                "input": "224x224x3 NHWC",
                "parallelism": f"pp{world}",
                "cuts": pipe.cuts,
                "compression": args.compression
                + (f"@{args.zfp_bits}b" if args.compression != "none"
                   else ""),
                "hip_graphs": bool(args.graphs),
                "dual_rail": bool(args.dual_rail),
                "weights": "random-init",
            },
        }
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    os.close(real_stdout)
    dist.destroy_process_group()


def _spawned(rank, args, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["LOCAL_RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(args.gpus)
    worker(args)


def main():
    args = parse_args()
    if "WORLD_SIZE" in os.environ or args.gpus <= 1:
        # launched under torchrun (driver's N>1 form) or single rank
        worker(args)
        return
    # bare `bench.py --gpus N`: self-spawn N ranks (one per GPU) so the
    # scaling curve needs no external launcher
    import torch.multiprocessing as mp

    port = 29500 + (os.getpid() % 1000)
    mp.spawn(_spawned, args=(args, port), nprocs=args.gpus, join=True)


if __name__ == "__main__":
    main()
