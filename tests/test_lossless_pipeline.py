"""compression="lossless" through the distributed pipeline over gloo: the
compressed relay must give exactly what the unpartitioned model gives —
the tolerance the uncompressed pipeline meets."""

import os
import subprocess
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from defer_amd.config import PipelineConfig
from defer_amd.models import resnet50

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, q, cuts, steps, defer):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if defer:
        # the RCCL-order interleave s_0, s_1, p_0, ... forced on gloo; only
        # safe without the rank0 result-return cycle, so the last rank
        # collects
        os.environ["DEFER_AMD_VARRING_DEFER"] = "1"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(0)
        from defer_amd.parallel.comm import VarP2PRing
        from defer_amd.parallel.pipeline import DistPipeline

        model = resnet50()
        cfg = PipelineConfig(device="cpu", dtype="fp32",
                             partition_layers=cuts, ring_depth=2,
                             compression="lossless", backend="gloo",
                             return_results=not defer)
        pipe = DistPipeline(model, cfg, (1, 64, 64, 3))
        for ring in (pipe.recv_ring, pipe.send_ring):
            assert ring is None or isinstance(ring, VarP2PRing)
            assert ring is None or ring.defer == defer

        torch.manual_seed(1234)
        inputs = [torch.randn(1, 64, 64, 3) for _ in range(steps)]
        feed = (lambda k: inputs[k]) if rank == 0 else None
        runs = []
        for _ in range(2 if defer else 1):   # rings must reset between runs
            res = {}
            pipe.run(steps, feed=feed,
                     collect=lambda k, y: res.__setitem__(k, y.clone()))
            runs.append(res)
        if rank == (world - 1 if defer else 0):
            with torch.no_grad():
                want = [model(x) for x in inputs]
            for k in range(steps):
                for res in runs:
                    assert res[k].shape == want[k].shape
                    q.put(("err", k,
                           (res[k] - want[k]).abs().max().item()))
            # a hop that shipped raw bytes would pass the check above
            if pipe.send_ring is not None:
                raw = 4
                for d in pipe.send_ring.codec.shape:
                    raw *= d
                q.put(("wire", pipe.send_ring._host_n[0], raw))
    finally:
        dist.destroy_process_group()


def _run(world, cuts, port, steps=3, defer=False):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_worker,
                         args=(r, world, port, q, cuts, steps, defer))
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0, f"worker failed: {p.exitcode}"
    msgs = []
    while not q.empty():
        msgs.append(q.get())
    errs = [m[2] for m in msgs if m[0] == "err"]
    assert len(errs) == steps * (2 if defer else 1)
    for e in errs:
        assert e == 0.0, f"lossless relay changed the output by {e}"
    for _, n, raw in (m for m in msgs if m[0] == "wire"):
        assert 0 < n < raw, (n, raw)


def test_lossless_two_stage_bit_identical():
    _run(2, ["add_8"], 29901)


def test_lossless_three_stage_bit_identical():
    _run(3, ["add_4", "add_12"], 29902)


def test_lossless_deferred_interleave_gloo():
    """World 3, two lossless hops, no result return, the deferred
    size/payload order of the RCCL path, two runs on the same rings."""
    _run(3, ["add_4", "add_12"], 29903, defer=True)


def test_node_cli_lossless():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29904",
               WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    out = subprocess.run(
        [sys.executable, "-m", "defer_amd.node", "--device", "cpu",
         "--compression", "lossless", "--items", "2", "--batch", "2",
         "--report", "1"],
        capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "images/sec" in out.stdout
