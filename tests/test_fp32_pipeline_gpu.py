"""Whole-model fp32 execution on the GPU: PipelineConfig(dtype="fp32")
through StageExecutor, the graph passes, threaded DEFER and hipGraph
capture.

Accuracy criterion (no measured tolerance): with p the output
probabilities, max|p_gpu_fp32 - p_cpu| <= max|p_gpu_bf16 - p_cpu| / 64.
fp32's unit roundoff is 2^15 finer than bf16's; asking for 2^6 leaves 2^9
for the different summation orders of the two fp32 implementations. The
measured maxima are recorded in profiles/numerics_envelope_fp32.txt.
"""

import functools
import queue
import threading

import pytest
import torch

from defer_amd import DEFER, PipelineConfig
from defer_amd.graph import GraphModel
from defer_amd.models import MODELS
from defer_amd.parallel.pipeline import StageExecutor

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _model(name):
    """A fresh, identically seeded instance: StageExecutor moves and casts
    the parameters of the model it is given."""
    torch.manual_seed(0)
    return MODELS[name]()


@functools.lru_cache(maxsize=None)
def _input(batch):
    g = torch.Generator().manual_seed(1234)
    return torch.randn(batch, 64, 64, 3, generator=g)


@functools.lru_cache(maxsize=None)
def _cpu_probs(name, batch):
    with torch.no_grad():
        return _model(name)(_input(batch)).float()


@functools.lru_cache(maxsize=None)
def _gpu_probs(name, batch, dtype, **kw):
    ex = StageExecutor(GraphModel(_model(name).graph), DEV, dtype,
                       use_graph=False, **kw)
    with torch.no_grad():
        y = ex.run(_input(batch).to(DEV, dtype))
    assert y.dtype == dtype
    return y.float().cpu()


@pytest.mark.parametrize("name,batch", [("resnet50", 2), ("densenet121", 1),
                                        ("vgg19_gap", 1)])
def test_fp32_is_64x_closer_to_cpu_than_bf16(name, batch):
    p_cpu = _cpu_probs(name, batch)
    p32 = _gpu_probs(name, batch, torch.float32)
    p16 = _gpu_probs(name, batch, torch.bfloat16)
    e32 = (p32 - p_cpu).abs().max().item()
    e16 = (p16 - p_cpu).abs().max().item()
    print(f"{name} b{batch} 64x64: max|p_fp32-p_cpu| = {e32:.3e}, "
          f"max|p_bf16-p_cpu| = {e16:.3e}, ratio = {e16 / max(e32, 1e-300):.0f}")
    assert p32.shape == p_cpu.shape
    assert e32 <= e16 / 64
    assert torch.equal(p32.argmax(-1), p_cpu.argmax(-1))


def test_fp32_graph_passes_do_not_change_bits():
    """fuse_residual_adds / fuse_expand_reduce in fp32 run the same
    arithmetic as the unfused graph (the chain op is a composition)."""
    on = _gpu_probs("resnet50", 2, torch.float32, fuse=True, chain=True)
    off = _gpu_probs("resnet50", 2, torch.float32, fuse=False)
    assert torch.equal(on, off)


def test_fp32_defer_four_stages_matches_single_stage():
    want = _gpu_probs("resnet50", 2, torch.float32)
    g = torch.Generator().manual_seed(99)
    xs = [_input(2), torch.randn(2, 64, 64, 3, generator=g)]
    ex = StageExecutor(GraphModel(_model("resnet50").graph), DEV,
                       torch.float32, use_graph=False)
    with torch.no_grad():
        wants = [ex.run(x.to(DEV)).cpu() for x in xs]
    assert torch.equal(wants[0], want)

    eng = DEFER([DEV] * 4, config=PipelineConfig(device="cuda",
                                                 dtype="fp32"))
    in_q, out_q = queue.Queue(8), queue.Queue(8)
    err = []

    def serve():
        try:
            eng.run_defer(_model("resnet50"), ["add_4", "add_8", "add_12"],
                          in_q, out_q)
        except Exception as e:       # fail the test at once, not by timeout
            err.append(e)
            out_q.put(None)

    t = threading.Thread(target=serve)
    t.start()
    for x in xs:
        in_q.put(x.to(DEV))
    in_q.put(None)
    outs = []
    for _ in xs:
        o = out_q.get(timeout=120)
        assert o is not None, f"pipeline failed: {err!r}"
        outs.append(o)
    t.join(timeout=60)
    assert not t.is_alive() and not err
    for o, w in zip(outs, wants):
        assert o.dtype == torch.float32
        assert torch.equal(o.cpu(), w)


def test_fp32_hipgraph_replay_matches_eager():
    want = _gpu_probs("resnet50", 2, torch.float32)
    ex = StageExecutor(GraphModel(_model("resnet50").graph), DEV,
                       torch.float32, use_graph=True)
    x = _input(2).to(DEV)
    with torch.no_grad():
        first = ex.run(x).cpu()       # captures, then replays once
        second = ex.run(x).cpu()      # replay
    torch.cuda.synchronize()
    assert ex._graph is not None, "fp32 stage did not capture"
    assert torch.equal(first, want)
    assert torch.equal(second, want)
