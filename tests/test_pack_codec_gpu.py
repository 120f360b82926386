"""Lossless pack wire on the GPU: the kernels in csrc/pack.hip against the
numpy spec (defer_amd/ops/pack_ref.py), byte for byte."""

import numpy as np
import pytest
import torch

from defer_amd.ops import pack_ref

from test_pack_codec import PATTERN_SETS


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _to_gpu(pat):
    """numpy bit patterns -> cuda tensor of bf16 (uint16) or fp32 (uint32)"""
    if pat.dtype == np.uint16:
        return torch.from_numpy(pat.view(np.int16).copy()).cuda() \
            .view(torch.bfloat16)
    return torch.from_numpy(pat.view(np.int32).copy()).cuda() \
        .view(torch.float32)


def _patterns_of(t):
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("name,pat", PATTERN_SETS,
                         ids=[s[0] for s in PATTERN_SETS])
def test_gpu_matches_spec(name, pat):
    _need_gpu()
    from defer_amd.ops import codec as zc

    x = _to_gpu(pat)
    spec = pack_ref.encode(pat)
    wire = zc.pack_encode(x)
    assert wire.dtype == torch.uint8 and wire.is_cuda
    assert wire.numel() == spec.size, (wire.numel(), spec.size)
    got = wire.cpu().numpy()
    assert np.array_equal(got, spec), \
        f"first differing byte {int(np.argmax(got != spec))}"
    # GPU decodes the spec's wire
    y = zc.pack_decode(torch.from_numpy(spec).cuda(), pat.shape, x.dtype)
    assert y.dtype == x.dtype and tuple(y.shape) == pat.shape
    assert np.array_equal(_patterns_of(y), pat)
    # CPU decodes the GPU's wire
    assert np.array_equal(pack_ref.decode(got, pat.shape, pat.dtype), pat)


@pytest.mark.gpu
def test_gpu_multi_chunk_round_trip():
    """300 chunks plus a partial one: more chunk totals than one round of
    the offsets kernel's 256-thread scan."""
    _need_gpu()
    from defer_amd.ops import codec as zc

    n = 300 * 16384 + 777
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.relu(torch.randn(n, device="cuda", generator=g)) \
        .to(torch.bfloat16)
    wire = zc.pack_encode(x)
    want = pack_ref.encoded_bytes(_patterns_of(x))
    assert wire.numel() == want, (wire.numel(), want)
    assert wire.numel() < n           # ~50 % zeros: better than 2x
    y = zc.pack_decode(wire, (n,), torch.bfloat16)
    assert torch.equal(y.view(torch.int16), x.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gpu_encode_into_respects_buffer(dtype):
    """pack_encode_into on a worst-case buffer: device int64 = spec size,
    bytes past it untouched."""
    _need_gpu()
    from defer_amd import ops as _ops
    from defer_amd.ops import codec as zc

    m = _ops._load_hip()
    n = 3 * 16384 + 65
    g = torch.Generator(device="cuda").manual_seed(6)
    x = torch.relu(torch.randn(n, device="cuda", generator=g)).to(dtype)
    bits = 16 if dtype == torch.bfloat16 else 32
    cap = zc.pack_wire_bytes_max((n,), dtype)
    assert cap == pack_ref.wire_bytes_max(n, bits)
    assert cap == int(m.pack_wire_bytes_max(n, bits))
    out = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(int(m.pack_scratch_bytes(n, bits)),
                          dtype=torch.uint8, device="cuda")
    size = torch.full((1,), -1, dtype=torch.long, device="cuda")
    m.pack_encode_into(x, scratch, out, size)
    spec = pack_ref.encode(_patterns_of(x))
    assert int(size.item()) == spec.size
    got = out.cpu().numpy()
    assert np.array_equal(got[:spec.size], spec)
    assert (got[spec.size:] == 0xA5).all()
    with pytest.raises(RuntimeError):
        m.pack_encode_into(x, scratch, out[:cap - 1], size)


@pytest.mark.gpu
def test_var_ring_cuda_sender_bookkeeping_lossless(monkeypatch):
    """VarP2PRing's CUDA sender with the lossless codec, without a peer:
    stub dist.isend and verify the issued sequence s_0,s_1,p_0,s_2,p_1,...
    with device-computed lengths equal to the spec's and payloads that
    decode to the exact input."""
    _need_gpu()
    import torch.distributed as dist

    from defer_amd.config import PipelineConfig
    from defer_amd.parallel.comm import Codec, VarP2PRing

    sent = []

    class _W:
        def wait(self):
            pass

    def fake_isend(t, dst=None, **kw):
        torch.cuda.synchronize()          # value must be final by now
        sent.append(t.detach().clone())
        return _W()

    monkeypatch.setattr(dist, "isend", fake_isend)

    shape = (2, 14, 14, 256)
    cfg = PipelineConfig(compression="lossless", ring_depth=2)
    c = Codec(cfg, shape, torch.bfloat16, "cuda")
    ring = VarP2PRing(c, cfg.ring_depth)
    assert ring.defer and ring.cuda
    torch.manual_seed(9)
    xs = [torch.relu(torch.randn(*shape) * (k + 1)).to("cuda",
                                                       torch.bfloat16)
          for k in range(4)]
    for k, x in enumerate(xs):
        ring.send_encoded(k, x, dst=1)
    ring.flush()
    kinds = ["s", "s", "p", "s", "p", "s", "p", "p"]
    items = [0, 1, 0, 2, 1, 3, 2, 3]
    assert len(sent) == len(kinds)
    sizes = {}
    for t, kind, it in zip(sent, kinds, items):
        if kind == "s":
            assert t.dtype == torch.long and t.numel() == 1
            sizes[it] = int(t.item())
            assert sizes[it] == pack_ref.encoded_bytes(_patterns_of(xs[it]))
        else:
            assert t.numel() == sizes[it], (it, t.numel(), sizes[it])
            got = c.decode(t)
            assert torch.equal(got.view(torch.int16),
                               xs[it].view(torch.int16)), \
                f"item {it} corrupted"
