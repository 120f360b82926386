"""Lossless pack wire: the numpy spec (defer_amd/ops/pack_ref.py) and its
Codec mode on the CPU. Patterns are compared as integers throughout — a
float comparison would let -0.0 and NaN payloads slip."""

import numpy as np
import pytest
import torch

from defer_amd.ops import pack_ref

EDGE_NUMELS = (1, 63, 64, 65, 16383, 16384, 16385)


def all_bf16_patterns():
    return np.random.default_rng(0).permutation(65536).astype(np.uint16)


def random_u32_patterns():
    rng = np.random.default_rng(1)
    return rng.integers(0, 2 ** 32, 64 * 50 + 13,
                        dtype=np.uint64).astype(np.uint32)


def edge_patterns(n, dtype):
    """ReLU-like data with NaN/Inf/denormal/-0.0 patterns mixed in, n values
    (the group and chunk edges of EDGE_NUMELS)."""
    rng = np.random.default_rng(100 + n)
    x = np.maximum(rng.standard_normal(n), 0).astype(np.float32)
    p = x.view(np.uint32).copy()
    special = np.array([0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000,
                        0x00000001, 0x00010000, 0x807F0000, 0xFFFFFFFF],
                       dtype=np.uint32)
    pos = rng.integers(0, n, min(n, 8))
    p[pos] = special[:pos.size]
    if dtype == np.uint16:
        return (p >> 16).astype(np.uint16)
    return p


def pattern_sets():
    """(name, patterns) for every case of the spec round trip; shared with
    the GPU tests."""
    sets = [("all_bf16", all_bf16_patterns()),
            ("random_u32", random_u32_patterns()),
            ("negzero_bf16", np.full(200, 0x8000, dtype=np.uint16)),
            ("negzero_f32", np.full(200, 0x80000000, dtype=np.uint32)),
            ("zeros_bf16", np.zeros(1000, dtype=np.uint16)),
            ("zeros_f32", np.zeros(1000, dtype=np.uint32))]
    for n in EDGE_NUMELS:
        sets.append((f"edge{n}_bf16", edge_patterns(n, np.uint16)))
        sets.append((f"edge{n}_f32", edge_patterns(n, np.uint32)))
    return sets


PATTERN_SETS = pattern_sets()


@pytest.mark.parametrize("name,pat", PATTERN_SETS,
                         ids=[s[0] for s in PATTERN_SETS])
def test_spec_round_trip_and_size_bound(name, pat):
    E = pat.dtype.itemsize * 8
    wire = pack_ref.encode(pat)
    assert wire.dtype == np.uint8
    assert wire.size <= pack_ref.wire_bytes_max(pat.size, E)
    assert wire.size == pack_ref.encoded_bytes(pat)
    got = pack_ref.decode(wire, pat.shape, pat.dtype)
    assert got.dtype == pat.dtype
    assert np.array_equal(got, pat)


def test_all_patterns_expand_below_bound():
    pat = all_bf16_patterns()
    wire = pack_ref.encode(pat)
    assert wire.size < 1.11 * pat.size * 2


def test_all_zero_wire_is_tables_only():
    for dt in (np.uint16, np.uint32):
        pat = np.zeros(64 * 300 + 5, dtype=dt)
        wire = pack_ref.encode(pat)
        ngroups = 301
        nchunks = 2
        assert wire.size == 16 + 4 * (nchunks + 1) + 304
        assert wire.size == pack_ref.table_bytes(pat.size)
        assert not wire[16:].any()
        assert ngroups == (pat.size + 63) // 64


def test_float32_input_is_its_bit_pattern():
    x = np.array([1.5, -0.0, 0.0, np.nan, -np.inf, 1e-42], dtype=np.float32)
    wire = pack_ref.encode(x)
    assert np.array_equal(wire, pack_ref.encode(x.view(np.uint32)))
    back = pack_ref.decode(wire, x.shape, np.float32)
    assert np.array_equal(back.view(np.uint32), x.view(np.uint32))


def test_decode_rejects_mismatched_request():
    wire = pack_ref.encode(np.arange(100, dtype=np.uint16))
    with pytest.raises(ValueError):
        pack_ref.decode(wire, (100,), np.uint32)
    with pytest.raises(ValueError):
        pack_ref.decode(wire, (99,), np.uint16)
    with pytest.raises(ValueError):
        pack_ref.decode(wire[:-4], (100,), np.uint16)


def _relu_randn():
    torch.manual_seed(0)
    return torch.relu(torch.randn(64 * 200 + 5))


def test_relu_ratio():
    x = _relu_randn()
    b16 = x.bfloat16().view(torch.int16).numpy().view(np.uint16)
    r16 = b16.size * 2 / pack_ref.encode(b16).size
    r32 = x.numel() * 4 / pack_ref.encode(x.numpy()).size
    print(f"relu(randn) ratio: bf16 {r16:.3f}x, fp32 {r32:.3f}x")
    assert r16 >= 2.0
    assert r32 >= 2.0


def test_fp32_of_bf16_values_costs_what_bf16_costs():
    x = _relu_randn().bfloat16()
    b16 = x.view(torch.int16).numpy().view(np.uint16)
    f32 = x.float().numpy()
    assert np.array_equal(pack_ref.group_lengths(f32),
                          pack_ref.group_lengths(b16))
    w16, w32 = pack_ref.encode(b16), pack_ref.encode(f32)
    t = pack_ref.table_bytes(b16.size)
    assert w32.size - t == w16.size - t
    # same tables too, so the whole wire is the same size
    assert w32.size == w16.size


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_codec_round_trip(dtype):
    from defer_amd.config import PipelineConfig
    from defer_amd.parallel.comm import Codec, VarP2PRing, make_ring

    shape = (2, 7, 7, 96)
    cfg = PipelineConfig(compression="lossless", device="cpu")
    c = Codec(cfg, shape, dtype, "cpu")
    assert c.variable
    assert c.wire_dtype == torch.uint8
    torch.manual_seed(3)
    x = torch.relu(torch.randn(*shape)).to(dtype)
    x.view(-1)[5] = float("nan")
    x.view(-1)[6] = -0.0
    wire = c.encode(x)
    assert wire.dtype == torch.uint8 and wire.numel() <= c.wire_numel
    assert wire.numel() < x.numel() * x.element_size()
    y = c.decode(wire)
    assert y.dtype == dtype and y.shape == x.shape
    idt = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(y.view(idt), x.view(idt))
    x2 = torch.relu(torch.randn(*shape)).to(dtype)
    assert torch.equal(c.decode(c.encode(x2)), x2)
    assert isinstance(make_ring(c, 2), VarP2PRing)


def test_codec_rejects_other_dtypes():
    from defer_amd.config import PipelineConfig
    from defer_amd.parallel.comm import Codec

    cfg = PipelineConfig(compression="lossless", device="cpu")
    with pytest.raises(ValueError, match="bf16 or fp32"):
        Codec(cfg, (4, 4), torch.float16, "cpu")


def test_lossless_excluded_from_dual_rail():
    from defer_amd.config import PipelineConfig
    from defer_amd.parallel.comm import dual_active

    for mode in ("lossless", "zfp+lz4"):
        cfg = PipelineConfig(compression=mode, dual_rail=True)
        assert not dual_active(cfg, 4)
    assert dual_active(PipelineConfig(compression="fp8", dual_rail=True), 4)


def test_config_rejects_misspelt_mode():
    from defer_amd.config import PipelineConfig

    PipelineConfig(compression="lossless")
    with pytest.raises(ValueError, match="unknown compression"):
        PipelineConfig(compression="loseless")
