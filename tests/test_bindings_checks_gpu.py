"""GPU: what the entry points of csrc/entry_*.cpp share (csrc/entry_util.h).

The optional fp32 scale / bias vectors of the chain, chain-projection and
linear_gelu entries go through f32_vec like every other op's: a vector on
the CPU or of the wrong length is refused before anything is allocated or
launched, where a host pointer, or a vector too short, would otherwise reach
the kernel. No kernel runs in these tests: every call raises in its checks,
and the launch counters stay where they were.

The four launch counters are one type; their dicts keep their keys."""

import pytest
import torch

import defer_amd._hip_ops as hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = dict(device=DEV, dtype=torch.bfloat16)

# the smallest shapes the entries accept: one pixel, 64 -> 64 -> 64
X = (1, 1, 1, 64)
W = (64, 1, 1, 64)


def _bad_vectors():
    """(what is wrong, the vector): fp32[64] is what the entries take."""
    return [("cpu", torch.ones(64)),
            ("short", torch.ones(32, device=DEV)),
            ("long", torch.ones(128, device=DEV))]


def _launches():
    return (hip.conv1x1_chain_stats()["launches"],
            hip.chain_proj_stats()["launches"],
            hip.conv_ws_stats()["launches"])


@pytest.mark.parametrize("slot", ["s3", "b3", "s1", "b1"])
def test_conv1x1_chain_refuses_a_bad_vector(slot):
    x, res = torch.zeros(X, **BF), torch.zeros(X, **BF)
    w3, w1 = torch.zeros(W, **BF), torch.zeros(W, **BF)
    before = _launches()
    for mode in (0, 1, 2):
        for what, v in _bad_vectors():
            vec = dict(s3=None, b3=None, s1=None, b1=None)
            vec[slot] = v
            with pytest.raises(RuntimeError):
                hip.conv1x1_chain(x, w3, vec["s3"], vec["b3"], res, True, w1,
                                  vec["s1"], vec["b1"], True, mode=mode)
    torch.cuda.synchronize()
    assert _launches() == before


@pytest.mark.parametrize("slot", ["s3", "b3", "sp", "bp", "s1", "b1"])
def test_conv1x1_chain_proj_refuses_a_bad_vector(slot):
    x, xp = torch.zeros(X, **BF), torch.zeros(X, **BF)
    w3, wp, w1 = (torch.zeros(W, **BF) for _ in range(3))
    before = _launches()
    for mode in (0, 1):
        for what, v in _bad_vectors():
            vec = dict(s3=None, b3=None, sp=None, bp=None, s1=None, b1=None)
            vec[slot] = v
            with pytest.raises(RuntimeError):
                hip.conv1x1_chain_proj(x, w3, vec["s3"], vec["b3"], xp, wp,
                                       vec["sp"], vec["bp"], True, w1,
                                       vec["s1"], vec["b1"], True, mode=mode)
    torch.cuda.synchronize()
    assert _launches() == before


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
def test_linear_gelu_refuses_a_bad_bias(dtype):
    x = torch.zeros(1, 64, device=DEV, dtype=dtype)
    w = torch.zeros(64, 64, device=DEV, dtype=dtype)
    for what, v in _bad_vectors():
        with pytest.raises(RuntimeError):
            hip.linear_gelu(x, w, v)
    torch.cuda.synchronize()


def test_refusal_names_the_op_and_the_argument():
    x, res = torch.zeros(X, **BF), torch.zeros(X, **BF)
    w = torch.zeros(W, **BF)
    with pytest.raises(RuntimeError) as e:
        hip.conv1x1_chain(x, w, torch.ones(64), None, res, True, w, None,
                          None, True)
    assert "conv1x1_chain: s3 must be" in str(e.value)
    assert "on x's device" in str(e.value)


def test_stats_dicts_keep_their_keys():
    want = {
        "conv_ws_stats": ["launches", "blocks", "tiles_per_block"],
        "conv1x1_chain_stats": ["launches", "blocks", "bm"],
        "chain_proj_stats": ["launches", "blocks"],
        "stem_pool_stats": ["launches", "bands", "rows_per_band"],
    }
    for name, keys in want.items():
        d = getattr(hip, name)()
        assert list(d) == keys, name
        assert all(type(v) is int and v >= 0 for v in d.values()), name
