"""GPU: the 128-row-tile form of the chained expand->reduce kernel
(csrc/chain.hip, K1 = 256, N2 = 256) against the two conv2d_bn_act launches
and against the 64-row form. All three must agree bit for bit on y and a2;
ops.conv1x1_chain_stats() shows which tile height really ran."""

import pytest
import torch

import defer_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K1, N2 = 256, 256


def _inputs(N, H, W, N1, affine=True):
    g = torch.Generator().manual_seed(1313 + N1 + N * H * W)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = r(N, H, W, K1).to(DEV, torch.bfloat16)
    res = r(N, H, W, N1).to(DEV, torch.bfloat16)
    w3 = (r(N1, 1, 1, K1) * (2.0 / K1) ** 0.5).to(DEV, torch.bfloat16)
    w1 = (r(N2, 1, 1, N1) * (2.0 / N1) ** 0.5).to(DEV, torch.bfloat16)
    if affine:
        s3 = (torch.rand(N1, generator=g) + 0.5).to(DEV)
        b3 = (r(N1) * 0.1).to(DEV)
    else:
        s3 = b3 = None
    s1 = (torch.rand(N2, generator=g) + 0.5).to(DEV)
    b1 = (r(N2) * 0.1).to(DEV)
    return x, w3, s3, b3, res, w1, s1, b1


def _run(t, act3, **kw):
    x, w3, s3, b3, res, w1, s1, b1 = t
    out = ops.conv1x1_chain(x, w3, s3, b3, res, act3, w1, s1, b1, "relu",
                            **kw)
    torch.cuda.synchronize()
    return out


CASES = [
    # (N, H, W), N1, act3, affine3, max_blocks
    ((1, 7, 7), 64, "relu", True, 0),      # M=49 < one tile: clamped rows
    ((1, 7, 7), 128, "relu", True, 0),
    ((1, 8, 16), 64, "relu", True, 0),     # M=128: one exact tile, one chunk
    ((1, 8, 16), 128, "none", True, 0),
    ((2, 14, 14), 64, "relu", True, 1),    # M=392: 4 tiles, the last 8 rows,
    ((2, 14, 14), 128, "relu", True, 1),   # all in one block: tile hand-over
    ((2, 14, 14), 128, "relu", True, 2),   # 2 + 2 tiles
    ((2, 14, 14), 128, "relu", True, 0),   # default grid, one tile a block
    ((2, 14, 14), 64, "relu", False, 2),   # s3 = b3 = None
    ((2, 14, 14), 128, "none", False, 1),
    ((2, 14, 14), 1024, "relu", True, 1),  # the real class, 16 chunks
]


@pytest.mark.parametrize("case", CASES,
                         ids=[f"t{i}" for i in range(len(CASES))])
def test_bm128_bitwise_equals_two_launches_and_bm64(case):
    (N, H, W), N1, act3, affine, max_blocks = case
    t = _inputs(N, H, W, N1, affine)
    M = N * H * W
    want_y, want_a2 = _run(t, act3, mode=2)
    y64, a64 = _run(t, act3, mode=1, max_blocks=max_blocks, bm=64)
    assert ops.conv1x1_chain_stats()["bm"] == 64
    n0 = ops.conv1x1_chain_stats()["launches"]
    y, a2 = _run(t, act3, mode=1, max_blocks=max_blocks, bm=128)
    st = ops.conv1x1_chain_stats()
    assert st["launches"] == n0 + 1 and st["bm"] == 128
    tiles = (M + 127) // 128
    assert st["blocks"] == (min(max_blocks, tiles) if max_blocks else tiles)
    assert y.shape == want_y.shape and a2.shape == want_a2.shape
    assert torch.equal(y, want_y) and torch.equal(a2, want_a2)
    assert torch.equal(y, y64) and torch.equal(a2, a64)


def test_policy_keeps_64_rows_within_one_round():
    # 7 tiles of 64 rows: far below the gate (more than 256 such tiles)
    t = _inputs(2, 14, 14, 1024)
    y0, a0 = _run(t, "relu", mode=0)
    assert ops.conv1x1_chain_stats()["bm"] == 64
    y2, a2 = _run(t, "relu", mode=2)
    assert torch.equal(y0, y2) and torch.equal(a0, a2)


def test_policy_takes_128_rows_past_one_round():
    # M = 16512: 258 tiles of 64 rows, just past the gate; 129 of 128
    t = _inputs(1, 129, 128, 1024)
    y0, a0 = _run(t, "relu", mode=0)
    st = ops.conv1x1_chain_stats()
    assert st["bm"] == 128 and st["blocks"] == 129
    y2, a2 = _run(t, "relu", mode=2)
    y64, a64 = _run(t, "relu", mode=0, bm=64)
    assert ops.conv1x1_chain_stats()["bm"] == 64
    assert torch.equal(y0, y2) and torch.equal(a0, a2)
    assert torch.equal(y0, y64) and torch.equal(a0, a64)


def test_other_classes_keep_64_rows_when_128_is_asked_for():
    # K1 = 256, N2 = 512 has no 128-row form: bm = 128 runs its 64-row one
    g = torch.Generator().manual_seed(99)
    x = torch.randn(1, 9, 9, 256, generator=g).to(DEV, torch.bfloat16)
    res = torch.randn(1, 9, 9, 128, generator=g).to(DEV, torch.bfloat16)
    w3 = (torch.randn(128, 1, 1, 256, generator=g) * 0.1).to(
        DEV, torch.bfloat16)
    w1 = (torch.randn(512, 1, 1, 128, generator=g) * 0.1).to(
        DEV, torch.bfloat16)
    args = (x, w3, None, None, res, "relu", w1, None, None, "relu")
    y, a2 = ops.conv1x1_chain(*args, mode=1, bm=128)
    assert ops.conv1x1_chain_stats()["bm"] == 64
    y2, a22 = ops.conv1x1_chain(*args, mode=2)
    assert torch.equal(y, y2) and torch.equal(a2, a22)


def test_bm_is_checked():
    t = _inputs(1, 7, 7, 64)
    with pytest.raises(ValueError):
        _run(t, "relu", mode=1, bm=96)
