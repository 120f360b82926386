"""GPU: the weight-stationary 3x3 window kernel (csrc/conv_ws.hip) against
the conv paths it replaces for 64 -> 64 channel 3x3/s1/p1 convs. The outputs
must match bit for bit: the kernel runs the same MFMA with the same lane
mapping, accumulates (r,s) ascending then the two channel halves ascending
without splitting the sum, and rounds with the same epilogue expression."""

import pytest
import torch

import defer_amd.ops as ops
from defer_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _relerr(got, want):
    got = got.float().cpu()
    want = want.float().cpu()
    denom = want.abs().max().clamp(min=1e-6)
    return ((got - want).abs().max() / denom).item()


def _inputs(N, H, W, cin=64, cout=64, res=False):
    g = torch.Generator().manual_seed(8642 + N * 1000003 + H * 1009 + W
                                      + cin * 17 + cout)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = r(N, H, W, cin).to(DEV, torch.bfloat16)
    w = (r(cout, 3, 3, cin) * (2.0 / (cin * 9)) ** 0.5).to(DEV,
                                                           torch.bfloat16)
    scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
    bias = (r(cout) * 0.1).to(DEV)
    return x, w, scale, bias, r


def _check(shape, max_blocks, act, res, blocks=None, tiles_per_block=None):
    N, H, W = shape
    x, w, scale, bias, r = _inputs(N, H, W)
    residual = r(N, H, W, 64).to(DEV, torch.bfloat16) if res else None
    before = ops.conv_ws_stats()["launches"]
    want = ops.conv2d_bn_act(x, w, scale, bias, 1, 1, act, residual, mode=2)
    assert ops.conv_ws_stats()["launches"] == before   # mode 2: old path
    got = ops.conv2d_bn_act(x, w, scale, bias, 1, 1, act, residual, mode=1,
                            max_blocks=max_blocks)
    torch.cuda.synchronize()
    st = ops.conv_ws_stats()
    assert st["launches"] == before + 1                # the new kernel ran
    if blocks is not None:
        assert (st["blocks"], st["tiles_per_block"]) == (blocks,
                                                         tiles_per_block)
    assert got.shape == want.shape == (N, H, W, 64)
    assert torch.equal(got, want)
    cpu = ref.conv2d_bn_act(x.cpu(), w.cpu(), scale.cpu(), bias.cpu(), 1, 1,
                            act, None if residual is None
                            else residual.cpu())
    assert _relerr(got, cpu) <= 0.005


SHAPES = [
    # (N, H, W), max_blocks, blocks, tiles per block
    ((1, 8, 16), 0, 1, 1),       # exactly one tile
    ((1, 5, 7), 0, 1, 1),        # smaller than a tile
    ((2, 9, 17), 0, 8, 1),       # one pixel past a tile in both directions,
                                 # image boundary between tiles
    ((3, 56, 56), 0, 84, 1),     # the workload's geometry, half tile in width
    ((5, 16, 32), 1, 1, 20),     # one block walks all 20 tiles (even count)
    ((5, 16, 32), 3, 3, 7),      # uneven walks of 7, 7 and 6 tiles
    ((32, 32, 64), 0, 512, 1),   # 512 tiles: mode 2 is conv_win_kernel
]


@pytest.mark.parametrize(
    "shape,max_blocks,blocks,tpb", SHAPES,
    ids=[f"{n}x{h}x{w}-mb{mb}" for (n, h, w), mb, _, _ in SHAPES])
def test_ws_bitwise_equals_old_path(shape, max_blocks, blocks, tpb):
    _check(shape, max_blocks, "relu", False, blocks, tpb)


CROSS = [((2, 9, 17), 0), ((5, 16, 32), 1), ((32, 32, 64), 0)]


@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", ["relu", "none"])
@pytest.mark.parametrize(
    "shape,max_blocks", CROSS,
    ids=[f"{n}x{h}x{w}-mb{mb}" for (n, h, w), mb in CROSS])
def test_ws_residual_and_activation(shape, max_blocks, act, res):
    _check(shape, max_blocks, act, res)


def test_ws_all_ones_is_exact():
    x = torch.ones(1, 12, 20, 64, device=DEV, dtype=torch.bfloat16)
    w = torch.ones(64, 3, 3, 64, device=DEV, dtype=torch.bfloat16)
    scale = torch.ones(64, device=DEV)
    bias = torch.zeros(64, device=DEV)
    before = ops.conv_ws_stats()["launches"]
    got = ops.conv2d_bn_act(x, w, scale, bias, 1, 1, "none", None, mode=1)
    torch.cuda.synchronize()
    assert ops.conv_ws_stats()["launches"] == before + 1
    want = torch.full((1, 12, 20, 64), 576.0)
    want[:, 0, :, :] = 384.0
    want[:, -1, :, :] = 384.0
    want[:, :, 0, :] = 384.0
    want[:, :, -1, :] = 384.0
    for i in (0, -1):
        for j in (0, -1):
            want[:, i, j, :] = 256.0
    assert torch.equal(got.float().cpu(), want)
    assert torch.equal(
        got, ops.conv2d_bn_act(x, w, scale, bias, 1, 1, "none", None,
                               mode=2))


def _fallback(x, w, scale, bias, stride):
    want = ops.conv2d_bn_act(x, w, scale, bias, stride, 1, "relu", None,
                             mode=2)
    before = ops.conv_ws_stats()["launches"]
    got = ops.conv2d_bn_act(x, w, scale, bias, stride, 1, "relu", None,
                            mode=1)
    torch.cuda.synchronize()
    assert ops.conv_ws_stats()["launches"] == before   # the old path ran
    assert torch.equal(got, want)
    cpu = ref.conv2d_bn_act(x.cpu(), w.cpu(), scale.cpu(), bias.cpu(),
                            stride, 1, "relu", None)
    assert _relerr(got, cpu) <= 0.005


def test_other_channel_count_falls_back():
    x, w, scale, bias, _ = _inputs(2, 56, 56, cin=128, cout=128)
    _fallback(x, w, scale, bias, 1)


def test_stride_two_falls_back():
    x, w, scale, bias, _ = _inputs(2, 56, 56)
    _fallback(x, w, scale, bias, 2)
