"""GPU: the fused stem conv + max-pool kernel (csrc/stem_pool.hip) against
the conv2d_bn_act + maxpool2d launches it replaces. The outputs must match
bit for bit: the kernel feeds the same MFMA sequence, rounds with the same
epilogue expression and takes the max over the same taps."""

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


def _inputs(N, H, W, cin=3, cout=64, k=7, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(4321 + N * 1000003 + H * 1009 + W
                                      + cin * 17 + cout)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = r(N, H, W, cin).to(DEV, dtype)
    w = (r(cout, k, k, cin) * (2.0 / (cin * k * k)) ** 0.5).to(DEV, dtype)
    scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
    bias = r(cout) * 0.1
    bias[::5] = -8.0        # whole pool windows are zero after the ReLU
    return x, w, scale, bias.to(DEV)


def _two_step(x, w, scale, bias, stride, pad, act, pk, ps, pp):
    y = ops.conv2d_bn_act(x, w, scale, bias, stride=stride, padding=pad,
                          act=act)
    return ops.maxpool2d(y, pk, ps, pp)


def _cpu_ref(x, w, scale, bias, stride, pad, act, pk, ps, pp):
    y = ref.conv2d_bn_act(x.cpu(), w.cpu(), scale.cpu(), bias.cpu(), stride,
                          pad, act, None)
    return ref.maxpool2d(y, pk, ps, pp)


STEM = (2, 3, "relu", 3, 2, 1)   # stride, pad, act, pool k/s/p

# The launcher splits an image into about 512 / N bands, so a small batch
# gets one-row bands (a halo step and one step per band) and only a large
# batch makes a block walk several steps down a band, which is what the
# workload runs (28 rows per band at batch 256, 7 at batch 64). min_rpb is
# the rows per band the case must reach.
SHAPES = [
    # (N, H, W), max_blocks, min_rpb
    ((1, 224, 224), 0, 1),    # the real image size, in 56 one-row bands
    ((3, 64, 64), 0, 1),      # image boundaries inside the grid
    ((2, 30, 30), 0, 1),      # conv 15x15 (odd): last pool row/col clipped
    ((1, 18, 18), 0, 1),      # conv 9x9: smaller than any tile
    ((1, 40, 236), 0, 1),     # conv 20x118: wider than the flagship row
    ((5, 34, 34), 1, 1),      # one block walks every band of every image
    ((5, 34, 34), 2, 1),      # two blocks, carry row reset at each start
    # the steady-state walk: 6 steps per band, so the 16-slot input ring
    # wraps, the conv-row ring rotates, each step's last conv row is the
    # next one's first tap and the prefetched rows land in retired slots
    ((128, 96, 96), 0, 6),    # conv 48x48, 4 bands of 6 pooled rows
    ((128, 94, 94), 0, 6),    # conv 47x47 (odd): a one-row last step
                              # after five two-row steps
    ((128, 94, 94), 3, 6),    # three blocks walk all 512 multi-step bands
    ((64, 64, 64), 0, 2),     # 8 bands of 2: the shortest walk past s = 0
]


@pytest.mark.parametrize(
    "shape,max_blocks,min_rpb", SHAPES,
    ids=[f"{n}x{h}x{w}-mb{mb}" for (n, h, w), mb, _ in SHAPES])
def test_fused_bitwise_equals_two_step(shape, max_blocks, min_rpb):
    x, w, scale, bias = _inputs(*shape)
    want = _two_step(x, w, scale, bias, *STEM)
    before = ops.stem_pool_stats()["launches"]
    got = ops.conv_bn_act_maxpool(x, w, scale, bias, *STEM, mode=1,
                                  max_blocks=max_blocks)
    torch.cuda.synchronize()
    # the fused kernel ran (the two launches would be equal too), with the
    # band length this case is here for
    st = ops.stem_pool_stats()
    assert st["launches"] == before + 1
    assert st["rows_per_band"] >= min_rpb
    assert got.shape == want.shape
    assert (want == 0).any() and (want > 0).any()
    assert torch.equal(got, want)
    # and the pair is the right function, not merely self-consistent
    assert _relerr(got, _cpu_ref(x, w, scale, bias, *STEM)) < 0.005


FALLBACKS = {
    "cout32": dict(cout=32),
    "cin4": dict(cin=4),
    "pool220": dict(pool=(2, 2, 0)),
    "act-none": dict(act="none"),
}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("why", list(FALLBACKS))
def test_other_geometry_falls_back(why, mode):
    c = FALLBACKS[why]
    x, w, scale, bias = _inputs(2, 30, 30, cin=c.get("cin", 3),
                                cout=c.get("cout", 64))
    geo = (2, 3, c.get("act", "relu")) + c.get("pool", (3, 2, 1))
    want = _two_step(x, w, scale, bias, *geo)
    before = ops.stem_pool_stats()["launches"]
    got = ops.conv_bn_act_maxpool(x, w, scale, bias, *geo, mode=mode)
    torch.cuda.synchronize()
    assert ops.stem_pool_stats()["launches"] == before   # two launches
    assert torch.equal(got, want)
    assert _relerr(got, _cpu_ref(x, w, scale, bias, *geo)) < 0.005


def test_modes_agree_on_the_stem():
    x, w, scale, bias = _inputs(2, 64, 64)
    outs, fused = [], []
    for m in (0, 1, 2):
        before = ops.stem_pool_stats()["launches"]
        outs.append(ops.conv_bn_act_maxpool(x, w, scale, bias, *STEM,
                                            mode=m))
        fused.append(ops.stem_pool_stats()["launches"] - before)
    assert fused == [1, 1, 0]       # policy and force fuse, mode 2 does not
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2])
    assert _relerr(outs[1], _cpu_ref(x, w, scale, bias, *STEM)) < 0.005


def test_fp32_composes_the_fp32_ops():
    x, w, scale, bias = _inputs(2, 30, 30, dtype=torch.float32)
    want = _two_step(x, w, scale, bias, *STEM)
    before = ops.stem_pool_stats()["launches"]
    got = ops.conv_bn_act_maxpool(x, w, scale, bias, *STEM, mode=1)
    assert ops.stem_pool_stats()["launches"] == before
    assert got.dtype == torch.float32
    assert torch.equal(got, want)
    assert _relerr(got, _cpu_ref(x, w, scale, bias, *STEM)) < 0.005
