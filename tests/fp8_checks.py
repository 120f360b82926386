"""Shared data and bounds of the fp8 conv tests (test_conv_fp8.py on the CPU,
test_conv_fp8_gpu.py on the GPU). Not a test module.

CASES are (N, H, W, Cin, Cout, R, stride, pad), the smallest shapes that reach
each way csrc/conv_fp8.hip can go wrong (K-tile = 128 bytes, tiles 64x64 and
128x128).

Exact data: x integer in [-4, 4], w in [-2, 2] (exact in e4m3), scale from
{2^-3, 2^-4, -2^-3}, bias and residual small integers times a power of two,
so every fp32 intermediate is exact (|sum| <= 8K < 2^24) and the expected
output is one RNE rounding of an exactly known value. Channels 0 and 1 carry a
bias of +-2^18 so the e4m3 output saturates; out_scale = 2^9 puts the rest in
the e4m3 subnormals, ties included.

Random data, per-element bound (docs/TESTING.md's form), t the float64 value
before the output rounding and mag the same sum on absolute values:
  bf16: |got - t|   <= 2^-8 |t| + 1.5 (K + 7) 2^-24 mag
  e4m3: |got - t_q| <= max(2^-4 |t_q|, 2^-10) + 1.5 (K + 7) 2^-24 mag_q
in quantised units after the clamp. Nothing in it comes from the kernel."""

import torch
import torch.nn.functional as F

from defer_amd.models.resnet import _resnet

FP8 = torch.float8_e4m3fn
CASES = [
    (1, 7, 7, 16, 16, 3, 1, 1),         # K = 144: a tile + a 16-byte tail
    (2, 9, 9, 64, 80, 3, 2, 1),         # K = 576, taps straddle tiles, s2
    (1, 8, 8, 48, 32, 1, 1, 0),         # GEMM mode, K below one tile
    (2, 20, 20, 128, 128, 1, 1, 0),     # exact K, several M tiles
    (1, 6, 5, 32, 16, 3, 1, 0),         # no padding, H != W
    (1, 14, 14, 256, 256, 3, 1, 1),     # the large tile
    (1, 15, 15, 16, 32, 7, 2, 3),       # 7x7/s2 on 16 channels
]
ACTS = ("none", "relu", "relu6")
# few workgroups for many tiles, so the grid-stride loop iterates
MAX_BLOCKS = {CASES[3]: 2}
EXACT_OUT_SCALE = 2.0 ** 9
EXACT_RES_SCALE = 0.5


def out_shape(case):
    n, h, w, _, cout, r, stride, pad = case
    return (n, (h + 2 * pad - r) // stride + 1,
            (w + 2 * pad - r) // stride + 1, cout)


def make_inputs(case, exact, seed=0):
    """x_q, w_q, residual_q (e4m3) and fp32 scale, bias."""
    n, h, w, cin, cout, r, _, _ = case
    g = torch.Generator().manual_seed(seed)
    if exact:
        x = torch.randint(-4, 5, (n, h, w, cin), generator=g).float()
        wt = torch.randint(-2, 3, (cout, r, r, cin), generator=g).float()
        scale = torch.tensor([2.0 ** -3, 2.0 ** -4, -2.0 ** -3])[
            torch.randint(0, 3, (cout,), generator=g)]
        bias = torch.randint(-8, 9, (cout,), generator=g).float() * 0.25
        bias[0], bias[1] = 2.0 ** 18, -2.0 ** 18
        res = torch.randint(-6, 7, out_shape(case), generator=g).float() * 0.5
    else:
        x = torch.randn(n, h, w, cin, generator=g)
        wt = torch.randn(cout, r, r, cin, generator=g)
        scale = (torch.rand(cout, generator=g) + 0.5) / (r * cin ** 0.5)
        bias = torch.randn(cout, generator=g) * 0.2
        res = torch.randn(out_shape(case), generator=g)
    return x.to(FP8), wt.to(FP8), res.to(FP8), scale, bias


def expected(case, x_q, w_q, scale, bias, act, res_q, res_scale):
    """(t, mag) in float64: the value before the output rounding and the same
    sum on absolute values."""
    stride, pad = case[6], case[7]
    xd = x_q.double().permute(0, 3, 1, 2)
    wd = w_q.double().permute(0, 3, 1, 2)
    s, b = scale.double(), bias.double()
    t = F.conv2d(xd, wd, stride=stride, padding=pad).permute(0, 2, 3, 1) * s + b
    mag = F.conv2d(xd.abs(), wd.abs(), stride=stride,
                   padding=pad).permute(0, 2, 3, 1) * s.abs() + b.abs()
    if res_q is not None:
        t = t + res_scale * res_q.double()
        mag = mag + abs(res_scale) * res_q.double().abs()
    if act != "none":
        t = t.clamp(0.0, 6.0 if act == "relu6" else float("inf"))
    return t, mag


def check_bound(case, got, t, mag, out_scale):
    k = case[5] * case[5] * case[3]
    acc = 1.5 * (k + 7) * 2.0 ** -24
    if out_scale is None:
        assert got.dtype == torch.bfloat16
        err, lim = (got.double() - t).abs(), 2.0 ** -8 * t.abs() + acc * mag
    else:
        assert got.dtype == FP8
        t_q = (t / out_scale).clamp(-448.0, 448.0)
        err = (got.double() - t_q).abs()
        lim = torch.maximum(2.0 ** -4 * t_q.abs(),
                            torch.tensor(2.0 ** -10)) + acc * mag / out_scale
    assert bool((err <= lim).all()), float((err - lim).max())


def toy_resnet():
    """A three-block ResNet (one bottleneck in each of three stages) that
    ends in its 16 logits, seeded."""
    torch.manual_seed(0)
    return _resnet((1, 1, 1, 0), "toy", num_classes=16).graph.split(
        ["fc1000"])[0]
