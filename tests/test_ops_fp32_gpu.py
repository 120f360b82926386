"""GPU numerics of the fp32 execution path (csrc/conv_f32.hip,
csrc/ops_f32.hip): every op on fp32 GPU tensors.

Two kinds of check, neither uses a measured tolerance:

* exact-integer data (A, D): inputs are small integers, so every product
  and partial sum is an integer below 2^24 and any summation order gives
  the same bits -> torch.equal against the CPU reference. x needs 10
  significant bits, so a silent bf16 downcast anywhere fails.
* random floats (B, C) against a float64 truth, with the standard forward
  error bound of the operation in units of u = 2^-24: a length-K fmaf
  chain plus four epilogue roundings is (K + 4)*u*A with
  A = conv(|x|,|w|)*|scale| + |bias| + |res|.

Each test prints the observed error over its bound; the recorded figures
are in profiles/numerics_envelope_fp32.txt.
"""

import pytest
import torch
import torch.nn.functional as F

import defer_amd.ops as ops
from defer_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24

# (N, H, W, Cin, Cout, R, stride, pad, act, res) and what each one hits
# with the kernel's 128x128 / 128x64 tiles and K tile of 32
CONV_CASES = [
    (2, 9, 11, 72, 40, 3, 1, 1, "none", False),    # K tail 648, Cout/M tail
    (1, 23, 23, 3, 64, 7, 2, 3, "relu", False),    # Cin%4 stem, K = 147
    (1, 12, 10, 3, 64, 3, 1, 1, "relu", False),    # odd-Cin 3x3 stem
    (2, 7, 7, 512, 136, 1, 1, 0, "none", True),    # GEMM mode, M = 98, res
    (1, 14, 14, 512, 64, 3, 2, 1, "relu", False),  # K = 4608, narrow tile
    (3, 5, 7, 1024, 72, 1, 2, 0, "none", False),   # strided 1x1 (not GEMM)
    (2, 20, 20, 64, 256, 1, 1, 0, "relu", True),   # several m- and n-tiles
    (1, 8, 8, 64, 64, 3, 1, 1, "none", False),     # pad predication
    (1, 6, 6, 8, 8, 3, 1, 0, "none", False),       # smaller than one tile
]
CONV_IDS = [f"c{i}" for i in range(len(CONV_CASES))]


def _randint(lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape).float()


def _out_hw(H, W, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


def _int_conv_inputs(case):
    N, H, W, Cin, Cout, R, stride, pad, act, has_res = case
    K = R * R * Cin
    xm = min(1000, (2 ** 24 - 4096) // (2 * K) - 1)
    x = _randint(-xm, xm, N, H, W, Cin)
    w = _randint(-2, 2, Cout, R, R, Cin)
    bias = _randint(-8, 8, Cout)
    OH, OW = _out_hw(H, W, R, stride, pad)
    res = _randint(-8, 8, N, OH, OW, Cout) if has_res else None
    return x, w, bias, res


def _gpu(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("case", CONV_CASES, ids=CONV_IDS)
def test_conv_exact_integers(case):
    N, H, W, Cin, Cout, R, stride, pad, act, has_res = case
    x, w, bias, res = _int_conv_inputs(case)
    want = ref.conv2d_bn_act(x, w, None, bias, stride, pad, act, res)
    got = ops.conv2d_bn_act(_gpu(x), _gpu(w), None, _gpu(bias),
                            stride=stride, padding=pad, act=act,
                            residual=_gpu(res))
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got.cpu(), want)
    # the data really does need more than bf16's 8 significant bits
    assert not torch.equal(x.bfloat16().float(), x)


def test_conv_all_ones_border_sums():
    """x = w = 1: each output is 64 * (number of in-bounds taps), so a
    wrong pad predicate shows as a wrong integer on the border."""
    x = torch.ones(1, 8, 8, 64)
    w = torch.ones(64, 3, 3, 64)
    want = ref.conv2d_bn_act(x, w, None, None, 1, 1, "none", None)
    got = ops.conv2d_bn_act(_gpu(x), _gpu(w), None, None, stride=1,
                            padding=1, act="none")
    assert want[0, 0, 0, 0] == 4 * 64 and want[0, 3, 3, 0] == 9 * 64
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("M,K,N,xm", [(3, 2048, 1000, 1000),
                                      (5, 25088, 64, 300)],
                         ids=["head", "vgg_fc"])
def test_linear_exact_integers(M, K, N, xm):
    x = _randint(-xm, xm, M, K)
    w = _randint(-2, 2, N, K)
    bias = _randint(-8, 8, N)
    want = ref.linear(x, w, bias)
    got = ops.linear(_gpu(x), _gpu(w), _gpu(bias))
    assert got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)


def test_conv_deterministic():
    N, H, W, Cin, Cout, R, stride, pad, act, _ = CONV_CASES[4]
    x = torch.randn(N, H, W, Cin, device=DEV)
    w = torch.randn(Cout, R, R, Cin, device=DEV) * 0.02
    sc = torch.rand(Cout, device=DEV) + 0.5
    bi = torch.randn(Cout, device=DEV)
    a = ops.conv2d_bn_act(x, w, sc, bi, stride=stride, padding=pad, act=act)
    b = ops.conv2d_bn_act(x, w, sc, bi, stride=stride, padding=pad, act=act)
    assert torch.equal(a, b)


FLOAT_CASES = [(c, i) for c, i in zip(CONV_CASES, CONV_IDS)
               if c[5] * c[5] * c[3] <= 1024]


@pytest.mark.parametrize("case", [c for c, _ in FLOAT_CASES],
                         ids=[i for _, i in FLOAT_CASES])
def test_conv_random_vs_fp64_bound(case):
    N, H, W, Cin, Cout, R, stride, pad, act, has_res = case
    K = R * R * Cin
    x = torch.randn(N, H, W, Cin)
    w = torch.randn(Cout, R, R, Cin) * (2.0 / K) ** 0.5
    scale = torch.rand(Cout) + 0.5
    bias = torch.randn(Cout) * 0.1
    OH, OW = _out_hw(H, W, R, stride, pad)
    res = torch.randn(N, OH, OW, Cout) if has_res else None

    def conv64(xx, ww):
        y = F.conv2d(xx.double().permute(0, 3, 1, 2),
                     ww.double().permute(0, 3, 1, 2), stride=stride,
                     padding=pad)
        return y.permute(0, 2, 3, 1)

    truth = conv64(x, w) * scale.double() + bias.double()
    A = conv64(x.abs(), w.abs()) * scale.double().abs() + bias.double().abs()
    if has_res:
        truth = truth + res.double()
        A = A + res.double().abs()
    if act == "relu":
        truth = torch.relu(truth)      # 1-Lipschitz: the bound carries over
    got = ops.conv2d_bn_act(_gpu(x), _gpu(w), _gpu(scale), _gpu(bias),
                            stride=stride, padding=pad, act=act,
                            residual=_gpu(res))
    err = (got.cpu().double() - truth).abs()
    bound = (K + 4) * U * A
    print(f"fp32 conv {case}: max err/A = {(err / A).max().item():.3e}, "
          f"max err/bound = {(err / bound).max().item():.4f}")
    assert (err <= bound).all()


# ---- other ops ----

SHAPE = (2, 9, 11, 72)


def test_relu_add_maxpool_concat_exact():
    x = torch.randn(*SHAPE)
    y = torch.randn(*SHAPE)
    assert torch.equal(ops.relu(_gpu(x)).cpu(), ref.relu(x))
    for act in ("relu", "none"):
        assert torch.equal(ops.add_act(_gpu(x), _gpu(y), act).cpu(),
                           ref.add_act(x, y, act))
    for k, s, p in ((3, 2, 1), (2, 2, 0)):
        assert torch.equal(ops.maxpool2d(_gpu(x), k, s, p).cpu(),
                           ref.maxpool2d(x, k, s, p))
    a = torch.randn(2, 9, 11, 32)
    b = torch.randn(2, 9, 11, 16)
    c = torch.randn(2, 9, 11, 24)
    assert torch.equal(ops.concat_channels([_gpu(a), _gpu(b)]).cpu(),
                       ref.concat_channels([a, b]))
    assert torch.equal(
        ops.concat_channels([_gpu(a), _gpu(b), _gpu(c)]).cpu(),
        ref.concat_channels([a, b, c]))


@pytest.mark.parametrize("act", ["none", "relu"])
def test_batchnorm_apply_bound(act):
    x = torch.randn(*SHAPE)
    scale = torch.rand(72) + 0.5
    bias = torch.randn(72) * 0.1
    truth = x.double() * scale.double() + bias.double()
    bound = 2 * U * ((x.double() * scale.double()).abs()
                     + bias.double().abs())
    if act == "relu":
        truth = torch.relu(truth)
    got = ops.batchnorm_apply(_gpu(x), _gpu(scale), _gpu(bias), act)
    err = (got.cpu().double() - truth).abs()
    assert got.dtype == torch.float32
    assert (err <= bound).all()


def test_avgpool_bound():
    x = torch.randn(*SHAPE)            # odd H, W: the last row/col drop
    xd = x.double().permute(0, 3, 1, 2)
    truth = F.avg_pool2d(xd, 2, 2, 0).permute(0, 2, 3, 1)
    mean_abs = F.avg_pool2d(xd.abs(), 2, 2, 0).permute(0, 2, 3, 1)
    got = ops.avgpool2d(_gpu(x), 2, 2, 0)
    err = (got.cpu().double() - truth).abs()
    assert got.shape == truth.shape
    assert (err <= 5 * U * mean_abs).all()


def test_global_avg_pool_bound():
    x = torch.randn(3, 7, 7, 72)
    truth = x.double().mean(dim=(1, 2))
    mean_abs = x.double().abs().mean(dim=(1, 2))
    got = ops.global_avg_pool(_gpu(x))
    err = (got.cpu().double() - truth).abs()
    assert got.shape == truth.shape
    assert (err <= (49 + 2) * U * mean_abs).all()


def test_softmax_bound():
    cols = 1000
    x = 4 * torch.randn(5, cols)
    truth = F.softmax(x.double(), dim=-1)
    R = (x.max(dim=-1).values - x.min(dim=-1).values).double().unsqueeze(-1)
    got = ops.softmax(_gpu(x)).cpu().double()
    rel = (got - truth).abs() / truth
    print(f"fp32 softmax: max rel err / bound = "
          f"{(rel / ((cols + R + 8) * U)).max().item():.4f}")
    assert (rel <= (cols + R + 8) * U).all()
    assert ((got.sum(dim=-1) - 1).abs() <= cols * U).all()


def test_rejections_are_readable():
    x = torch.randn(1, 4, 4, 8, device=DEV)
    w = torch.randn(8, 1, 1, 8, device=DEV)
    # C % 4 != 0
    with pytest.raises(RuntimeError, match="% 4 == 0"):
        ops.conv2d_bn_act(x, torch.randn(6, 1, 1, 8, device=DEV),
                          padding=0)
    with pytest.raises(RuntimeError, match="% 4 == 0"):
        ops.batchnorm_apply(torch.randn(2, 6, device=DEV),
                            torch.ones(6, device=DEV),
                            torch.zeros(6, device=DEV))
    with pytest.raises(RuntimeError, match="% 4 == 0"):
        ops.maxpool2d(torch.randn(1, 4, 4, 6, device=DEV), 2, 2, 0)
    with pytest.raises(RuntimeError, match="% 4 == 0"):
        ops.relu(torch.randn(6, device=DEV))
    # mixed dtypes, both ways round
    with pytest.raises(RuntimeError, match="w must be fp32"):
        ops.conv2d_bn_act(x, w.bfloat16(), padding=0)
    with pytest.raises(RuntimeError, match="w must be bf16"):
        ops.conv2d_bn_act(x.bfloat16(), w, padding=0)
    with pytest.raises(RuntimeError, match="res must be fp32"):
        ops.conv2d_bn_act(x, w, padding=0, residual=x.bfloat16())
    with pytest.raises(RuntimeError, match="b must be fp32"):
        ops.add_act(x, x.bfloat16())
    # fp16 stays unsupported
    with pytest.raises(RuntimeError, match="must be bf16 or fp32"):
        ops.conv2d_bn_act(x.half(), w.half(), padding=0)
    with pytest.raises(RuntimeError, match="must be bf16 or fp32"):
        ops.relu(x.half())
    with pytest.raises(RuntimeError, match="must be bf16 or fp32"):
        ops.softmax(torch.randn(2, 8, device=DEV).half())


def test_conv_output_beyond_4gib():
    """1x1 conv whose fp32 output is 4.3 GB (> 2^32 bytes, < 2^31
    elements): the kernel addresses through float* + 64-bit element
    index, so the last image lands where the first does. Conv is
    per-image independent: compare images 0 and 167 only."""
    NB, H, W, Cin, Cout = 168, 56, 56, 8, 2048
    assert NB * H * W * Cout * 4 > 2 ** 32 and NB * H * W * Cout < 2 ** 31
    x = _randint(-1000, 1000, NB, H, W, Cin)
    w = _randint(-2, 2, Cout, 1, 1, Cin)
    bias = _randint(-8, 8, Cout)
    got = ops.conv2d_bn_act(_gpu(x), _gpu(w), None, _gpu(bias), stride=1,
                            padding=0, act="none")
    assert got.shape == (NB, H, W, Cout)
    for n in (0, NB - 1):
        want = ref.conv2d_bn_act(x[n:n + 1], w, None, bias, 1, 0, "none",
                                 None)
        assert torch.equal(got[n:n + 1].cpu(), want)
    del got
    torch.cuda.empty_cache()
