"""GPU: dwconv7x7 (csrc/dwconv7.hip), layernorm_channels
(csrc/layernorm.hip), linear_gelu (the ACT_GELU epilogues), the two conv
geometries ConvNeXt adds to the existing kernels, and convnext_tiny().

u = 2^-24 and u_b = 2^-8 as in docs/TESTING.md, which derives every bound
used here. Two are measured on the CPU, not on the kernel: LN_E0, the worst
normalised error of the fp32 torch formulation of LayerNorm on this file's
inputs, and GELU_E0, the worst error of fp32 F.gelu over [-10, 10]; the
kernels get 4x each (another summation order, another erff).

dwconv7x7's tile policy balances the tile rows (TH = ceil(H / ceil(H / 8))),
so no H leaves a tile with a single live row; 9x17 is two tiles of 5 and 4
rows and, at TW = 16, a second tile column with one live column."""

import functools

import pytest
import torch
import torch.nn.functional as F

from defer_amd import ops
from defer_amd.graph import GraphModel
from defer_amd.models import convnext_tiny
from defer_amd.ops import reference as ref
from defer_amd.parallel.pipeline import StageExecutor

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U, UB = 2.0 ** -24, 2.0 ** -8
LN_E0 = 1.36e-5         # measured 1.352e-5 (fp32 torch, rows of 100 + randn)
GELU_E0 = 1.21e-6       # measured 1.207e-6 (fp32 F.gelu, at v = 3.49)
DTYPES = (torch.float32, torch.bfloat16)

DW_SHAPES = [(1, 1, 1, 8), (1, 2, 3, 8), (2, 7, 7, 24), (3, 5, 33, 40),
             (1, 14, 14, 104), (1, 9, 17, 8)]


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def _relerr(got, want):
    got, want = got.double().cpu(), want.double()
    return ((got - want).abs().max() / want.abs().max().clamp(min=1e-6)).item()


def _dw64(x, w, b):
    c = x.shape[-1]
    y = F.conv2d(x.double().permute(0, 3, 1, 2),
                 w.double().permute(2, 0, 1).unsqueeze(1),
                 None if b is None else b.double(), padding=3, groups=c)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", DW_SHAPES, ids=_ids(DW_SHAPES))
def test_dwconv7x7_exact_integers(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randint(-2, 3, shape, generator=g).float()
    w = torch.randint(-1, 2, (7, 7, shape[-1]), generator=g).float()
    b = torch.randint(0, 3, (shape[-1],), generator=g).float()
    for bias in (b, None):
        want = ref.dwconv7x7(x, w, bias)
        assert want.abs().max() <= 100
        for dt in DTYPES:
            for cap in (0, 2):                  # 2: fewer blocks than tiles
                got = ops.dwconv7x7(
                    x.to(DEV, dt), w.to(DEV, dt),
                    None if bias is None else bias.to(DEV), max_blocks=cap)
                assert got.dtype == dt and got.shape == want.shape
                assert torch.equal(got.float().cpu(), want), (dt, cap)


@pytest.mark.parametrize("shape", DW_SHAPES[2:5], ids=_ids(DW_SHAPES[2:5]))
def test_dwconv7x7_random_floats(shape):
    g = torch.Generator().manual_seed(sum(shape) * 7)
    x = torch.randn(*shape, generator=g)
    w = torch.randn(7, 7, shape[-1], generator=g) / 7
    b = torch.randn(shape[-1], generator=g) * 0.5
    got = ops.dwconv7x7(x.to(DEV), w.to(DEV), b.to(DEV))
    err = (got.double().cpu() - _dw64(x, w, b)).abs()
    bound = (49 + 4) * U * _dw64(x.abs(), w.abs(), b.abs())
    print(f"fp32 {shape}: worst err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    xb, wb = x.bfloat16(), w.bfloat16()
    runs = [ops.dwconv7x7(xb.to(DEV), wb.to(DEV), b.to(DEV))
            for _ in range(3)]
    e = _relerr(runs[0], _dw64(xb.float(), wb.float(), b))
    print(f"bf16 {shape}: rel err {e:.5f}")
    assert e < 0.005
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_dwconv7x7_refuses_on_the_gpu():
    x = torch.zeros(1, 4, 4, 8, device=DEV)
    w, b = torch.zeros(7, 7, 8, device=DEV), torch.zeros(8, device=DEV)
    for args, rule in (((x, w, b.cpu()), "device"), ((x, w.cpu(), b), "device"),
                       ((x, w, b[:4]), "fp32[C]"),
                       ((x, w.bfloat16(), b), "mixed dtypes"),
                       ((x.transpose(1, 2), w, b), "contiguous")):
        with pytest.raises(RuntimeError) as e:
            ops.dwconv7x7(*args)
        assert rule in str(e.value)
    assert ops.dwconv7x7(x[:0], w, b).shape == (0, 4, 4, 8)


def _ln_case(rows, C, dt):
    """x = 100 + randn, float64 reference, the normaliser |weight| * (|xhat|
    + 1) + |bias| of the bound, all from the inputs as the kernel sees them."""
    g = torch.Generator().manual_seed(rows * 4099 + C)
    x = (100 + torch.randn(rows, C, generator=g)).to(dt)
    w = torch.rand(C, generator=g) + 0.5
    b = torch.randn(C, generator=g) * 0.5
    xhat = F.layer_norm(x.double(), (C,), None, None, 1e-6)
    want = xhat * w.double() + b.double()
    return x, w, b, want, w.double() * (xhat.abs() + 1) + b.abs().double()


def _ln_bound(want, norm, dt):
    return 4 * LN_E0 * norm + (UB * want.abs() if dt == torch.bfloat16 else 0)


@pytest.mark.parametrize("C", [4, 8, 96, 104, 768, 2048])
def test_layernorm_channels(C):
    for dt in DTYPES if C % 8 == 0 else DTYPES[:1]:
        for rows, shape, cap in ((1, (1, C), 0), (3, (1, 3, 1, C), 0),
                                 (65, (5, 13, 1, C), 0), (65, (65, C), 1)):
            x, w, b, want, norm = _ln_case(rows, C, dt)
            bound = _ln_bound(want, norm, dt)
            torch_err = (ref.layernorm_channels(x.float(), w, b).double()
                         - want).abs()
            assert (torch_err <= bound).all()
            got = ops.layernorm_channels(x.reshape(shape).to(DEV), w.to(DEV),
                                         b.to(DEV), max_blocks=cap)
            assert got.dtype == dt and got.shape == shape
            err = (got.double().cpu().reshape(rows, C) - want).abs()
            print(f"{dt} rows {rows} C {C}: worst err/bound "
                  f"{(err / bound).max().item():.3f}")
            assert (err <= bound).all()
        const = torch.full((3, C), 3.0, dtype=dt, device=DEV)
        got = ops.layernorm_channels(const, w.to(DEV), b.to(DEV))
        assert torch.equal(got.cpu(), b.to(dt).expand(3, C))


LG_SHAPES = [(1, 8, 8), (65, 96, 384), (200, 768, 72), (63, 384, 96)]


@pytest.mark.parametrize("M,K,N", LG_SHAPES, ids=_ids(LG_SHAPES))
def test_linear_gelu(M, K, N):
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g)
    shape = (M, 1, 1, K) if M % 2 else (2, M // 2, K)    # 4-D and 3-D x
    for bias in (b, None):
        b64 = 0 if bias is None else bias.double()
        bd = None if bias is None else bias.to(DEV)
        got = ops.linear_gelu(x.reshape(shape).to(DEV), w.to(DEV), bd)
        assert got.shape == shape[:-1] + (N,)
        err = (got.double().cpu().reshape(M, N)
               - F.gelu(x.double() @ w.double().t() + b64)).abs()
        mag = x.abs().double() @ w.abs().double().t() + abs(b64)
        bound = 1.13 * (K + 4) * U * mag + 4 * GELU_E0
        print(f"fp32 {M}x{K}x{N}: worst err/bound "
              f"{(err / bound).max().item():.3f}")
        assert (err <= bound).all()
        xb, wb = x.bfloat16(), w.bfloat16()
        got = ops.linear_gelu(xb.reshape(shape).to(DEV), wb.to(DEV), bd)
        want = F.gelu(xb.double() @ wb.double().t() + b64)
        e = _relerr(got.reshape(M, N), want)
        print(f"bf16 {M}x{K}x{N}: rel err {e:.5f}")
        assert got.dtype == torch.bfloat16 and e < 0.005


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
def test_linear_gelu_exact_values(dt):
    """Integer x and w: the pre-activation is exact. gelu(0) is 0; from 6 up
    1 + erff is 2 to well inside a bf16 ulp, so the bf16 output is the
    pre-activation."""
    x = torch.zeros(4, 8)
    x[1, 0], x[2, :2], x[3, :] = 6, 4, 2        # rows give 0, 6, 8, 16
    w = torch.ones(8, 8)
    got = ops.linear_gelu(x.to(DEV, dt), w.to(DEV, dt)).float().cpu()
    rows = 4 if dt == torch.bfloat16 else 1
    assert torch.equal(got[:rows], x.sum(-1, keepdim=True).expand(4, 8)[:rows])


@pytest.mark.parametrize("x_shape,cout,k", [((2, 32, 32, 3), 96, 4),
                                            ((2, 8, 8, 96), 192, 2)],
                         ids=["stem 4x4s4", "downsample 2x2s2"])
def test_convnext_conv_geometries(x_shape, cout, k):
    g = torch.Generator().manual_seed(k)
    cin = x_shape[-1]
    x = torch.randn(*x_shape, generator=g)
    w = torch.randn(cout, k, k, cin, generator=g) * (k * k * cin) ** -0.5
    b = torch.randn(cout, generator=g)
    got = ops.conv2d_bn_act(x.to(DEV), w.to(DEV), None, b.to(DEV), k, 0)
    want = ref.conv2d_bn_act(x, w, None, b, k, 0)
    assert got.shape == want.shape and _relerr(got, want) < 1e-5
    xb, wb = x.bfloat16(), w.bfloat16()
    got = ops.conv2d_bn_act(xb.to(DEV), wb.to(DEV), None, b.to(DEV), k, 0)
    assert _relerr(got, ref.conv2d_bn_act(xb.float(), wb.float(), None, b,
                                          k, 0)) < 0.005


def _model():
    torch.manual_seed(0)
    return convnext_tiny()


@functools.lru_cache(maxsize=None)
def _input():
    return torch.randn(2, 64, 64, 3, generator=torch.Generator().manual_seed(1))


def _run(dtype, **kw):
    ex = StageExecutor(GraphModel(_model().graph), DEV, dtype, **kw)
    x = _input().to(DEV, dtype)
    with torch.no_grad():
        outs = [ex.run(x).float().cpu() for _ in range(3)]
    return ex, outs


def test_convnext_tiny_fp32_matches_the_cpu_model():
    with torch.no_grad():
        p_cpu = _model()(_input())
    _, (p32, _, _) = _run(torch.float32)
    print(f"convnext_tiny b2 64x64: max|p_fp32 - p_cpu| = "
          f"{(p32 - p_cpu).abs().max().item():.3e}")
    assert p32.shape == (2, 1000)
    assert torch.equal(p32.argmax(-1), p_cpu.argmax(-1))


def test_convnext_tiny_bf16_fusion_and_hipgraph():
    """fuse_residual_adds adds the skip to the fp32 accumulator of
    pointwise_conv_2 instead of to its bf16 output: one bf16 rounding (u_b
    of the value) fewer in each of the 18 blocks, 18 * u_b at the worst. A
    replayed hipGraph equals the eager run of the same stage graph."""
    _, (fused, _, _) = _run(torch.bfloat16, fuse=True)
    _, (plain, _, _) = _run(torch.bfloat16, fuse=False)
    print(f"fused vs unfused: rel {_relerr(fused, plain):.4f}")
    assert _relerr(fused, plain) <= 18 * UB
    assert ((fused.sum(-1) - 1).abs() < 1e-2).all()
    ex, replays = _run(torch.bfloat16, fuse=True, use_graph=True)
    assert ex._graph is not None, "stage did not capture"
    assert all(torch.equal(r, fused) for r in replays)
