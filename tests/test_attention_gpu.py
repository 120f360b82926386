"""GPU: ops.attention (csrc/attention.hip), embed_tokens, class_token, the
patch conv geometry of a ViT and a small ViT through StageExecutor.

u_b = 2^-8 as in docs/TESTING.md, which derives the bounds used here. One is
measured on the CPU, not on the kernel: ATT_E0, the worst error of the fp32
torch formulation (ref.attention) against float64 on this file's random
inputs, relative to A = P64 @ |v|; the kernels get 4x (another summation
order, another exp).

T sits at every edge of a 16-row query group and a 64-key tile: one live row,
one live key in the last tile, two and four key tiles, the ragged 197."""

import functools

import pytest
import torch

from defer_amd import ops
from defer_amd.graph import GraphModel
from defer_amd.models.vit import _vit
from defer_amd.ops import reference as ref
from defer_amd.parallel.pipeline import StageExecutor

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UB = 2.0 ** -8
ATT_E0 = 3.8e-6         # measured 3.747e-6 (T = 197 peaky; 6.3e-7 without it)
DTYPES = (torch.float32, torch.bfloat16)
D = 64
CASES = [(t, n, h) for t in (1, 15, 16, 17, 63, 64, 65, 130, 197)
         for n, h in ((1, 1), (2, 3))]
IDS = ["T{}-N{}-h{}".format(*c) for c in CASES]


def _pack(q, k, v):
    """q, k, v [N, T, heads, D] -> qkv [N, T, 3 * heads * D]."""
    return torch.stack((q, k, v), dim=2).reshape(q.shape[0], q.shape[1], -1)


def _heads(out, h):
    return out.float().cpu().reshape(out.shape[0], out.shape[1], h, D)


def _att64(qkv, h):
    """float64 attention of qkv as given, and A = P @ |v|, both [N, T, C]."""
    n, t = qkv.shape[:2]
    q, k, v = qkv.double().reshape(n, t, 3, h, D).permute(2, 0, 3, 1, 4)
    p = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1)
    back = lambda x: x.permute(0, 2, 1, 3).reshape(n, t, h * D)  # noqa: E731
    return back(p @ v), back(p @ v.abs())


def _bound(want, a, dt):
    fp32 = 4 * ATT_E0 * a
    return fp32 + (UB * a + UB * want.abs() if dt == torch.bfloat16 else 0)


@pytest.mark.parametrize("T,N,h", CASES, ids=IDS)
def test_attention_one_hot_gather_is_bit_exact(T, N, h):
    g = torch.Generator().manual_seed(T * 31 + N)
    k = torch.randint(0, 2, (N, T, h, D), generator=g).float() * 2 - 1
    dots = torch.einsum("nthd,nshd->nhts", k, k)
    dots -= 64 * torch.eye(T)                       # the diagonal is 64
    assert dots.max() <= 40                         # gap >= 96: exp is 0
    pi = torch.stack([torch.stack([torch.randperm(T, generator=g)
                                   for _ in range(h)]) for _ in range(N)])
    idx = pi.permute(0, 2, 1)[..., None].expand(N, T, h, D)
    q = 32 * k.gather(1, idx)                       # q[n, t, h] = 32 k[n, pi]
    v = torch.randn(N, T, h, D, generator=g).bfloat16().float()
    for dt in DTYPES:
        got = ops.attention(_pack(q, k, v).to(DEV, dt), h)
        assert got.dtype == dt and got.shape == (N, T, h * D)
        assert torch.equal(_heads(got, h), v.gather(1, idx)), dt


@pytest.mark.parametrize("T,N,h", CASES, ids=IDS)
def test_attention_uniform_rows_give_the_mean(T, N, h):
    g = torch.Generator().manual_seed(T * 37 + N)
    k = torch.randn(N, T, h, D, generator=g)
    v = torch.randint(-2, 3, (N, T, h, D), generator=g).float()
    qkv = _pack(torch.zeros_like(k), k, v)
    want = v.double().mean(1, keepdim=True).expand(N, T, h, D)
    a = v.double().abs().mean(1, keepdim=True).expand(N, T, h, D)
    for dt in DTYPES:
        got = _heads(ops.attention(qkv.to(DEV, dt), h), h)
        if T in (16, 64):
            assert torch.equal(got, want.float()), dt
        else:
            err = (got.double() - want).abs()
            assert (err <= _bound(want, a, dt)).all(), dt


@functools.lru_cache(maxsize=None)
def _random_case(T, N, h, peaky):
    g = torch.Generator().manual_seed(T * 41 + N + peaky)
    q, k, v = (torch.randn(N, T, h, D, generator=g) for _ in range(3))
    return _pack(q * (4 if peaky else 1), k, v)     # scores ~ N(0, 1), or 16


@pytest.mark.parametrize("T,N,h,peaky",
                         [c + (0,) for c in CASES] + [(197, 2, 3, 1)],
                         ids=IDS + ["T197-N2-h3-peaky"])
def test_attention_random_floats_against_float64(T, N, h, peaky):
    for dt in DTYPES:
        qkv = _random_case(T, N, h, peaky).to(dt)
        want, a = _att64(qkv, h)
        bound = _bound(want, a, dt)
        if dt == torch.float32:
            e0 = ((ref.attention(qkv, h).double() - want).abs() / a).max()
            print(f"torch fp32 T{T} N{N} h{h}: err/A {e0.item():.3e}")
            assert e0 <= ATT_E0
        runs = [ops.attention(qkv.to(DEV), h) for _ in range(3)]
        err = (runs[0].double().cpu() - want).abs()
        print(f"{dt} T{T} N{N} h{h} peaky{peaky}: worst err/bound "
              f"{(err / bound).max().item():.3f}")
        assert (err <= bound).all()
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_attention_refusals_and_empties():
    x = torch.zeros(2, 5, 3 * 2 * D, device=DEV)
    for qkv, heads, rule in ((x, 4, "D == 64"), (x.half(), 2, "bf16 or fp32"),
                             (x.transpose(0, 1), 2, "contiguous"),
                             (x[0], 2, "rank >= 3"),
                             (x, 5, "3 * heads * D")):
        with pytest.raises(RuntimeError) as e:
            ops.attention(qkv, heads)
        assert rule in str(e.value)
    assert ops.attention(x[:0], 2).shape == (0, 5, 2 * D)
    x = _random_case(17, 2, 3, 0).bfloat16().to(DEV)
    got = ops.attention(x.unsqueeze(1), 3)
    assert got.shape == (2, 1, 17, 3 * D)
    assert torch.equal(got[:, 0], ops.attention(x, 3))


@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 2, 2, 8), (3, 2, 3, 40),
                                   (2, 2, 2, 4)], ids=str)
def test_embed_tokens_and_class_token(shape):
    n, hh, ww, c = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randint(-8, 9, shape, generator=g).float()
    cls = torch.randint(-8, 9, (c,), generator=g).float()
    pos = torch.randint(-8, 9, (1 + hh * ww, c), generator=g).float()
    for dt in DTYPES if c % 8 == 0 else DTYPES[:1]:
        want = ref.embed_tokens(x.to(dt), cls, pos.to(dt))
        got = ops.embed_tokens(x.to(DEV, dt), cls.to(DEV), pos.to(DEV, dt))
        assert got.dtype == dt and got.shape == (n, 1, 1 + hh * ww, c)
        assert torch.equal(got.cpu(), want)
        tok = ops.class_token(got)
        assert tok.shape == (n, c)
        assert torch.equal(tok.cpu(), ref.class_token(want))


def _relerr(got, want):
    got, want = got.double().cpu(), want.double()
    return ((got - want).abs().max() / want.abs().max().clamp(min=1e-6)).item()


def test_vit_patch_conv_geometry():
    g = torch.Generator().manual_seed(16)
    x = torch.randn(2, 32, 32, 3, generator=g)
    w = torch.randn(64, 16, 16, 3, generator=g) * 768 ** -0.5
    b = torch.randn(64, generator=g)
    got = ops.conv2d_bn_act(x.to(DEV), w.to(DEV), None, b.to(DEV), 16, 0)
    want = ref.conv2d_bn_act(x, w, None, b, 16, 0)
    assert got.shape == want.shape == (2, 2, 2, 64)
    assert _relerr(got, want) < 1e-5
    xb, wb = x.bfloat16(), w.bfloat16()
    got = ops.conv2d_bn_act(xb.to(DEV), wb.to(DEV), None, b.to(DEV), 16, 0)
    assert _relerr(got, ref.conv2d_bn_act(xb.float(), wb.float(), None, b,
                                          16, 0)) < 0.005


DEPTH = 2


def _model():
    torch.manual_seed(0)
    return _vit(depth=DEPTH, dim=128, heads=2, patch=16, image=64)


def _run(dtype, **kw):
    ex = StageExecutor(GraphModel(_model().graph), DEV, dtype, **kw)
    x = torch.randn(2, 64, 64, 3, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        outs = [ex.run(x.to(DEV, dtype)).float().cpu() for _ in range(3)]
    return ex, x, outs


def test_vit_fp32_matches_the_cpu_model():
    _, x, (p32, _, _) = _run(torch.float32)
    with torch.no_grad():
        p_cpu = _model()(x)
    print(f"vit d2 dim128 b2 64x64: max|p_fp32 - p_cpu| = "
          f"{(p32 - p_cpu).abs().max().item():.3e}")
    assert p32.shape == (2, 1000)
    assert torch.equal(p32.argmax(-1), p_cpu.argmax(-1))


def test_vit_bf16_fusion_and_hipgraph():
    """fuse_residual_adds adds the skip to the fp32 accumulator of proj and
    mlp_2 instead of to their bf16 outputs: one bf16 rounding (u_b of the
    value) fewer at each of the two adds of a block, 2 * depth * u_b at the
    worst. A replayed hipGraph equals the eager run of the same graph."""
    _, _, (fused, _, _) = _run(torch.bfloat16, fuse=True)
    _, _, (plain, _, _) = _run(torch.bfloat16, fuse=False)
    print(f"fused vs unfused: rel {_relerr(fused, plain):.4f}")
    assert _relerr(fused, plain) <= 2 * DEPTH * UB
    assert ((fused.sum(-1) - 1).abs() < 1e-2).all()
    ex, _, replays = _run(torch.bfloat16, fuse=True, use_graph=True)
    assert ex._graph is not None, "stage did not capture"
    assert all(torch.equal(r, fused) for r in replays)
