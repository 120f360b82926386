"""GPU: ops.window_attention (csrc/window_attention.hip), ops.patch_merge and
a small Swin through StageExecutor.

u_b = 2^-8 as in docs/TESTING.md, which derives the bounds used here. One is
measured on the CPU, not on the kernel: WATT_E0, the worst error of the fp32
torch formulation (ref.window_attention) against float64 on this file's
random inputs, relative to A = P64 @ |v|; the kernels get 4x (another
summation order, another exp).

The geometries (H, W, window, shift, N, heads) reach T = 4, 9, 16, 49 and 64
(one query group mostly padding, one exact group, the ragged 3 * 16 + 1, no
padded key at all), H != W, whole and partial workgroups, and a shift inside
a single window."""

import functools

import pytest
import torch

from defer_amd import ops
from defer_amd.graph import GraphModel
from defer_amd.models.swin import _swin
from defer_amd.ops import reference as ref
from defer_amd.parallel.pipeline import StageExecutor

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UB = 2.0 ** -8
WATT_E0 = 2.7e-6        # measured 2.583e-6 ((14,21,7,3,2,3) peaky; 5.3e-7 without)
DTYPES = (torch.float32, torch.bfloat16)
D = 32
CASES = [(4, 4, 2, 0, 1, 1), (4, 4, 2, 1, 2, 3), (6, 6, 3, 1, 1, 3),
         (8, 12, 4, 2, 2, 1), (7, 7, 7, 0, 1, 3), (14, 21, 7, 3, 2, 3),
         (16, 16, 8, 4, 1, 5), (7, 7, 7, 3, 1, 1)]
IDS = ["H{}W{}-w{}s{}-N{}h{}".format(*c) for c in CASES]


def _windows(x, w, s):
    """[N, H, W, ...] -> [N, H/w, W/w, T, ...]: roll by -s, then partition."""
    n, hh, ww = x.shape[:3]
    x = torch.roll(x, (-s, -s), (1, 2))
    x = x.reshape(n, hh // w, w, ww // w, w, *x.shape[3:]).transpose(2, 3)
    return x.reshape(n, hh // w, ww // w, w * w, *x.shape[5:])


def _unwindows(x, hh, ww, w, s):
    """The inverse of _windows for [N, H/w, W/w, T, C]."""
    n, c = x.shape[0], x.shape[-1]
    x = x.reshape(n, hh // w, ww // w, w, w, c).transpose(2, 3)
    return torch.roll(x.reshape(n, hh, ww, c), (s, s), (1, 2))


def _apart(hh, ww, w, s):
    """[H/w, W/w, T, T] bool: token pairs whose row or column regions differ
    (region of a shifted row r': 0 below H - w, 1 below H - s, else 2)."""
    def reg(size):
        r = torch.arange(size)
        return (r >= size - w).long() + (r >= size - s).long() if s else 0 * r
    lab = (reg(hh)[:, None] * 3 + reg(ww)[None])[None, :, :, None]
    lab = _windows(lab, w, 0)[0, ..., 0]            # labels of the shifted frame
    return lab[..., :, None] != lab[..., None, :]


def _winatt64(qkv, table, h, w, s):
    """float64 window attention of qkv and table as given, and A = P @ |v|,
    both [N, H, W, C]: roll, partition, gather, mask, softmax, reverse."""
    n, hh, ww, _ = qkv.shape
    x = _windows(qkv.double().reshape(n, hh, ww, 3, h, D), w, s)
    q, k, v = x.permute(4, 0, 1, 2, 5, 3, 6)        # each [N, nh, nw, h, T, D]
    i, j = torch.arange(w * w) // w, torch.arange(w * w) % w
    idx = (i[:, None] - i[None] + w - 1) * (2 * w - 1) + j[:, None] - j[None] \
        + w - 1
    score = q @ k.transpose(-1, -2) * D ** -0.5 + \
        table.double()[idx].permute(2, 0, 1)
    score = score - 100.0 * _apart(hh, ww, w, s)[:, :, None]
    p = torch.softmax(score, dim=-1)
    back = lambda o: _unwindows(                              # noqa: E731
        o.transpose(3, 4).reshape(n, hh // w, ww // w, w * w, h * D),
        hh, ww, w, s)
    return back(p @ v), back(p @ v.abs())


def _bound(want, a, dt):
    fp32 = 4 * WATT_E0 * a
    return fp32 + (UB * a + UB * want.abs() if dt == torch.bfloat16 else 0)


@pytest.mark.parametrize("H,W,w,s,N,h", CASES, ids=IDS)
def test_window_means(H, W, w, s, N, h):
    """q = 0 and a zero table: every output is the mean of v over the query's
    allowed set, its window's tokens of the same row and column region."""
    g = torch.Generator().manual_seed(H * 37 + s)
    k = torch.randn(N, H, W, h * D, generator=g)
    v = torch.randint(-2, 3, (N, H, W, h * D), generator=g).float()
    qkv = torch.cat((torch.zeros_like(k), k, v), dim=-1)
    table = torch.zeros((2 * w - 1) ** 2, h)
    allowed = (~_apart(H, W, w, s)).double()[None]           # [1, nh, nw, T, T]
    cnt = allowed.sum(-1, keepdim=True)
    vw = _windows(v.double(), w, s)
    want = _unwindows(allowed @ vw / cnt, H, W, w, s)
    a = _unwindows(allowed @ vw.abs() / cnt, H, W, w, s)
    for dt in DTYPES:
        got = ops.window_attention(qkv.to(DEV, dt), table.to(DEV, dt), h, w, s)
        assert got.dtype == dt and got.shape == (N, H, W, h * D)
        got = got.float().cpu()
        if w in (2, 4, 8):                  # every allowed set is a power of two
            assert torch.equal(got, want.float()), dt
        else:
            err = (got.double() - want).abs()
            assert (err <= _bound(want, a, dt)).all(), dt


@functools.lru_cache(maxsize=None)
def _random_case(H, W, w, s, N, h, peaky):
    g = torch.Generator().manual_seed(H * 41 + W + s + N + peaky)
    q, k, v = (torch.randn(N, H, W, h * D, generator=g) for _ in range(3))
    table = torch.randn((2 * w - 1) ** 2, h, generator=g)
    return torch.cat((q * (4 if peaky else 1), k, v), dim=-1), table


@pytest.mark.parametrize("H,W,w,s,N,h,peaky",
                         [c + (0,) for c in CASES] + [CASES[5] + (1,)],
                         ids=IDS + [IDS[5] + "-peaky"])
def test_window_attention_random_floats_against_float64(H, W, w, s, N, h,
                                                        peaky):
    for dt in DTYPES:
        qkv, table = (x.to(dt) for x in _random_case(H, W, w, s, N, h, peaky))
        want, a = _winatt64(qkv, table, h, w, s)
        bound = _bound(want, a, dt)
        if dt == torch.float32:
            e0 = ((ref.window_attention(qkv, table, h, w, s).double() - want)
                  .abs() / a).max()
            print(f"torch fp32 {H}x{W} w{w} s{s}: err/A {e0.item():.3e}")
            assert e0 <= WATT_E0
        runs = [ops.window_attention(qkv.to(DEV), table.to(DEV), h, w, s)
                for _ in range(3)]
        err = (runs[0].double().cpu() - want).abs()
        print(f"{dt} {H}x{W} w{w} s{s} N{N} h{h} peaky{peaky}: worst "
              f"err/bound {(err / bound).max().item():.3f}")
        assert (err <= bound).all()
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


@pytest.mark.parametrize("w", [2, 3, 4, 7, 8])
def test_unshifted_unbiased_windows_are_plain_attention(w):
    """shift 0 and a zero table: each window is softmax(q k^T / sqrt(32)) v
    over its tokens taken as a sequence, the definition ops.attention has."""
    n, h, side = 2, 2, 2 * w
    g = torch.Generator().manual_seed(w)
    x = torch.randn(n, side, side, 3 * h * D, generator=g)
    for dt in DTYPES:
        qkv, table = x.to(dt), torch.zeros((2 * w - 1) ** 2, h, dtype=dt)
        got = ops.window_attention(qkv.to(DEV), table.to(DEV), h, w, 0).cpu()
        for wr, wc in ((0, 0), (0, 1), (1, 0), (1, 1)):
            rows, cols = slice(wr * w, wr * w + w), slice(wc * w, wc * w + w)
            q, k, v = (qkv[:, rows, cols].double()
                       .reshape(n, w * w, 3, h, D).permute(2, 0, 3, 1, 4))
            p = torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, dim=-1)
            want, a = ((p @ m).transpose(1, 2).reshape(n, w, w, h * D)
                       for m in (v, v.abs()))
            err = (got[:, rows, cols].double() - want).abs()
            assert (err <= _bound(want, a, dt)).all(), (dt, wr, wc)


def test_window_attention_refusals_and_empties():
    x = torch.zeros(2, 6, 6, 3 * 2 * D, device=DEV)
    t = torch.zeros(25, 2, device=DEV)
    for qkv, tab, heads, w, s, rule in (
            (x.half(), t.half(), 2, 3, 0, "bf16 or fp32"),
            (x.transpose(1, 2), t, 2, 3, 0, "contiguous"),
            (x[0], t, 2, 3, 0, "4-D"),
            (x, t, 4, 3, 0, "3 * heads * 32"),
            (x, t, 2, 1, 0, "window^2 <= 64"),
            (x, t, 2, 9, 0, "window^2 <= 64"),
            (x, t, 2, 4, 0, "divide H and W"),
            (x[:, :, :3].contiguous(), t, 2, 2, 0, "divide H and W"),
            (x, t, 2, 3, 3, "0 <= shift < window"),
            (x, t, 2, 3, -1, "0 <= shift < window"),
            (x, t[:9], 2, 3, 0, "bias_table must be"),
            (x, t.bfloat16(), 2, 3, 0, "bias_table must be"),
            (x, torch.zeros(2, 25, device=DEV).t(), 2, 3, 0,
             "bias_table must be"),
            (torch.empty(1, 4730, 4730, 96, device=DEV, dtype=torch.bfloat16),
             t[:9, :1].bfloat16(), 1, 2, 0, "2^31 or more elements")):
        with pytest.raises(RuntimeError) as e:
            ops.window_attention(qkv, tab, heads, w, s)
        assert rule in str(e.value), rule
    assert ops.window_attention(x[:0], t, 2, 3, 1).shape == (0, 6, 6, 2 * D)


@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (2, 4, 6, 8), (3, 2, 2, 40),
                                   (2, 2, 2, 4)], ids=str)
def test_patch_merge(shape):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)))
    for dt in DTYPES if shape[3] % 8 == 0 else DTYPES[:1]:
        xd = x.to(dt)
        got = ops.patch_merge(xd.to(DEV))
        assert got.dtype == dt and got.is_contiguous()
        assert torch.equal(got.cpu(), ref.patch_merge(xd))
        assert torch.equal(got.cpu(), torch.cat(
            [xd[:, r::2, c::2] for c in (0, 1) for r in (0, 1)], dim=-1))
    with pytest.raises(RuntimeError, match="must be even"):
        ops.patch_merge(torch.zeros(1, 3, 2, 8, device=DEV))


def _relerr(got, want):
    got, want = got.double().cpu(), want.double()
    return ((got - want).abs().max() / want.abs().max().clamp(min=1e-6)).item()


DEPTHS = (2, 2)


def _model():
    torch.manual_seed(0)
    return _swin(depths=DEPTHS, dim=64, heads=(2, 4), window=4, image=64)


def _run(dtype, **kw):
    ex = StageExecutor(GraphModel(_model().graph), DEV, dtype, **kw)
    x = torch.randn(2, 64, 64, 3, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        outs = [ex.run(x.to(DEV, dtype)).float().cpu() for _ in range(3)]
    return ex, x, outs


def test_swin_fp32_matches_the_cpu_model():
    _, x, (p32, _, _) = _run(torch.float32)
    with torch.no_grad():
        p_cpu = _model()(x)
    print(f"swin d(2,2) dim64 b2 64x64: max|p_fp32 - p_cpu| = "
          f"{(p32 - p_cpu).abs().max().item():.3e}")
    assert p32.shape == (2, 1000)
    assert torch.equal(p32.argmax(-1), p_cpu.argmax(-1))


def test_swin_bf16_fusion_and_hipgraph():
    """As for the ViT (test_attention_gpu.py): fusing an add into proj or
    mlp_2 saves one bf16 rounding at each of the two adds of a block, 2 *
    depth_total * u_b at the worst. A replayed hipGraph equals the eager
    run."""
    _, _, (fused, _, _) = _run(torch.bfloat16, fuse=True)
    _, _, (plain, _, _) = _run(torch.bfloat16, fuse=False)
    print(f"fused vs unfused: rel {_relerr(fused, plain):.4f}")
    assert _relerr(fused, plain) <= 2 * sum(DEPTHS) * UB
    assert ((fused.sum(-1) - 1).abs() < 1e-2).all()
    ex, _, replays = _run(torch.bfloat16, fuse=True, use_graph=True)
    assert ex._graph is not None, "stage did not capture"
    assert all(torch.equal(r, fused) for r in replays)
