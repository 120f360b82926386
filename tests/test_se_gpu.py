"""GPU: the squeeze-excite kernels (csrc/se.hip), hardswish as an op and in
the conv and depthwise epilogues, the lowered small MobileNetV3 and
mobilenet_v3_large().

No tolerance here is measured. Exact data must be torch.equal to the CPU
reference in both dtypes; random squeeze-excite data is held to the derived
per-element bound of se_checks.py (docs/TESTING.md); the conv families use
the tolerances of test_conv_relu6_on_mobilenet_families, with 3 more
roundings for the activation in fp32."""

import functools

import pytest
import torch

import mobile_nets_v3  # noqa: F401  (the nets of test_lower_mobile_v3)
import se_checks
import test_lower_mobile_v3 as TL
from defer_amd import ops
from defer_amd.graph import GraphModel, LayerGraph
from defer_amd.models import mobilenet_v3_large
from defer_amd.ops import reference as ref
from defer_amd.parallel.pipeline import StageExecutor

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
DTYPES = (torch.float32, torch.bfloat16)
GRID_CAP_LANES = 2048 * 256     # of the 1-D kernels: more work iterates


def _relerr(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return ((got - want).abs().max()
            / want.abs().max().clamp(min=1e-6)).item()


def _dev(t, dt=None):
    if t is None:
        return None
    return t.to(DEV) if dt is None else t.to(DEV, dt)


def _se_gpu(x, w1, b1, w2, b2, act, dt):
    return ops.squeeze_excite(_dev(x, dt), _dev(w1, dt), _dev(b1),
                              _dev(w2, dt), _dev(b2), act)


# ------------------------------------------------- squeeze-excite, exact
def _exact_inputs(shape, cr, seed):
    """x[n, :, :, c] = a[n, c] + p(h, w) with integer a in [-4, 4] and a
    +-1 checkerboard p that sums to zero, so the mean is a exactly; integer
    w1, b1 and multiples of 3 in w2, b2, so every gate argument is a
    multiple of 3 and every gate exactly 0, 0.5 or 1. Channels 0, 1, 2 of
    the gate are 0.5, 1 and 0 for sure. |x| <= 5: x * g is exact in bf16,
    and every partial sum of the pool and the FCs is a small integer, exact
    in fp32 in any order."""
    n, h, w, c = shape
    assert (h * w) % 2 == 0
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-4, 5, (n, 1, 1, c), generator=g).float()
    hh, ww = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    p = (((hh * w + ww) % 2) * 2 - 1).float().view(1, h, w, 1)
    assert p.sum() == 0
    x = a + p
    w1 = torch.randint(-1, 2, (cr, c), generator=g).float()
    b1 = torch.randint(-2, 3, (cr,), generator=g).float()
    w2 = torch.randint(-1, 2, (c, cr), generator=g).float() * 3
    b2 = torch.randint(-1, 2, (c,), generator=g).float() * 3
    w2[:3] = 0
    b2[:3] = torch.tensor([0.0, 3.0, -3.0])
    return x, w1, b1, w2, b2


EXACT = [((2, 4, 4, 24), 8), ((1, 8, 8, 40), 16), ((3, 2, 1, 8), 3),
         ((1, 8, 8, 4104), 8)]


@pytest.mark.parametrize("shape,cr", EXACT,
                         ids=["x".join(map(str, s)) + f"-{r}"
                              for s, r in EXACT])
def test_squeeze_excite_exact_data(shape, cr):
    x, w1, b1, w2, b2 = _exact_inputs(shape, cr, sum(shape) + cr)
    for act in ("relu", "none"):
        want = ref.squeeze_excite(x, w1, b1, w2, b2, act)
        gate = se_checks.truth64(x, w1, b1, w2, b2, act)[2]
        assert set(gate.unique().tolist()) == {0.0, 0.5, 1.0}
        assert torch.equal(want.double(),
                           se_checks.truth64(x, w1, b1, w2, b2, act)[3])
        for dt in DTYPES:
            got = _se_gpu(x, w1, b1, w2, b2, act, dt)
            assert got.dtype == dt and got.shape == x.shape
            assert got.is_contiguous()
            assert torch.equal(got.float().cpu(), want), (act, dt)


# ------------------------------------------------ squeeze-excite, random
# (N, H, W, C) / Cr: one pixel and one vector; 9 vectors, HW = 49; fewer
# pixels than pixel groups; a long pixel loop with 2 vectors; more channel
# vectors than the gate block has lanes (514 fp32 at C = 2056, 513 bf16 and
# 1026 fp32 at C = 4104, for 512); Cr in {1, 6} (w2 rows read element by
# element) and 12 (vectors in fp32 only)
RANDOM = [((1, 1, 1, 8), 8), ((2, 7, 7, 72), 24), ((3, 5, 3, 960), 240),
          ((1, 56, 56, 16), 8), ((1, 2, 2, 2056), 8), ((1, 2, 2, 4104), 8),
          ((2, 7, 7, 72), 1), ((2, 7, 7, 72), 6), ((2, 3, 3, 40), 12)]


def _random_inputs(shape, cr, seed, bias=True):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) + 0.5
    w1 = torch.randn(cr, c, generator=g) * (2.0 / c) ** 0.5
    w2 = torch.randn(c, cr, generator=g) * 3 * (1.0 / cr) ** 0.5
    b1 = torch.randn(cr, generator=g) * 0.5 if bias else None
    b2 = torch.randn(c, generator=g) if bias else None
    return x, w1, b1, w2, b2


@pytest.mark.parametrize("shape,cr", RANDOM,
                         ids=["x".join(map(str, s)) + f"-{r}"
                              for s, r in RANDOM])
def test_squeeze_excite_random_data(shape, cr):
    for act, bias in (("relu", True), ("none", False)):
        x, w1, b1, w2, b2 = _random_inputs(shape, cr, sum(shape) * 3 + cr,
                                           bias)
        for dt in DTYPES:
            # the truth is computed from the rounded inputs
            xr, w1r, w2r = x.to(dt), w1.to(dt), w2.to(dt)
            got = _se_gpu(xr, w1r, b1, w2r, b2, act, dt)
            worst = se_checks.check_squeeze_excite(
                xr, w1r, b1, w2r, b2, act, got.cpu(),
                f"squeeze_excite {shape}/{cr} {act} {dt}")
            print(f"squeeze_excite {shape}/{cr} {act} {dt}: worst err/bound "
                  f"{worst:.3f}")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
def test_scale_pass_past_the_grid_cap(dt):
    shape, cr = (2, 48, 48, 960), 240
    per = 8 if dt == torch.bfloat16 else 4
    assert 2 * 48 * 48 * 960 // per > GRID_CAP_LANES
    x, w1, b1, w2, b2 = _random_inputs(shape, cr, 17)
    xr, w1r, w2r = x.to(dt), w1.to(dt), w2.to(dt)
    got = _se_gpu(xr, w1r, b1, w2r, b2, "relu", dt)
    worst = se_checks.check_squeeze_excite(xr, w1r, b1, w2r, b2, "relu",
                                           got.cpu())
    print(f"squeeze_excite {shape}/{cr} {dt}: worst err/bound {worst:.3f}")
    # the two launches apart give the same bits
    g = ops.se_gate(_dev(xr), _dev(w1r), _dev(b1), _dev(w2r), _dev(b2))
    assert g.dtype == torch.float32 and g.shape == (2, 960)
    assert torch.equal(ops.channel_scale(_dev(xr), g), got)


def test_squeeze_excite_is_deterministic():
    x, w1, b1, w2, b2 = _random_inputs((4, 14, 14, 480), 120, 5)
    for dt in DTYPES:
        args = (_dev(x, dt), _dev(w1, dt), _dev(b1), _dev(w2, dt), _dev(b2))
        a = ops.squeeze_excite(*args)
        for _ in range(3):
            assert torch.equal(ops.squeeze_excite(*args), a)


def test_squeeze_excite_rejects_what_the_kernels_do_not_serve():
    bf = dict(device=DEV, dtype=torch.bfloat16)
    x = torch.zeros(2, 4, 4, 16, **bf)
    w1, w2 = torch.zeros(8, 16, **bf), torch.zeros(16, 8, **bf)
    b1, b2 = torch.zeros(8, device=DEV), torch.zeros(16, device=DEV)
    call = ops.squeeze_excite
    assert call(x, w1, b1, w2, b2).shape == x.shape
    assert call(x, w1, None, w2, None).shape == x.shape
    with pytest.raises(RuntimeError, match="NHWC"):
        call(x[0], w1, b1, w2, b2)
    with pytest.raises(RuntimeError, match="contiguous"):
        call(x.permute(0, 2, 1, 3), w1, b1, w2, b2)
    with pytest.raises(RuntimeError, match="contiguous"):
        call(x, w2.t(), b1, w2, b2)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(torch.zeros(2 * 4 * 4 * 16 + 8, **bf)[4:-4].view(2, 4, 4, 16),
             w1, b1, w2, b2)
    with pytest.raises(RuntimeError, match="bf16|mixed dtypes"):
        call(x, w1.float(), b1, w2, b2)
    with pytest.raises(RuntimeError, match="mixed dtypes"):
        call(x.float(), w1, b1, w2, b2)
    with pytest.raises(RuntimeError, match="bf16 or fp32"):
        call(x.half(), w1.half(), b1, w2.half(), b2)
    with pytest.raises(RuntimeError, match=r"w1 must be \[Cr, C\]"):
        call(x, torch.zeros(8, 32, **bf), b1, w2, b2)
    with pytest.raises(RuntimeError, match=r"w2 must be \[C, Cr\]"):
        call(x, w1, b1, w1, b2)
    with pytest.raises(RuntimeError, match="b1 must be"):
        call(x, w1, b2, w2, b2)                 # fp32[16] where [8] goes
    with pytest.raises(RuntimeError, match="b2 must be"):
        call(x, w1, b1, w2, b2.bfloat16())
    with pytest.raises(RuntimeError, match="b1 must be"):
        call(x, w1, b1.cpu(), w2, b2)
    with pytest.raises(RuntimeError, match="C % 8"):
        call(x[..., :12].contiguous(), w1[:, :12].contiguous(), b1,
             w2[:12].contiguous(), b2[:12].contiguous())
    with pytest.raises(RuntimeError, match="empty spatial extent"):
        call(x[:, :0], w1, b1, w2, b2)
    with pytest.raises(ValueError, match="gelu"):
        call(x, w1, b1, w2, b2, act="gelu")
    with pytest.raises(ValueError, match="gate"):
        call(x, w1, b1, w2, b2, gate="sigmoid")
    # fp32 takes C % 4; N == 0 is an empty tensor
    y = call(x[..., :12].float().contiguous(),
             w1[:, :12].float().contiguous(), b1,
             w2[:12].float().contiguous(), b2[:12].contiguous())
    assert y.shape == (2, 4, 4, 12)
    y = call(x[:0], w1, b1, w2, b2)
    assert y.shape == (0, 4, 4, 16) and y.dtype == torch.bfloat16


# -------------------------------------------------------------- hardswish
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
def test_hardswish_op(dt):
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(3, 5, 7, 8, generator=g) * 6).to(dt)
    planted = torch.tensor([-3.0, -0.0, 0.0, 3.0, 2.984375, -3.015625, 6.5])
    x.view(-1)[:7] = planted.to(dt)
    assert torch.equal(x.view(-1)[:7].float(), planted)     # all bf16 numbers
    got = ops.hardswish(x.to(DEV))
    assert got.dtype == dt and got.shape == x.shape
    assert torch.equal(got.cpu(), ref.hardswish(x))
    head = got.view(-1)[:7].float().cpu()
    assert torch.equal(head[[0, 1, 2, 3, 5, 6]],
                       torch.tensor([0.0, 0.0, 0.0, 3.0, 0.0, 6.5]))
    # on the ramp: 2.97658... in fp32, which bf16 rounds back up to x
    assert 2.96 < head[4] < 2.984375 or dt == torch.bfloat16
    # v for v >= 3 and 0 for v <= -3, bit for bit
    hi, lo = x >= 3, x <= -3
    assert hi.any() and lo.any()
    assert torch.equal(got.cpu()[hi], x[hi]) and not got.cpu()[lo].any()
    per = 8 if dt == torch.bfloat16 else 4
    big = torch.randn((GRID_CAP_LANES + 1000) * per, generator=g).to(dt) * 6
    assert torch.equal(ops.hardswish(big.to(DEV)).cpu(), ref.hardswish(big))
    with pytest.raises(RuntimeError, match="numel"):
        ops.hardswish(torch.zeros(6, device=DEV, dtype=dt))  # relu's rules


def _check_hardswish_of(o, hs):
    """hs is a kernel's hardswish output and o the same kernel's output
    with act "none". Both kernels apply the activation to the fp32 value v
    and round once. In fp32 o is v, so hs EQUALS the reference hardswish of
    o, hence o where o >= 3 and 0 where o <= -3. In bf16 o is v rounded:
    hardswish is v itself for v >= 3 and rounding is monotone, so o > 3
    gives hs == o and o < -3 gives 0, bit for bit. At o == +-3 itself v may
    lie up to half an ulp (2^-7) inside the ramp, where v * (v + 3) / 6 is
    just below v at +3 (it rounds to 3 or to the bf16 number below,
    2.984375) and within 3 * 2^-7 / 6 = 2^-8 of zero at -3: those elements
    are held to exactly that, not skipped."""
    if o.dtype == torch.float32:
        assert torch.equal(hs, ref.hardswish(o))
        hi, lo = o >= 3, o <= -3
    else:
        hi, lo = o > 3, o < -3
        at = o == 3
        assert ((hs[at] == 3) | (hs[at] == 2.984375)).all()
        at = o == -3
        assert (hs[at].float().abs() <= 2.0 ** -8).all()
        assert (hs[at] <= 0).all()
    assert hi.any() and lo.any() and ((o > -3) & (o < 3)).any()
    assert torch.equal(hs[hi], o[hi])
    assert not hs[lo].any()


# the conv families MobileNetV3 reaches: (x shape, Cout, R, stride, pad,
# residual)
CONV_FAMILIES = {
    "stem3to16s2": ((2, 33, 33, 3), 16, 3, 2, 1, False),
    "expand80to200": ((2, 6, 6, 80), 200, 1, 1, 0, False),
    "expand112to672": ((2, 6, 6, 112), 672, 1, 1, 0, False),
    "last160to960": ((2, 3, 3, 160), 960, 1, 1, 0, False),
    "project672to112res": ((2, 6, 6, 672), 112, 1, 1, 0, True),
}


@pytest.mark.parametrize("name", sorted(CONV_FAMILIES))
def test_conv_hardswish_on_mobilenet_v3_families(name):
    """bf16 within 0.005 of the largest output, fp32 within (K + 4 + 3)u of
    the magnitude sum (3 for the activation's add, product and product).
    One rounding in bf16 too: against a float64 truth t of the rounded
    inputs, |got - t| <= u_b |t| + 3/2 (K + 7) u mag per element, u_b = 2^-8
    the worst case of one rounding to bf16 and 3/2 the largest slope of
    hardswish, which carries the fp32 error of its argument. An activation
    applied to the already rounded conv output adds up to 3/2 u_b |v| and
    breaks this. Bit for bit: _check_hardswish_of. The project conv with a
    residual and no activation is unchanged: it is its own reference run."""
    xs, cout, R, stride, pad, has_res = CONV_FAMILIES[name]
    g = torch.Generator().manual_seed(len(name) * 101 + cout)
    cin = xs[-1]
    K = R * R * cin
    x = torch.randn(*xs, generator=g)
    w = torch.randn(cout, R, R, cin, generator=g) * (2.0 / K) ** .5
    # a wide spread of scales, so that both exact regions are hit
    scale = torch.rand(cout, generator=g) * 8 + 0.5
    bias = torch.randn(cout, generator=g) * 2
    OH = (xs[1] + 2 * pad - R) // stride + 1
    OW = (xs[2] + 2 * pad - R) // stride + 1
    res = torch.randn(xs[0], OH, OW, cout, generator=g) if has_res else None
    acts = ("none",) if has_res else ("none", "relu", "hardswish")
    for dt in DTYPES:
        xd, wd = x.to(dt), w.to(dt)
        rd = None if res is None else res.to(dt)
        outs = {}
        for act in acts:
            want = ref.conv2d_bn_act(xd.float(), wd.float(), scale, bias,
                                     stride, pad, act,
                                     None if rd is None else rd.float())
            got = ops.conv2d_bn_act(
                xd.to(DEV), wd.to(DEV), scale.to(DEV), bias.to(DEV), stride,
                pad, act, None if rd is None else rd.to(DEV))
            assert got.dtype == dt and got.shape == want.shape
            # float64 truth and magnitude sum of the inputs as rounded
            want64 = ref.conv2d_bn_act(
                xd.double(), wd.double(), scale.double(), bias.double(),
                stride, pad, "none",
                None if rd is None else rd.double()).double()
            if act == "relu":
                want64 = want64.clamp(min=0)
            elif act == "hardswish":
                want64 = want64 * (want64 + 3).clamp(0, 6) / 6
            mag = ref.conv2d_bn_act(
                xd.abs().double(), wd.abs().double(), scale.double(),
                bias.abs().double(), stride, pad, "none",
                None if rd is None else rd.abs().double()).double()
            err = (got.double().cpu() - want64).abs()
            if dt == torch.bfloat16:
                e = _relerr(got, want)
                print(f"{name} bf16 {act}: rel err {e:.5f}")
                assert e < 0.005
                bound = 2.0 ** -8 * want64.abs() + 1.5 * (K + 7) * U * mag
                print(f"{name} bf16 {act}: worst err/one-rounding bound "
                      f"{(err / bound).max().item():.3f}")
                assert (err <= bound).all()
            else:
                bound = (K + 4 + (3 if act == "hardswish" else 0)) * U * mag
                print(f"{name} fp32 {act}: worst err/bound "
                      f"{(err / bound).max().item():.3f}")
                assert (err <= bound).all()
            outs[act] = got.cpu()
        if has_res:
            continue
        o, hs = outs["none"], outs["hardswish"]
        assert torch.equal(outs["relu"], o.clamp(min=0))    # relu untouched
        _check_hardswish_of(o, hs)


DW_SHAPES = [(2, 15, 9, 24), (1, 14, 14, 144), (1, 3, 2, 960)]
DW_GEOMS = [(3, 1), (3, 2), (5, 1), (5, 2)]          # (R, stride)


@pytest.mark.parametrize("R,stride", DW_GEOMS,
                         ids=[f"k{r}s{s}" for r, s in DW_GEOMS])
@pytest.mark.parametrize("shape", DW_SHAPES,
                         ids=["x".join(map(str, s)) for s in DW_SHAPES])
def test_dwconv_hardswish_exact_integers(shape, R, stride):
    """x in [-2, 2], w in {-1, 0, 1}, scale 3 and bias in {-3, 0, 3}: every
    hardswish argument is a multiple of 3 with |v| <= 25*2*3 + 3 = 153, so
    it lies in the exact regions and the output (v or 0) is exact in bf16.
    Channel 0 is all 2 * 1 (v >= 3) and channel 1 all 2 * -1 (v <= -3)."""
    pad = R // 2
    g = torch.Generator().manual_seed(sum(shape) + R + stride)
    C = shape[-1]
    x = torch.randint(-2, 3, shape, generator=g).float()
    w = torch.randint(-1, 2, (R, R, C), generator=g).float()
    scale = torch.full((C,), 3.0)
    bias = torch.randint(-1, 2, (C,), generator=g).float() * 3
    x[..., 0:2] = 2
    w[..., 0], w[..., 1] = 1, -1
    bias[0:2] = 0
    v = ref.dwconv2d_bn_act(x, w, scale, bias, stride, pad, "none")
    assert torch.equal(v, (v / 3).round() * 3) and v.abs().max() <= 153
    assert (v >= 3).any() and (v <= -3).any() and (v == 0).any()
    want = ref.dwconv2d_bn_act(x, w, scale, bias, stride, pad, "hardswish")
    assert torch.equal(want, v.clamp(min=0))
    for dt in DTYPES:
        args = (x.to(DEV, dt), w.to(DEV, dt), scale.to(DEV), bias.to(DEV),
                stride, pad)
        got = ops.dwconv2d_bn_act(*args, "hardswish")
        assert got.dtype == dt and got.shape == want.shape
        assert torch.equal(got.float().cpu(), want), dt
        # relu and none are what they were
        assert torch.equal(ops.dwconv2d_bn_act(*args, "none").float().cpu(), v)
        assert torch.equal(ops.dwconv2d_bn_act(*args, "relu").float().cpu(),
                           v.clamp(min=0))
        assert torch.equal(ops.dwconv2d_bn_act(*args, "relu6").float().cpu(),
                           v.clamp(0, 6))


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
def test_dwconv_hardswish_random_floats(dt):
    """On arbitrary data the depthwise epilogue applies the reference
    hardswish to the fp32 value and rounds once: _check_hardswish_of, the
    elements at +-3 included."""
    g = torch.Generator().manual_seed(23)
    x = (torch.randn(2, 14, 14, 40, generator=g) * 2).to(dt)
    w = torch.randn(5, 5, 40, generator=g).to(dt) * 0.4
    scale = torch.rand(40, generator=g) * 4 + 0.5
    bias = torch.randn(40, generator=g)
    args = (x.to(DEV), w.to(DEV), scale.to(DEV), bias.to(DEV), 2, 2)
    o = ops.dwconv2d_bn_act(*args, "none").cpu()
    hs = ops.dwconv2d_bn_act(*args, "hardswish").cpu()
    if dt == torch.bfloat16:
        want = ref.dwconv2d_bn_act(x.float(), w.float(), scale, bias, 2, 2,
                                   "hardswish")
        assert _relerr(hs, want) < 0.005
    _check_hardswish_of(o, hs)


# ------------------------------------------------------------ whole models
def _without_head(graph):
    """The graph up to its last 4-D node (before the global pool)."""
    i = next(i for i, n in enumerate(graph.nodes)
             if type(n.layer).__name__ == "GlobalAvgPool")
    return LayerGraph(graph.nodes[:i])


def test_lowered_tiny_mobilenet_v3_exact_on_the_gpu():
    """The exact-integer set-up (test_lower_mobile_v3.exact_int_net asserts
    the premise): fp32 on the GPU EQUALS the torch model. In bf16 every 4-D
    value is a multiple of 1/2 of at most 8 bits and the gates are fp32, so
    the features EQUAL the torch model's. The head's mean over 64 positions
    does not fit bf16's 8 bits, so the bf16 logits are compared with the
    same lowered graph run on the CPU in bf16, whose ops round where the
    kernels do."""
    net, x, g, want = TL.exact_int_net()
    ex = StageExecutor(GraphModel(g), DEV, torch.float32)
    got = ex.run(x.to(DEV))
    assert got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)

    _, _, g16, _ = TL.exact_int_net()
    with torch.no_grad():
        feat = net.features(x)                              # NCHW
        want16 = g16.forward(x.bfloat16())
    assert want16.dtype == torch.bfloat16
    ex = StageExecutor(GraphModel(_without_head(g16)), DEV, torch.bfloat16)
    got = ex.run(x.to(DEV, torch.bfloat16))
    assert got.dtype == torch.bfloat16
    assert torch.equal(got.float().cpu(), feat.permute(0, 2, 3, 1))
    _, _, g16, _ = TL.exact_int_net()
    ex = StageExecutor(GraphModel(g16), DEV, torch.bfloat16)
    got = ex.run(x.to(DEV, torch.bfloat16))
    assert torch.equal(got.cpu(), want16)
    # and those logits are the torch model's up to bf16's four roundings in
    # the head (pooled features, Linear, Hardswish, logits), 2^-9 each, the
    # hardswish's slope of at most 3/2 on the first two, relative to the sum
    # of magnitudes, which with about two non-zero weights per output is at
    # most twice the largest value: (2 * 3/2 + 2) * 2^-9 * 2 < 2^-5
    assert _relerr(got, want) < 2.0 ** -5


def _mbv3():
    torch.manual_seed(0)
    return mobilenet_v3_large()


@functools.lru_cache(maxsize=None)
def _mb_input():
    return torch.randn(2, 96, 96, 3,
                       generator=torch.Generator().manual_seed(1))


@functools.lru_cache(maxsize=None)
def _mb_gpu(dtype, **kw):
    ex = StageExecutor(GraphModel(_mbv3().graph), DEV, dtype, **kw)
    with torch.no_grad():
        y = ex.run(_mb_input().to(DEV, dtype))
    assert y.dtype == dtype
    return y.float().cpu()


def test_mobilenet_v3_large_fp32_is_64x_closer_to_cpu_than_bf16():
    """The criterion of test_fp32_pipeline_gpu.py."""
    with torch.no_grad():
        p_cpu = _mbv3()(_mb_input()).float()
    p32 = _mb_gpu(torch.float32)
    p16 = _mb_gpu(torch.bfloat16)
    e32 = (p32 - p_cpu).abs().max().item()
    e16 = (p16 - p_cpu).abs().max().item()
    print(f"mobilenetv3large b2 96x96: max|p_fp32-p_cpu| = {e32:.3e}, "
          f"max|p_bf16-p_cpu| = {e16:.3e}, ratio = "
          f"{e16 / max(e32, 1e-300):.0f}")
    assert p32.shape == p_cpu.shape == (2, 1000)
    assert e32 <= e16 / 64
    assert torch.equal(p32.argmax(-1), p_cpu.argmax(-1))


def test_mobilenet_v3_large_fp32_fusion_and_bf16_hipgraph():
    """The passes do not change fp32 bits (the conv's epilogue and add_act
    run the same fp32 operations), and a bf16 hipGraph replay, squeeze-excite
    launches included, equals the eager run of the same stage graph."""
    assert torch.equal(_mb_gpu(torch.float32),
                       _mb_gpu(torch.float32, fuse=False))
    fused = _mb_gpu(torch.bfloat16)
    ex = StageExecutor(GraphModel(_mbv3().graph), DEV, torch.bfloat16,
                       use_graph=True)
    x = _mb_input().to(DEV, torch.bfloat16)
    with torch.no_grad():
        first = ex.run(x).float().cpu()       # captures, then replays once
        second = ex.run(x).float().cpu()      # replay
    torch.cuda.synchronize()
    assert ex._graph is not None, "stage did not capture"
    assert torch.equal(first, fused)
    assert torch.equal(second, fused)
    ex = StageExecutor(GraphModel(_mbv3().graph), DEV, torch.float32,
                       use_graph=True)
    x = _mb_input().to(DEV)
    with torch.no_grad():
        ex.run(x)
        replay = ex.run(x).float().cpu()
    assert ex._graph is not None, "stage did not capture"
    assert torch.equal(replay, _mb_gpu(torch.float32))
