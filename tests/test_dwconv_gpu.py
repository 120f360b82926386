"""GPU: the depthwise conv kernels (csrc/dwconv.hip), ReLU6 in the conv
epilogues and as an op, the lowered small MobileNetV2 and mobilenet_v2().

No tolerance here is measured. Exact-integer data must be torch.equal to
the CPU reference in both dtypes; random bf16 data uses the project's conv
tolerance (0.005 of the largest output: the two differ by one bf16 rounding
of the output, 2^-9); random fp32 data the forward error bound of a
length-R*S fmaf chain plus the epilogue, (R*S + 4) * 2^-24 * (|scale| *
sum|x*w| + |bias|), the form of test_ops_fp32_gpu.py."""

import functools

import pytest
import torch

import mobile_nets  # noqa: F401  (the nets of test_lower_mobile)
import test_lower_mobile as TL
from defer_amd import ops
from defer_amd.graph import GraphModel, LayerGraph
from defer_amd.models import mobilenet_v2
from defer_amd.ops import reference as ref
from defer_amd.parallel.pipeline import StageExecutor

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
DTYPES = (torch.float32, torch.bfloat16)
ACTS = ("none", "relu", "relu6")

# (N, H, W, C): one pixel; a strip shorter than the kernel's 4 (3x3) or 2
# (5x5) rows with 120 lanes per pixel; odd sizes under stride 2; C that is
# no multiple of 16 or 32; more than one block (14x14x144, 5x33x40)
SHAPES = [(1, 7, 7, 8), (2, 15, 9, 24), (1, 14, 14, 144), (3, 5, 33, 40),
          (1, 1, 1, 8), (1, 3, 2, 960)]
GEOMS = [(3, 1), (3, 2), (5, 1), (5, 2)]          # (R, stride)


def _relerr(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return ((got - want).abs().max()
            / want.abs().max().clamp(min=1e-6)).item()


def _pads(shape, R):
    _, H, W, _ = shape
    return [p for p in (0, R // 2) if H + 2 * p >= R and W + 2 * p >= R]


def _int_inputs(shape, R, seed):
    """x in [-2, 2], w in {-1, 0, 1}, scale in {1, 2}, bias in 0..2, so
    |y| <= 25*2*2 + 2 = 102: exact in bf16 and in fp32 in any order.
    Channel 0 is all 2 * 1 with scale 2, bias 2 (y >= 6 wherever a tap is
    in bounds, and one always is) and channel 1 all 2 * -1 (y < 0), so a
    ReLU6 output holds both a 0 and a 6 whatever the shape."""
    g = torch.Generator().manual_seed(seed)
    N, H, W, C = shape
    x = torch.randint(-2, 3, shape, generator=g).float()
    w = torch.randint(-1, 2, (R, R, C), generator=g).float()
    scale = torch.randint(1, 3, (C,), generator=g).float()
    bias = torch.randint(0, 3, (C,), generator=g).float()
    x[..., 0:2] = 2
    w[..., 0], w[..., 1] = 1, -1
    scale[0:2], bias[0:2] = 2, 2
    return x, w, scale, bias


@pytest.mark.parametrize("R,stride", GEOMS,
                         ids=[f"k{r}s{s}" for r, s in GEOMS])
@pytest.mark.parametrize("shape", SHAPES,
                         ids=["x".join(map(str, s)) for s in SHAPES])
def test_dwconv_exact_integers(shape, R, stride):
    pads = _pads(shape, R)
    assert pads, "every shape admits padding R // 2"
    for pad in pads:
        x, w, scale, bias = _int_inputs(shape, R, sum(shape) + R + pad)
        for act in ACTS:
            want = ref.dwconv2d_bn_act(x, w, scale, bias, stride, pad, act)
            assert want.abs().max() <= 102
            if act == "relu6":
                assert (want == 0).any() and (want == 6).any()
            for dt in DTYPES:
                got = ops.dwconv2d_bn_act(
                    x.to(DEV, dt), w.to(DEV, dt), scale.to(DEV),
                    bias.to(DEV), stride, pad, act)
                assert got.dtype == dt and got.shape == want.shape
                assert got.is_contiguous()
                assert torch.equal(got.float().cpu(), want), (pad, act, dt)


def test_dwconv_without_scale_and_bias():
    x, w, _, _ = _int_inputs((2, 15, 9, 24), 3, 5)
    want = ref.dwconv2d_bn_act(x, w, None, None, 1, 1, "none")
    for dt in DTYPES:
        got = ops.dwconv2d_bn_act(x.to(DEV, dt), w.to(DEV, dt), None, None,
                                  1, 1, "none")
        assert torch.equal(got.float().cpu(), want)


FLOAT_SHAPES = [(2, 15, 9, 24), (1, 14, 14, 144), (3, 5, 33, 40)]


@pytest.mark.parametrize("R,stride", GEOMS,
                         ids=[f"k{r}s{s}" for r, s in GEOMS])
@pytest.mark.parametrize("shape", FLOAT_SHAPES,
                         ids=["x".join(map(str, s)) for s in FLOAT_SHAPES])
def test_dwconv_random_floats(shape, R, stride):
    for pad in _pads(shape, R):
        g = torch.Generator().manual_seed(sum(shape) * 7 + R + stride + pad)
        C = shape[-1]
        x = torch.randn(*shape, generator=g)
        w = torch.randn(R, R, C, generator=g) * (2.0 / (R * R)) ** 0.5
        scale = torch.rand(C, generator=g) + 0.5
        bias = torch.randn(C, generator=g) * 0.5
        for act in ("none", "relu6"):
            # bf16: inputs rounded first, so only the output rounding and
            # the fp32 summation order differ from the reference
            xb, wb = x.bfloat16(), w.bfloat16()
            want = ref.dwconv2d_bn_act(xb.float(), wb.float(), scale, bias,
                                       stride, pad, act)
            got = ops.dwconv2d_bn_act(xb.to(DEV), wb.to(DEV), scale.to(DEV),
                                      bias.to(DEV), stride, pad, act)
            e = _relerr(got, want)
            print(f"bf16 {shape} k{R} s{stride} p{pad} {act}: rel err "
                  f"{e:.5f}")
            assert e < 0.005
            # fp32 against float64
            want64 = ref.dwconv2d_bn_act(
                x.double(), w.double(), scale.double(), bias.double(),
                stride, pad, act).double()
            mag = ref.dwconv2d_bn_act(
                x.abs().double(), w.abs().double(), scale.double(),
                bias.abs().double(), stride, pad, "none").double()
            got = ops.dwconv2d_bn_act(x.to(DEV), w.to(DEV), scale.to(DEV),
                                      bias.to(DEV), stride, pad, act)
            err = (got.double().cpu() - want64).abs()
            bound = (R * R + 4) * U * mag
            print(f"fp32 {shape} k{R} s{stride} p{pad} {act}: worst "
                  f"err/bound {(err / bound).max().item():.3f}")
            assert (err <= bound).all()


def test_dwconv_is_deterministic():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 28, 28, 192, generator=g).to(DEV, torch.bfloat16)
    w = torch.randn(3, 3, 192, generator=g).to(DEV, torch.bfloat16)
    a = ops.dwconv2d_bn_act(x, w, None, None, 2, 1, "relu6")
    for _ in range(3):
        assert torch.equal(ops.dwconv2d_bn_act(x, w, None, None, 2, 1,
                                               "relu6"), a)


def test_dwconv_rejects_what_the_kernels_do_not_serve():
    x = torch.zeros(1, 8, 8, 16, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(3, 3, 16, device=DEV, dtype=torch.bfloat16)
    call = ops.dwconv2d_bn_act
    with pytest.raises(RuntimeError, match="3x3 or 5x5"):
        call(x, torch.zeros(7, 7, 16, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="3x3 or 5x5"):
        call(x, torch.zeros(3, 5, 16, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="stride 1 or 2"):
        call(x, w, stride=3)
    with pytest.raises(RuntimeError, match="padding"):
        call(x, w, padding=2)
    with pytest.raises(RuntimeError, match="C % 8"):
        call(x[..., :12].contiguous(), w[..., :12].contiguous())
    with pytest.raises(RuntimeError, match="C % 4"):
        call(x[..., :6].float().contiguous(), w[..., :6].float().contiguous())
    with pytest.raises(RuntimeError, match="contiguous"):
        call(x.permute(0, 2, 1, 3), w)
    with pytest.raises(RuntimeError, match="channels"):
        call(x, w[..., :8].contiguous())
    with pytest.raises(RuntimeError, match="fp32|bf16"):
        call(x, w.float())
    with pytest.raises(RuntimeError, match="scale"):
        call(x, w, torch.ones(8, device=DEV))
    with pytest.raises(RuntimeError, match="larger than the padded input"):
        call(x[:, :2, :2].contiguous(), w, padding=0)
    with pytest.raises(ValueError, match="gelu"):
        call(x, w, act="gelu")
    # fp32 takes C % 4
    y = call(x[..., :12].float().contiguous(),
             w[..., :12].float().contiguous())
    assert y.shape == (1, 8, 8, 12)
    assert call(x[:0], w).shape == (0, 8, 8, 16)


# ------------------------------------------------- conv2d_bn_act + relu6
# the conv families MobileNetV2 reaches, and the 64 -> 64 3x3 at a size
# where the weight-stationary kernel is policy: (x shape, Cout, R, stride,
# pad, residual)
CONV_FAMILIES = {
    "expand16to96": ((2, 12, 12, 16), 96, 1, 1, 0, False),
    "project96to24res": ((2, 12, 12, 96), 24, 1, 1, 0, True),
    "last320to1280": ((1, 7, 7, 320), 1280, 1, 1, 0, False),
    "stem3to32s2": ((2, 33, 33, 3), 32, 3, 2, 1, False),
    "ws64to64": ((32, 32, 64, 64), 64, 3, 1, 1, False),
}


@pytest.mark.parametrize("name", sorted(CONV_FAMILIES))
def test_conv_relu6_on_mobilenet_families(name):
    xs, cout, R, stride, pad, has_res = CONV_FAMILIES[name]
    g = torch.Generator().manual_seed(len(name) * 101 + cout)
    cin = xs[-1]
    x = torch.randn(*xs, generator=g)
    w = torch.randn(cout, R, R, cin, generator=g) * (2.0 / (R * R * cin)) ** .5
    # a wide spread of scales, so that both clamps are hit in every family
    scale = torch.rand(cout, generator=g) * 8 + 0.5
    bias = torch.randn(cout, generator=g) * 2
    OH = (xs[1] + 2 * pad - R) // stride + 1
    OW = (xs[2] + 2 * pad - R) // stride + 1
    res = torch.randn(xs[0], OH, OW, cout, generator=g) if has_res else None
    if name == "ws64to64":
        plan = ops.conv_plan(xs, (cout, R, R, cin), stride, pad)
        assert plan["family"] == "ws"
    for dt in DTYPES:
        xd, wd = x.to(dt), w.to(dt)
        rd = None if res is None else res.to(dt)
        outs = {}
        before = ops.conv_ws_stats()["launches"]
        for act in ACTS:
            want = ref.conv2d_bn_act(xd.float(), wd.float(), scale, bias,
                                     stride, pad, act,
                                     None if rd is None else rd.float())
            got = ops.conv2d_bn_act(
                xd.to(DEV), wd.to(DEV), scale.to(DEV), bias.to(DEV), stride,
                pad, act, None if rd is None else rd.to(DEV))
            assert got.dtype == dt and got.shape == want.shape
            if dt == torch.bfloat16:
                e = _relerr(got, want)
                print(f"{name} bf16 {act}: rel err {e:.5f}")
                assert e < 0.005
            else:
                # a length-K chain plus four epilogue roundings
                want64 = ref.conv2d_bn_act(
                    x.double(), w.double(), scale.double(), bias.double(),
                    stride, pad, act,
                    None if res is None else res.double()).double()
                mag = ref.conv2d_bn_act(
                    x.abs().double(), w.abs().double(), scale.double(),
                    bias.abs().double(), stride, pad, "none",
                    None if res is None else res.abs().double()).double()
                err = (got.double().cpu() - want64).abs()
                bound = (R * R * cin + 4) * U * mag
                print(f"{name} fp32 {act}: worst err/bound "
                      f"{(err / bound).max().item():.3f}")
                assert (err <= bound).all()
            outs[act] = got
        if name == "ws64to64" and dt == torch.bfloat16:
            assert ops.conv_ws_stats()["launches"] == before + 3
        # relu6 is the relu output with the upper clamp, bit for bit (6 is
        # a bf16 number and rounding is monotone), and relu the clamp of
        # none: the relu6 epilogue changed nothing else
        assert torch.equal(outs["relu6"], outs["relu"].clamp(max=6))
        assert torch.equal(outs["relu"], outs["none"].clamp(min=0))
        assert (outs["relu6"] == 0).any() and (outs["relu6"] == 6).any()
        assert (outs["relu"] > 6).any()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
def test_relu6_op(dt):
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(3, 5, 7, 8, generator=g) * 6).to(dt)
    x.view(-1)[:6] = torch.tensor([-0.0, 0.0, 6.0, 6.5, -1.0, 5.96875]).to(dt)
    got = ops.relu6(x.to(DEV))
    assert got.dtype == dt and got.shape == x.shape
    assert torch.equal(got.cpu(), x.clamp(0, 6))
    assert (got == 0).any() and (got == 6).any()
    big = torch.randn(1 << 20, generator=g).to(dt) * 8      # > 2048 blocks
    assert torch.equal(ops.relu6(big.to(DEV)).cpu(), big.clamp(0, 6))
    with pytest.raises(RuntimeError, match="numel"):
        ops.relu6(torch.zeros(6, device=DEV, dtype=dt))   # relu's rules


# ------------------------------------------------------------ whole models
def _without_head(graph):
    """The graph up to its last 4-D node (before the global pool)."""
    i = next(i for i, n in enumerate(graph.nodes)
             if type(n.layer).__name__ == "GlobalAvgPool")
    return LayerGraph(graph.nodes[:i])


def test_lowered_tiny_mobilenet_exact_on_the_gpu():
    """Integer data (test_lower_mobile.exact_int_net asserts the premise):
    fp32 on the GPU EQUALS the torch model. In bf16 every 4-D value is an
    integer of at most 8 bits, so the features EQUAL the torch model's;
    the head's mean over 64 positions (k / 64, k up to 384) does not fit
    bf16's 8 bits, so the bf16 logits are compared with the same lowered
    graph run on the CPU in bf16, whose ops round where the kernels do."""
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
    # and those logits are the torch model's up to bf16's rounding of the
    # pooled features and of the logits themselves: 2 * 2^-9 of the largest
    assert _relerr(got, want) < 2.0 ** -8


def _mbv2():
    torch.manual_seed(0)
    return mobilenet_v2()


@functools.lru_cache(maxsize=None)
def _mb_input():
    return torch.randn(2, 96, 96, 3,
                       generator=torch.Generator().manual_seed(1))


@functools.lru_cache(maxsize=None)
def _mb_gpu(dtype, **kw):
    ex = StageExecutor(GraphModel(_mbv2().graph), DEV, dtype, **kw)
    with torch.no_grad():
        y = ex.run(_mb_input().to(DEV, dtype))
    assert y.dtype == dtype
    return y.float().cpu()


def test_mobilenet_v2_fp32_is_64x_closer_to_cpu_than_bf16():
    """The criterion of test_fp32_pipeline_gpu.py."""
    with torch.no_grad():
        p_cpu = _mbv2()(_mb_input()).float()
    p32 = _mb_gpu(torch.float32)
    p16 = _mb_gpu(torch.bfloat16)
    e32 = (p32 - p_cpu).abs().max().item()
    e16 = (p16 - p_cpu).abs().max().item()
    print(f"mobilenetv2 b2 96x96: max|p_fp32-p_cpu| = {e32:.3e}, "
          f"max|p_bf16-p_cpu| = {e16:.3e}, ratio = "
          f"{e16 / max(e32, 1e-300):.0f}")
    assert p32.shape == p_cpu.shape == (2, 1000)
    assert e32 <= e16 / 64
    assert torch.equal(p32.argmax(-1), p_cpu.argmax(-1))


def _integerize_zoo(model, seed=0):
    """torch_nets.integerize for the zoo's layers: weights -1 / 0 / +1 with
    about three non-zeros per output, scale 1 or 2, bias 0..2."""
    gen = torch.Generator().manual_seed(seed)

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=gen).float()

    with torch.no_grad():
        for n in model.graph.nodes:
            lay = n.layer
            w = getattr(lay, "weight", None)
            if w is None:
                continue
            depthwise = w.dim() == 3                # [R, S, C]
            fan_in = w[..., 0].numel() if depthwise else w[0].numel()
            keep = torch.rand(w.shape, generator=gen) < min(1.0, 3.0 / fan_in)
            w.copy_((ints(w.shape, 0, 1) * 2 - 1) * keep)
            if getattr(lay, "scale", None) is not None:
                lay.scale.copy_(ints(lay.scale.shape, 1, 2))
            if lay.bias is not None:
                lay.bias.copy_(ints(lay.bias.shape, 0, 2))
    return model


def test_mobilenet_v2_bf16_fused_unfused_and_hipgraph():
    """fuse_residual_adds adds the skip to the project conv's fp32
    accumulator, the unfused graph to its bf16 output: one rounding fewer,
    so with arbitrary weights the two differ in the last bf16 bit. With
    integer weights and input every 4-D value is an integer of at most 8
    bits (asserted on the CPU), nothing rounds, and the fused, the unfused
    and the captured graph must all EQUAL each other and, at the last conv,
    the CPU reference."""
    x = torch.randint(-2, 3, (2, 96, 96, 3),
                      generator=torch.Generator().manual_seed(5)).float()
    model = _integerize_zoo(_mbv2())
    vals = TL.node_values(model.graph, x)
    for name, v in vals.items():
        if v.dim() == 4:
            assert torch.equal(v, v.round()) and v.abs().max() <= 256, name
    feat = vals["Conv_1"]
    assert (feat == 0).any() and (feat == 6).any()
    assert (vals["block_9_add"] != 0).float().mean() > 0.25
    outs = {}
    for key, kw in (("fused", dict(fuse=True)), ("plain", dict(fuse=False)),
                    ("graph", dict(fuse=True, use_graph=True))):
        ex = StageExecutor(GraphModel(_integerize_zoo(_mbv2()).graph), DEV,
                           torch.bfloat16, **kw)
        with torch.no_grad():
            outs[key] = ex.run(x.to(DEV, torch.bfloat16)).float().cpu()
            if key == "graph":
                assert ex._graph is not None, "stage did not capture"
                outs["replay"] = ex.run(
                    x.to(DEV, torch.bfloat16)).float().cpu()
    assert torch.equal(outs["fused"], outs["plain"])
    assert torch.equal(outs["graph"], outs["fused"])
    assert torch.equal(outs["replay"], outs["fused"])
    assert ((outs["fused"].sum(-1) - 1).abs() < 1e-2).all()
    head = mobilenet_v2(include_top=False)
    head.load_state_dict(_integerize_zoo(_mbv2()).state_dict(), strict=False)
    ex = StageExecutor(GraphModel(head.graph), DEV, torch.bfloat16)
    with torch.no_grad():
        got = ex.run(x.to(DEV, torch.bfloat16))
    assert torch.equal(got.float().cpu(), feat)


def test_mobilenet_v2_random_weights_fp32_fusion_and_bf16_hipgraph():
    """Random weights: the passes do not change fp32 bits (the conv's
    epilogue and add_act run the same fp32 operations), and a bf16 hipGraph
    replay equals the eager run of the same stage graph."""
    assert torch.equal(_mb_gpu(torch.float32),
                       _mb_gpu(torch.float32, fuse=False))
    fused = _mb_gpu(torch.bfloat16)
    ex = StageExecutor(GraphModel(_mbv2().graph), DEV, torch.bfloat16,
                       use_graph=True)
    x = _mb_input().to(DEV, torch.bfloat16)
    with torch.no_grad():
        first = ex.run(x).float().cpu()       # captures, then replays once
        second = ex.run(x).float().cpu()      # replay
    torch.cuda.synchronize()
    assert ex._graph is not None, "stage did not capture"
    assert torch.equal(first, fused)
    assert torch.equal(second, fused)
