"""Lowering FX-imported torch models onto the NHWC layers (defer_amd.lower),
the layout ops and the from_torch module-reuse fix, on the CPU.

The lowered graph runs the fp32 reference ops here; the same graphs run
the HIP kernels in test_lower_torch_gpu.py."""

import queue
import threading

import pytest
import torch
import torch.nn as nn

import torch_nets as T
from defer_amd import DEFER, PipelineConfig, ops
from defer_amd.graph import GraphModel, LayerGraph, from_torch
from defer_amd.lower import lower_torch, lowering_report
from defer_amd.models import layers as L
from defer_amd.parallel.partitioner import as_graph_model

TV_SHAPE = (2, 3, 32, 32)
VGG_SHAPE = (2, 3, 8, 8)
SMALL_SHAPE = (2, 3, 16, 16)

# Random-float gate: lowered fp32 error over the torch model's own fp32
# error, both against a float64 run of the torch model. The two differ by
# reassociation only, (conv + b - mean) * s + beta against conv * s + bias'.
# Observed on seeds 0..4 (docs/TESTING.md): worst 2.71 (island net, whose
# torch error that seed is 6e-8, two ulps), so the gate is 4 x 2.71.
RATIO_GATE = 11.0
ERR_FLOOR = 2.0 ** -24          # half an fp32 ulp: a torch error of zero
#                                 must not make the gate zero


def _kept(graph):
    return [(n, r) for n, r in lowering_report(graph) if r != "lowered"]


def _types(graph):
    return {n.name: type(n.layer) for n in graph.nodes}


def _relerr64(y, ref):
    return ((y.double() - ref).abs().max() / ref.abs().max()).item()


def _check_against_float64(cls, shape, seeds=range(5), **kw):
    for seed in seeds:
        gen = torch.Generator().manual_seed(seed)
        torch.manual_seed(seed)
        net = T.randomize_bn(cls(**kw).eval(), gen)
        x = torch.randn(*shape, generator=gen)
        with torch.no_grad():
            ref = T.as_double(net)(x.double())
            e_torch = _relerr64(net(x), ref)
            e_low = _relerr64(lower_torch(net, shape).forward(x), ref)
        print(f"{cls.__name__} seed {seed}: torch {e_torch:.3e} "
              f"lowered {e_low:.3e} ratio {e_low / max(e_torch, 1e-30):.2f}")
        assert e_low <= RATIO_GATE * max(e_torch, ERR_FLOOR), (
            cls.__name__, seed, e_torch, e_low)


# ------------------------------------------------------- 1. exact integers
@pytest.mark.parametrize("cls,shape", [(T.TVBlock, TV_SHAPE),
                                       (T.VGGHead, VGG_SHAPE)])
def test_exact_integers(cls, shape):
    """Small-integer inputs and parameters: fp32 arithmetic is exact, so
    the lowered graph must EQUAL the torch model. A wrong flatten
    permutation, BN fold sign, a dropped conv bias or OIHW read as OHWI
    all fail here."""
    net = T.integerize(cls().eval())
    x = T.int_input(shape)
    with torch.no_grad():
        want = net(x)
        # the premise: nothing rounded (the softmax of VGGHead aside) and
        # the ReLUs did not kill the signal
        logits_net = net if cls is T.TVBlock else nn.Sequential(
            net.features, net.flatten, net.classifier)
        logits = logits_net(x)
        assert torch.equal(logits.double(),
                           T.as_double(logits_net)(x.double()))
        assert (logits != 0).float().mean() >= 0.5
        got = lower_torch(net, shape).forward(x)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got, want)


def test_flatten_permutation_is_needed():
    """The VGG head's first Linear really depends on the column order: the
    lowered graph with the torch weight put back differs."""
    net = T.integerize(T.VGGHead().eval())
    x = T.int_input(VGG_SHAPE)
    g = lower_torch(net, VGG_SHAPE)
    dense = g.by_name["classifier_1"].layer
    assert not torch.equal(dense.weight, net.classifier[0].weight)
    with torch.no_grad():
        dense.weight.copy_(net.classifier[0].weight)
        assert not torch.equal(g.forward(x), net(x))


# -------------------------------------------------------- 2. random floats
@pytest.mark.parametrize("cls,shape", [
    (T.TVBlock, TV_SHAPE), (T.VGGHead, VGG_SHAPE), (T.CatNet, SMALL_SHAPE)])
def test_random_floats_within_reassociation(cls, shape):
    _check_against_float64(cls, shape)


# ------------------------------------------------------------ 3. structure
def test_tv_block_lowers_completely():
    net = T.TVBlock().eval()
    g = lower_torch(net, TV_SHAPE)
    assert _kept(g) == []
    gm = GraphModel(g)
    assert not [m for m in gm.modules()
                if isinstance(m, (nn.Conv2d, nn.BatchNorm2d, nn.Linear,
                                  L.TorchIsland))]
    ty = _types(g)
    assert [n for n, t in ty.items() if t is L.ToNHWC] == ["input__nhwc"]
    assert g.by_name["input__nhwc"].inputs == [LayerGraph.INPUT]
    assert L.ToNCHW not in ty.values()
    # each conv + bn + relu is ONE node named after the relu call; the
    # shared self.relu gives relu, relu_1, relu_2 per block
    for name in ("relu", "block1_relu", "block1_relu_1", "block2_relu",
                 "block2_relu_1"):
        assert ty[name] is L.ConvBNAct and g.by_name[name].layer.act == "relu"
    for name in ("block1_bn3", "block1_downsample_1", "block2_bn3"):
        assert ty[name] is L.ConvBNAct and g.by_name[name].layer.act == "none"
    for name in ("block1_relu_2", "block2_relu_2"):
        assert ty[name] is L.AddAct and g.by_name[name].layer.act == "relu"
    assert ty["maxpool"] is L.MaxPool
    assert ty["flatten"] is L.GlobalAvgPool and ty["fc"] is L.Dense
    assert len(g.nodes) == 14
    assert not any("conv" in n for n in ty)     # all fused away


def test_vgg_head_structure():
    g = lower_torch(T.VGGHead().eval(), VGG_SHAPE)
    assert _kept(g) == []
    assert [(n.name, type(n.layer)) for n in g.nodes] == [
        ("input__nhwc", L.ToNHWC), ("features_1", L.ConvBNAct),
        ("features_3", L.ConvBNAct), ("features_4", L.MaxPool),
        ("flatten", L.Flatten), ("classifier_1", L.Dense),
        ("classifier_3", L.Dense), ("softmax", L.Softmax)]
    assert g.by_name["classifier_1"].layer.act == "relu"
    # the eval Dropout is gone: the second Linear reads the first
    assert g.by_name["classifier_3"].inputs == ["classifier_1"]


def test_cat_net_lowers_with_shared_input_conversion():
    g = lower_torch(T.CatNet().eval(), SMALL_SHAPE)
    assert _kept(g) == []
    ty = _types(g)
    # x feeds c1 and both cats: one shared conversion
    assert [n for n, t in ty.items() if t is L.ToNHWC] == ["input__nhwc"]
    assert ty["cat"] is L.Concat and ty["cat_1"] is L.Concat
    assert g.by_name["cat_1"].inputs == ["input__nhwc", "relu", "relu_1"]
    assert ty["mean"] is L.GlobalAvgPool


def test_4d_output_returns_nchw():
    class Feat(nn.Module):
        def __init__(self):
            super().__init__()
            self.c = nn.Conv2d(3, 8, 3, padding=1)

        def forward(self, x):
            return torch.relu(self.c(x))

    net = Feat().eval()
    g = lower_torch(net, SMALL_SHAPE)
    assert g.output == "relu__nchw"
    assert isinstance(g.by_name["relu__nchw"].layer, L.ToNCHW)
    x = torch.randn(*SMALL_SHAPE)
    with torch.no_grad():
        want = net(x)
        got = g.forward(x)
    assert got.shape == want.shape and got.is_contiguous()
    assert torch.allclose(got, want, atol=1e-6)


def test_training_mode_raises():
    with pytest.raises(ValueError, match="eval"):
        lower_torch(T.TVBlock(), TV_SHAPE)


# -------------------------------------------------------------- 4. islands
def test_island_net_keeps_grouped_conv_and_sigmoid():
    net = T.IslandNet().eval()
    g = lower_torch(net, SMALL_SHAPE)
    kept = _kept(g)
    assert [n for n, _ in kept] == ["grouped", "sig"]
    assert "groups=2" in kept[0][1] and "Sigmoid" in kept[1][1]
    names = g.layer_names()
    conv = [n for n in names if "__" in n]
    assert conv == ["input__nhwc", "relu__nchw", "sig__nhwc"]
    assert names.index("relu__nchw") < names.index("grouped")
    assert names.index("sig") < names.index("sig__nhwc")
    assert g.by_name["grouped"].inputs == ["relu__nchw"]
    assert g.by_name["sig"].inputs == ["grouped"]       # NCHW to NCHW
    assert isinstance(g.by_name["grouped"].layer, L.TorchIsland)
    _check_against_float64(T.IslandNet, SMALL_SHAPE)


def test_strict_names_every_kept_node():
    with pytest.raises(ValueError) as e:
        lower_torch(T.IslandNet().eval(), SMALL_SHAPE, strict=True)
    msg = str(e.value)
    assert "grouped" in msg and "sig" in msg and "groups=2" in msg
    lower_torch(T.TVBlock().eval(), TV_SHAPE, strict=True)   # nothing kept


def test_padded_avgpool_counting_pads_stays_an_island():
    g = lower_torch(T.AvgPoolNet(True).eval(), SMALL_SHAPE)
    kept = _kept(g)
    assert [n for n, _ in kept] == ["pool"]
    assert "count_include_pad" in kept[0][1]
    _check_against_float64(T.AvgPoolNet, SMALL_SHAPE, seeds=range(2),
                           count_include_pad=True)
    g = lower_torch(T.AvgPoolNet(False).eval(), SMALL_SHAPE)
    assert _kept(g) == [] and _types(g)["pool"] is L.AvgPool
    _check_against_float64(T.AvgPoolNet, SMALL_SHAPE, seeds=range(2),
                           count_include_pad=False)


def test_island_follows_the_dtype_of_its_input():
    """StageExecutor leaves a torch module with a bf16 weight and an fp32
    bias; the island casts its own parameters to what comes in."""
    isl = L.TorchIsland(nn.Conv2d(4, 4, 3, padding=1, groups=2), "test")
    isl.inner.weight.data = isl.inner.weight.data.to(torch.bfloat16)
    y = isl(torch.randn(1, 4, 5, 5, dtype=torch.bfloat16))
    assert y.dtype == torch.bfloat16
    assert isl.inner.bias.dtype == torch.bfloat16
    assert isl(torch.randn(1, 4, 5, 5)).dtype == torch.float32


# ------------------------------------------------------------- 5. legality
def test_twelve_channel_pool_stays_an_island():
    g = lower_torch(T.TwelveNet().eval(), SMALL_SHAPE)
    kept = _kept(g)
    assert [n for n, _ in kept] == ["pool"]
    assert "C % 8" in kept[0][1]
    ty = _types(g)
    assert ty["relu"] is L.ConvBNAct            # Cout = 12 is legal
    assert g.by_name["pool"].inputs == ["relu__nchw"]
    assert g.by_name["relu_1"].inputs == ["pool__nhwc"]
    _check_against_float64(T.TwelveNet, SMALL_SHAPE)


def test_illegal_linear_keeps_its_flatten_in_torch_order():
    """A flatten whose Linear cannot lower (K % 8) must not be lowered
    either, or the island would read (h, w, c) columns."""
    class Odd(nn.Module):
        def __init__(self):
            super().__init__()
            self.c = nn.Conv2d(3, 4, 3, padding=1)
            self.fc = nn.Linear(4 * 3 * 3, 8)       # K = 36

        def forward(self, x):
            return self.fc(torch.relu(self.c(x)).flatten(1))

    net = Odd().eval()
    g = lower_torch(net, (2, 3, 3, 3))
    assert [n for n, _ in _kept(g)] == ["flatten", "fc"]
    x = torch.randn(2, 3, 3, 3)
    with torch.no_grad():
        assert torch.allclose(g.forward(x), net(x), atol=1e-6)


class _Head(nn.Module):
    """conv-relu, mean, Linear(8, n) [+ ReLU]."""

    def __init__(self, n, relu=True):
        super().__init__()
        self.c = nn.Conv2d(3, 8, 3, padding=1)
        self.fc = nn.Linear(8, n)
        self.act = nn.ReLU() if relu else nn.Identity()

    def forward(self, x):
        return self.act(self.fc(torch.relu(self.c(x)).mean(dim=(2, 3))))


def test_dense_takes_its_relu_only_where_ops_relu_takes_the_output():
    """Dense(act="relu") runs ops.relu on the [M, N] output (numel % 8):
    at batch 1 with N = 100 the Linear lowers alone and the ReLU stays
    torch code; at batch 2 (200 elements) it is taken in."""
    net = _Head(100).eval()
    g = lower_torch(net, (1, 3, 8, 8))
    kept = _kept(g)
    assert [n for n, _ in kept] == ["act"] and "numel % 8" in kept[0][1]
    assert _types(g)["fc"] is L.Dense and g.by_name["fc"].layer.act == "none"
    x = torch.randn(1, 3, 8, 8)
    with torch.no_grad():
        assert torch.allclose(g.forward(x), net(x), atol=1e-6)
    g = lower_torch(net, (2, 3, 8, 8))
    assert _kept(g) == [] and "fc" not in g.by_name
    assert g.by_name["act"].layer.act == "relu"


def test_linear_wider_than_the_cached_scale_stays_an_island():
    """The bf16 linear passes no scale, and the bindings' cached ones
    vector holds 8192."""
    g = lower_torch(_Head(10000, relu=False).eval(), (2, 3, 8, 8))
    kept = _kept(g)
    assert [n for n, _ in kept] == ["fc"] and "8192" in kept[0][1]
    g = lower_torch(_Head(8192, relu=False).eval(), (2, 3, 8, 8))
    assert _kept(g) == [] and _types(g)["fc"] is L.Dense


def test_in_place_ops_are_seen_by_later_readers():
    """torch writes an in-place ReLU or `a += b` into its input: a later
    reader of that tensor sees the result, an earlier one does not."""
    class Relu(nn.Module):
        def __init__(self, inplace):
            super().__init__()
            self.c = nn.Conv2d(3, 8, 3, padding=1)
            self.bn = nn.BatchNorm2d(8)
            self.pool = nn.MaxPool2d(1)
            self.relu = nn.ReLU(inplace=inplace)

        def forward(self, x):
            y = self.bn(self.c(x))
            before = self.pool(y)       # reads y before the ReLU
            z = self.relu(y)
            return z + y + before       # y: mutated iff inplace

    class Iadd(nn.Module):
        def __init__(self):
            super().__init__()
            self.c1 = nn.Conv2d(3, 8, 3, padding=1)
            self.c2 = nn.Conv2d(3, 8, 3, padding=1)

        def forward(self, x):
            a = self.c1(x)
            b = self.c2(x)
            a += b
            r = torch.relu(a)
            return r - a                # a is the sum here: zero where > 0

    gen = torch.Generator().manual_seed(17)
    x = torch.randn(2, 3, 8, 8, generator=gen)
    for net in (Relu(True), Relu(False), Iadd()):
        net = T.randomize_bn(net.eval(), gen)
        g = lower_torch(net, (2, 3, 8, 8))
        with torch.no_grad():
            want = net(x.clone())
            got = g.forward(x.clone())
        assert torch.allclose(got, want, atol=1e-5), type(net).__name__
    # the two ReLU variants really differ, so the test can tell them apart
    a, b = Relu(True).eval(), Relu(False).eval()
    b.load_state_dict(a.state_dict())
    with torch.no_grad():
        assert not torch.allclose(a(x.clone()), b(x.clone()))


def test_model_off_the_cpu_is_refused_readably():
    with pytest.raises(ValueError, match="model.cpu\\(\\)"):
        lower_torch(T.TVBlock().eval().to("meta"), TV_SHAPE)


# ---------------------------------------------------------------- 6. reuse
def test_from_torch_takes_a_module_called_twice():
    net = T.integerize(T.TVBlock().eval())
    g = from_torch(net)             # raised "duplicate node name" before
    names = g.layer_names()
    assert {"block1_relu", "block1_relu_1", "block1_relu_2"} <= set(names)
    x = T.int_input(TV_SHAPE)
    with torch.no_grad():
        assert torch.equal(g.forward(x), net(x))


def test_from_torch_keeps_the_names_of_modules_called_once():
    class Net(nn.Module):           # the net of test_defer_arbitrary_torch_model
        def __init__(self):
            super().__init__()
            self.c1 = nn.Conv2d(3, 8, 3, padding=1)
            self.c2 = nn.Conv2d(8, 8, 3, padding=1)
            self.c3 = nn.Conv2d(8, 8, 3, padding=1)
            self.head = nn.Linear(8, 5)

        def forward(self, x):
            a = torch.relu(self.c1(x))
            b = torch.relu(self.c2(a))
            c = torch.relu(self.c3(b) + b)
            return self.head(c.mean(dim=(2, 3)))

    assert from_torch(Net().eval()).layer_names() == [
        "c1", "relu", "c2", "relu_1", "c3", "add", "relu_2", "mean", "head"]

    class Seq(nn.Module):
        def __init__(self):
            super().__init__()
            self.body = nn.Sequential(nn.Conv2d(3, 4, 1), nn.ReLU())

        def forward(self, x):
            return self.body(x)

    assert from_torch(Seq().eval()).layer_names() == ["body_0", "body_1"]


# --------------------------------------------------------- 7. partitioning
def _run_defer(model, cuts, nodes, items, cfg):
    eng = DEFER(nodes, config=cfg)
    in_q, out_q = queue.Queue(10), queue.Queue(10)
    t = threading.Thread(target=eng.run_defer,
                         args=(model, cuts, in_q, out_q))
    t.start()
    for x in items:
        in_q.put(x)
    in_q.put(None)
    outs = [out_q.get(timeout=120) for _ in items]
    t.join(timeout=120)
    assert not t.is_alive()
    return outs


def test_every_valid_cut_gives_the_whole_models_output():
    net = T.integerize(T.TVBlock().eval())
    g = lower_torch(net, TV_SHAPE)
    cuts = g.valid_cut_points()
    assert cuts and "block1_relu_2" in cuts and "maxpool" in cuts
    x = T.int_input(TV_SHAPE)
    gen = torch.Generator().manual_seed(5)
    xr = torch.randn(*TV_SHAPE, generator=gen)
    with torch.no_grad():
        for inp in (x, xr):
            want = g.forward(inp)
            for c in cuts:
                a, b = g.split([c])
                assert torch.equal(b.forward(a.forward(inp)), want), c


def test_run_defer_with_lower_on():
    torch.manual_seed(3)
    net = T.randomize_bn(T.TVBlock().eval(), torch.Generator().manual_seed(3))
    xs = [torch.randn(1, 3, 32, 32) for _ in range(2)]
    cfg = PipelineConfig(lower=True, device="cpu", dtype="fp32",
                         input_shape=(1, 3, 32, 32))
    with torch.no_grad():
        whole = lower_torch(net, (1, 3, 32, 32))
        want = [whole.forward(x) for x in xs]
    outs = _run_defer(net, None, ["cpu", "cpu"], xs, cfg)
    for o, w in zip(outs, want):
        assert torch.equal(o, w)
    outs = _run_defer(net, ["block1_relu_2"], ["cpu", "cpu"], xs, cfg)
    for o, w in zip(outs, want):
        assert torch.equal(o, w)


def test_lower_flag_is_off_by_default_and_validated():
    net = T.TVBlock().eval()
    assert PipelineConfig().lower is False
    for gm in (as_graph_model(net), as_graph_model(net, PipelineConfig())):
        assert any(isinstance(m, nn.Conv2d) for m in gm.modules())
        assert not any(isinstance(m, L.ConvBNAct) for m in gm.modules())
    gm = as_graph_model(net, PipelineConfig(lower=True,
                                            input_shape=TV_SHAPE))
    assert not any(isinstance(m, nn.Conv2d) for m in gm.modules())
    assert gm.model_name == "TVBlock"
    with pytest.raises(ValueError, match="lower"):
        PipelineConfig(lower=1)
    with pytest.raises(ValueError, match="input_shape"):
        PipelineConfig(lower=True)


# ------------------------------------------------------ 8. ops on the CPU
_DT = (torch.float32, torch.bfloat16)


@pytest.mark.parametrize("src", _DT)
@pytest.mark.parametrize("dst", _DT + (None,))
def test_layout_ops_equal_the_permute_formulation(src, dst):
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 5, 3, 7, generator=gen).to(src)
    want_dt = src if dst is None else dst
    y = ops.to_nhwc(x, dst)
    assert y.dtype == want_dt and y.shape == (2, 3, 7, 5)
    assert y.is_contiguous()
    assert torch.equal(y, x.permute(0, 2, 3, 1).contiguous().to(want_dt))
    z = ops.to_nchw(y, dst)
    assert z.dtype == want_dt and z.shape == x.shape and z.is_contiguous()
    assert torch.equal(z, y.permute(0, 3, 1, 2).contiguous().to(want_dt))
    # inverse of each other (through bf16 the value is rounded once)
    assert torch.equal(z, x.to(want_dt))
    assert y.data_ptr() != x.data_ptr()         # fresh, never a view


def test_layout_ops_reject_what_the_other_ops_reject():
    x = torch.randn(2, 4, 3, 3)
    for op in (ops.to_nhwc, ops.to_nchw):
        with pytest.raises(RuntimeError, match="contiguous"):
            op(x.permute(0, 2, 3, 1))
        with pytest.raises(RuntimeError, match="bf16 or fp32"):
            op(x.half())
        with pytest.raises(RuntimeError, match="bf16 or fp32"):
            op(x, torch.float16)
        with pytest.raises(RuntimeError, match="4-D"):
            op(x[0])
        big = torch.empty(1, 2, 2 ** 15, 2 ** 15, dtype=torch.bfloat16,
                          device="meta")
        with pytest.raises(RuntimeError, match="2\\^31"):
            op(big)
