"""GPU: the grouped 3x3 conv kernels (csrc/gconv.hip), a lowered ResNeXt-style
torch module and resnext50_32x4d().

No tolerance here is measured. Exact-integer data must be torch.equal to the
CPU reference in both dtypes (which is also the test for leakage between the
groups of a 16-channel slab and for the zero tap slot); random bf16 data uses
the project's conv tolerance (0.005 of the largest output); random fp32 data
the forward error bound of a length-9*Cg fmaf chain plus the epilogue,
(9*Cg + 4) * 2^-24 * (|scale| * sum|x*w| + |bias|), the form of
test_ops_fp32_gpu.py."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from defer_amd import ops
from defer_amd.graph import GraphModel, LayerGraph
from defer_amd.lower import lower_torch
from defer_amd.models import resnext50_32x4d
from defer_amd.ops import reference as ref
from defer_amd.parallel.pipeline import StageExecutor

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
DTYPES = (torch.float32, torch.bfloat16)
ACTS = ("none", "relu", "relu6", "hardswish")
CGS = (4, 8, 16, 32)
GEOMS = [(1, 1), (2, 1), (1, 0), (2, 0)]            # (stride, pad)


def _inputs(shape, cg, seed, ints):
    """x, w [C, 3, 3, cg], scale, bias. ints: x and w in {-1, 0, 1}, scale
    in {1, 2}, bias in 0..2, so every partial sum is a small integer."""
    g = torch.Generator().manual_seed(seed)
    c = shape[-1]
    if ints:
        x = torch.randint(-1, 2, shape, generator=g).float()
        w = torch.randint(-1, 2, (c, 3, 3, cg), generator=g).float()
        scale = torch.randint(1, 3, (c,), generator=g).float()
        bias = torch.randint(0, 3, (c,), generator=g).float()
    else:
        x = torch.randn(shape, generator=g)
        w = torch.randn(c, 3, 3, cg, generator=g) / (3 * cg ** 0.5)
        scale = torch.rand(c, generator=g) + 0.5
        bias = torch.randn(c, generator=g) * 0.1
    return x, w, scale, bias


def _shapes(cg, stride, pad):
    """(N, H, W, C) with C a multiple of max(16, cg). The kernel's tile is
    8 x 16 outputs at stride 1 and 3 x 16 at stride 2, a workgroup holds 64
    channels and the grid is capped at 512 workgroups."""
    c1 = max(16, cg)
    th = 8 if stride == 1 else 3

    def size(out):                  # the input size that gives `out` outputs
        return (out - 1) * stride + 3 - 2 * pad

    return [
        (1, 3, 3, c1) if pad == 0 else (1, 1, 1, c1),       # one output
        (2, 7, 9, 96 if cg == 32 else 48),  # under a tile, odd, 3/4 block
        (1, size(th + 1), size(17), 160),   # a row and a column past a tile
        (8, 1552, 3, c1),           # > 3 x 512 tiles: the grid-stride loop
    ]


@pytest.mark.parametrize("stride,pad", GEOMS,
                         ids=[f"s{s}p{p}" for s, p in GEOMS])
@pytest.mark.parametrize("cg", CGS)
@pytest.mark.parametrize("case", range(4),
                         ids=["pixel", "small", "past_tile", "grid_stride"])
def test_gconv_exact_integers(case, cg, stride, pad):
    shape = _shapes(cg, stride, pad)[case]
    x, w, scale, bias = _inputs(shape, cg, 7 + case, ints=True)
    for act in ACTS:
        for dt in DTYPES:
            # the reference rounds its fp32 result once to the dtype of x
            want = ref.gconv2d_bn_act(x.to(dt), w.to(dt), scale, bias, stride,
                                      pad, act)
            assert want.abs().max() <= 256      # every sum is exact in bf16
            got = ops.gconv2d_bn_act(
                x.to(DEV, dt), w.to(DEV, dt), scale.to(DEV), bias.to(DEV),
                stride, pad, act)
            assert got.dtype == dt and got.shape == want.shape
            assert torch.equal(got.cpu(), want), (act, dt)


FLOAT_SHAPES = [(2, 13, 21, 64), (1, 28, 28, 96), (3, 9, 40, 160)]


@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("cg", CGS)
@pytest.mark.parametrize("shape", FLOAT_SHAPES,
                         ids=["x".join(map(str, s)) for s in FLOAT_SHAPES])
def test_gconv_random_floats(shape, cg, stride):
    x, w, scale, bias = _inputs(shape, cg, 11, ints=False)
    dev = [t.to(DEV) for t in (scale, bias)]
    xb, wb = x.bfloat16(), w.bfloat16()
    want = ref.gconv2d_bn_act(xb.float(), wb.float(), scale, bias, stride, 1,
                              "relu")
    got = ops.gconv2d_bn_act(xb.to(DEV), wb.to(DEV), *dev, stride, 1, "relu")
    err = ((got.float().cpu() - want).abs().max() / want.abs().max()).item()
    print(f"bf16 rel err {err:.5f}")
    assert err < 0.005

    def conv64(a, b):
        y = F.conv2d(a.double().permute(0, 3, 1, 2),
                     b.double().permute(0, 3, 1, 2), stride=stride,
                     padding=1, groups=shape[-1] // cg)
        return y.permute(0, 2, 3, 1)

    want64 = conv64(x, w) * scale.double() + bias.double()
    bound = (9 * cg + 4) * U * (conv64(x.abs(), w.abs()) * scale.double()
                                + bias.double().abs())
    got = ops.gconv2d_bn_act(x.to(DEV), w.to(DEV), *dev, stride, 1, "none")
    excess = ((got.double().cpu() - want64).abs() / bound).max().item()
    print(f"fp32 error / bound {excess:.3f}")
    assert excess <= 1.0


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
def test_gconv_is_deterministic_and_graph_capturable(dt):
    x, w, scale, bias = _inputs((4, 37, 50, 96), 8, 3, ints=False)
    args = (x.to(DEV, dt), w.to(DEV, dt), scale.to(DEV), bias.to(DEV), 2, 1,
            "hardswish")
    eager = ops.gconv2d_bn_act(*args)
    assert torch.equal(ops.gconv2d_bn_act(*args), eager)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.gconv2d_bn_act(*args)
    for _ in range(3):
        out.fill_(7)
        graph.replay()
        assert torch.equal(out, eager)


REFUSED = [
    ("Cg = 2", dict(cg=2), "got 2"),
    ("Cg = 12", dict(c=48, cg=12), "got 12"),
    ("C % 16", dict(c=24, cg=8), "C = 24"),
    ("5x5", dict(k=5), "5x5"),
    ("stride 3", dict(stride=3), "got 3"),
    ("pad 2", dict(pad=2), "got 2"),
    ("fp16", dict(dt=torch.float16), "float16"),
    ("CPU scale", dict(scale_dev="cpu"), "scale"),
]


@pytest.mark.parametrize("name,kw,match", REFUSED,
                         ids=[r[0] for r in REFUSED])
def test_gconv_refuses_what_the_kernels_do_not_serve(name, kw, match):
    c, cg, k = kw.get("c", 32), kw.get("cg", 8), kw.get("k", 3)
    dt = kw.get("dt", torch.bfloat16)
    x = torch.zeros(1, 8, 8, c, device=DEV, dtype=dt)
    w = torch.zeros(c, k, k, cg, device=DEV, dtype=dt)
    scale = torch.ones(c, device=kw.get("scale_dev", DEV))
    with pytest.raises((ValueError, RuntimeError), match=match):
        ops.gconv2d_bn_act(x, w, scale, None, kw.get("stride", 1),
                           kw.get("pad", 1), "relu")


class SmallResNeXt(nn.Module):
    """Three bottlenecks with a grouped conv2 of 32, 64 and 128 channels in
    8 groups (4, 8 and 16 channels each), the second and third at stride 2,
    written the way torchvision writes them; returns logits."""

    def __init__(self):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, 32, 3, padding=1, bias=False),
                                  nn.BatchNorm2d(32), nn.ReLU(inplace=True))
        blocks, cin = [], 32
        for width, stride in ((32, 1), (64, 2), (128, 2)):
            blocks.append(nn.Sequential(
                nn.Conv2d(cin, width, 1, bias=False), nn.BatchNorm2d(width),
                nn.ReLU(inplace=True),
                nn.Conv2d(width, width, 3, stride, 1, groups=8, bias=False),
                nn.BatchNorm2d(width), nn.ReLU(inplace=True),
                nn.Conv2d(width, width, 1, bias=False),
                nn.BatchNorm2d(width)))
            cin = width
        self.blocks = nn.ModuleList(blocks)
        self.proj = nn.ModuleList([nn.Conv2d(32, 64, 1, 2),
                                   nn.Conv2d(64, 128, 1, 2)])
        self.fc = nn.Linear(128, 16)

    def forward(self, x):
        x = self.stem(x)
        x = torch.relu(self.blocks[0](x) + x)
        x = torch.relu(self.blocks[1](x) + self.proj[0](x))
        x = torch.relu(self.blocks[2](x) + self.proj[1](x))
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
def test_lowered_resnext_module(dt):
    torch.manual_seed(5)
    net = SmallResNeXt().eval()
    for m in net.modules():             # BN statistics that are not 0 / 1
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    shape = (4, 3, 30, 30)
    x = torch.randn(*shape)
    with torch.no_grad():
        want = net(x)
    g = lower_torch(net, shape, strict=True)
    kinds = [type(n.layer).__name__ for n in g.nodes]
    assert kinds.count("GroupedConvBNAct") == 3
    got = StageExecutor(GraphModel(g), DEV, dt).run(x.to(DEV, dt))
    got = got.float().cpu()
    if dt == torch.float32:
        assert torch.allclose(got.softmax(-1), want.softmax(-1), atol=1e-6)
    else:
        cos = F.cosine_similarity(got, want, dim=-1)
        print(f"logits cosine {cos}")
        assert (cos > 0.98).all(), f"cosine {cos}"


def test_resnext50_bf16_against_its_cpu_forward():
    torch.manual_seed(0)
    model = resnext50_32x4d()
    nodes = [n for n in model.graph.nodes if n.name != "softmax"]
    logits = GraphModel(LayerGraph(nodes, output="fc1000"))
    x = torch.randn(2, 224, 224, 3).bfloat16()
    with torch.no_grad():
        want = logits(x.float())
    got = StageExecutor(logits, DEV, torch.bfloat16).run(x.to(DEV))
    cos = F.cosine_similarity(got.float().cpu(), want, dim=-1)
    print(f"logits cosine {cos}")
    assert (cos > 0.98).all(), f"cosine {cos}"
