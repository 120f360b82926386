"""fuse_conv_pool: the conv1 -> pool1 graph rewrite (CPU)."""

import torch

from defer_amd.graph import GraphModel
from defer_amd.models import densenet121, resnet50, resnet101, vgg19
from defer_amd.models.layers import ConvBNAct, MaxPool
from defer_amd.parallel.fusion import (ChainedExpandReduce, FusedConvPool,
                                       fuse_conv_pool, fuse_expand_reduce,
                                       fuse_residual_adds)


def _fused(graph):
    return [n for n in graph.nodes if isinstance(n.layer, FusedConvPool)]


def test_one_fused_node_per_7x7_stem():
    for make in (resnet50, resnet101, densenet121):
        g = fuse_conv_pool(make().graph)
        assert [n.name for n in _fused(g)] == ["pool1"], make.__name__
        assert "conv1" not in g.by_name
        assert g.by_name["pool1"].inputs == ["input"]


def test_vgg_pairs_are_left_unmatched():
    # 3x3 conv -> 2x2/p0 pool: not the fused kernel's class, so the pass
    # leaves the graph exactly as it was
    g0 = vgg19().graph
    g = fuse_conv_pool(g0)
    assert _fused(g) == []
    assert g.layer_names() == g0.layer_names()


def test_pool1_survives_as_a_cut_name():
    g0 = resnet50().graph
    g = fuse_conv_pool(g0)
    assert "pool1" in g.valid_cut_points()
    want = [n for n in g0.layer_names() if n != "conv1"]
    assert g.layer_names() == want
    assert g.output == g0.output


def test_modules_are_shared_not_copied():
    m = resnet50()
    g = fuse_conv_pool(m.graph)
    (n,) = _fused(g)
    assert n.layer.conv is m.graph.by_name["conv1"].layer
    assert n.layer.pool is m.graph.by_name["pool1"].layer
    # the unfused graph is still valid and unchanged
    assert isinstance(m.graph.by_name["conv1"].layer, ConvBNAct)
    assert isinstance(m.graph.by_name["pool1"].layer, MaxPool)


def test_forward_matches_unfused():
    for make in (resnet50, densenet121):
        m = make()
        x = torch.randn(1, 64, 64, 3)
        with torch.no_grad():
            want = m(x)
            got = GraphModel(fuse_conv_pool(m.graph))(x)
        assert torch.allclose(got, want, atol=1e-5), make.__name__


def test_forward_matches_through_stage_executor():
    from defer_amd.parallel.pipeline import StageExecutor

    m = resnet50()
    x = torch.randn(1, 64, 64, 3)
    with torch.no_grad():
        want = m(x)
    ex = StageExecutor(GraphModel(m.graph), "cpu", torch.float32)
    assert len(_fused(ex.model.graph)) == 1
    with torch.no_grad():
        got = ex.run(x)
    assert torch.allclose(got, want, atol=1e-5)
    off = StageExecutor(GraphModel(m.graph), "cpu", torch.float32,
                        fuse=False)
    assert len(_fused(off.model.graph)) == 0


def test_stage_cut_at_conv1_is_left_unfused():
    from defer_amd.parallel.pipeline import StageExecutor

    m = resnet50()
    stages = m.graph.split(["conv1"])
    fused = [fuse_conv_pool(s) for s in stages]
    assert all(_fused(g) == [] for g in fused)
    for s, g in zip(stages, fused):
        assert g.layer_names() == s.layer_names()
        assert g.output == s.output
    x = torch.randn(1, 64, 64, 3)
    with torch.no_grad():
        want = m(x)
        h = x
        for s in stages:
            h = StageExecutor(GraphModel(s), "cpu", torch.float32).run(h)
    assert torch.allclose(h, want, atol=1e-5)


def test_composes_with_the_other_passes():
    m = resnet50()
    g = fuse_conv_pool(fuse_expand_reduce(fuse_residual_adds(m.graph)))
    assert len(_fused(g)) == 1
    assert sum(isinstance(n.layer, ChainedExpandReduce)
               for n in g.nodes) == 15
    # order does not matter: pool1 is not part of any chained pair
    g2 = fuse_expand_reduce(fuse_residual_adds(fuse_conv_pool(m.graph)))
    assert g2.layer_names() == g.layer_names()
    x = torch.randn(1, 64, 64, 3)
    with torch.no_grad():
        assert torch.allclose(g.forward(x), m(x), atol=1e-5)
