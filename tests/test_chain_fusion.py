"""fuse_expand_reduce: the add_k -> res*_conv1 graph rewrite (CPU)."""

import torch

from defer_amd.graph import GraphModel, GraphNode, LayerGraph
from defer_amd.models import DEFER_8STAGE_CUTS, resnet50, resnet101
from defer_amd.models.layers import AddAct, ConvBNAct
from defer_amd.parallel.fusion import (ChainedExpandReduce,
                                       fuse_expand_reduce,
                                       fuse_residual_adds)


def _pairs(graph):
    return [n for n in graph.nodes
            if isinstance(n.layer, ChainedExpandReduce)]


def _fuse(graph):
    return fuse_expand_reduce(fuse_residual_adds(graph))


def test_pair_counts_whole_models():
    assert len(_pairs(_fuse(resnet50().graph))) == 15
    assert len(_pairs(_fuse(resnet101().graph))) == 32


def test_pair_count_per_stage_at_defer_cuts():
    stages = resnet50().graph.split(DEFER_8STAGE_CUTS)
    assert len(stages) == 8
    fused = [_fuse(s) for s in stages]
    # a pair whose conv1 lives in the next stage stays unfused
    assert sum(len(_pairs(g)) for g in fused) == 8
    for s, g in zip(stages, fused):
        assert g.output == s.output
        assert g.output in g.by_name


def test_names_survive():
    g0 = resnet50().graph
    g = _fuse(g0)
    names = set(g.layer_names())
    for n in g0.layer_names():
        if n.startswith("add_") or n.endswith("_conv1"):
            assert n in names, n


def test_modules_are_shared_not_copied():
    m = resnet50()
    g = _fuse(m.graph)
    for n in _pairs(g):
        add_name = n.name[:-len("__chain")]
        picks = [c for c in g.nodes if c.inputs == [n.name]]
        assert [c.name for c in picks][0] == add_name
        conv1 = m.graph.by_name[picks[1].name].layer
        assert n.layer.reduce is conv1
        conv3 = [x for x in m.graph.nodes
                 if x.layer is n.layer.expand.conv]
        assert len(conv3) == 1 and conv3[0].name.endswith("_conv3")
    # the unfused graph is still valid and unchanged
    assert sum(isinstance(x.layer, AddAct) for x in m.graph.nodes) == 16


def test_forward_matches_unfused():
    m = resnet50()
    x = torch.randn(1, 64, 64, 3)
    with torch.no_grad():
        want = m(x)
        got = GraphModel(_fuse(m.graph))(x)
    assert torch.allclose(got, want, atol=1e-5)


def test_forward_matches_through_stage_executor():
    from defer_amd.parallel.pipeline import StageExecutor

    m = resnet50()
    x = torch.randn(1, 64, 64, 3)
    with torch.no_grad():
        want = m(x)
    ex = StageExecutor(GraphModel(m.graph), "cpu", torch.float32)
    assert len(_pairs(ex.model.graph)) == 15
    with torch.no_grad():
        got = ex.run(x)
    assert torch.allclose(got, want, atol=1e-5)
    off = StageExecutor(GraphModel(m.graph), "cpu", torch.float32,
                        chain=False)
    assert len(_pairs(off.model.graph)) == 0


def _block(consumer, consumer_inputs=None, with_consumer=True):
    """x -> a(1x1) -> c3(1x1, none) -> add(c3, x) [-> consumer]."""
    nodes = [
        GraphNode("a", ConvBNAct(16, 8, 1, 1, 0, "relu"), ["input"]),
        GraphNode("c3", ConvBNAct(8, 16, 1, 1, 0, "none"), ["a"]),
        GraphNode("add_1", AddAct("relu"), ["c3", "input"]),
    ]
    if with_consumer:
        nodes.append(GraphNode("nxt", consumer,
                               consumer_inputs or ["add_1"]))
    return LayerGraph(nodes)


def test_matching_toy_block_fuses_and_agrees():
    g0 = _block(ConvBNAct(16, 8, 1, 1, 0, "relu"))
    g = _fuse(g0)
    assert len(_pairs(g)) == 1
    x = torch.randn(2, 5, 5, 16)
    with torch.no_grad():
        assert torch.allclose(g.forward(x), g0.forward(x), atol=1e-5)


def test_non_matches_left_alone():
    cases = {
        "3x3 consumer": _block(ConvBNAct(16, 8, 3, 1, 1, "relu")),
        "stride-2 consumer": _block(ConvBNAct(16, 8, 1, 2, 0, "relu")),
        "add_k is the stage output": _block(None, with_consumer=False),
    }
    # a consumer that takes a residual: FusedConvAddAct after the first
    # pass, i.e. a conv with two inputs
    nodes = _block(None, with_consumer=False).nodes + [
        GraphNode("c", ConvBNAct(16, 16, 1, 1, 0, "none"), ["add_1"]),
        GraphNode("add_2", AddAct("relu"), ["c", "add_1"]),
    ]
    cases["consumer takes a residual"] = LayerGraph(nodes)
    x = torch.randn(1, 6, 6, 16)
    for why, g0 in cases.items():
        g1 = fuse_residual_adds(g0)
        g2 = fuse_expand_reduce(g1)
        assert len(_pairs(g2)) == 0, why
        assert g2.layer_names() == g1.layer_names(), why
        with torch.no_grad():
            assert torch.equal(g2.forward(x), g1.forward(x)), why
