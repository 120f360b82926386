"""fuse_chain_projection: folding the res2_0 projection shortcut into its
chained add_k -> conv1 node (CPU)."""

import pytest
import torch

from defer_amd.graph import GraphModel, GraphNode, LayerGraph
from defer_amd.models import (DEFER_8STAGE_CUTS, resnet50, resnet101,
                              resnet152)
from defer_amd.models.layers import AddAct, ConvBNAct
from defer_amd.parallel.fusion import (ChainedExpandReduce,
                                       ChainedExpandReduceProj,
                                       fuse_chain_projection,
                                       fuse_expand_reduce,
                                       fuse_residual_adds)


def _chain(graph):
    return fuse_expand_reduce(fuse_residual_adds(graph))


def _projs(graph):
    return [n for n in graph.nodes
            if isinstance(n.layer, ChainedExpandReduceProj)]


@pytest.mark.parametrize("make", [resnet50, resnet101, resnet152])
def test_one_node_rewritten_per_model(make):
    g1 = _chain(make().graph)
    g2 = fuse_chain_projection(g1)
    (n,) = _projs(g2)
    assert n.name == "add_1__chain"
    assert n.inputs == ["res2_0_conv2", "pool1"]
    assert "res2_0_proj" not in g2.by_name
    # everything else is the graph it was
    assert len(g2.nodes) == len(g1.nodes) - 1
    kept = [m for m in g1.nodes if m.name != "res2_0_proj"]
    for a, b in zip(kept, g2.nodes):
        assert a.name == b.name
        if b is not n:
            assert a.layer is b.layer and a.inputs == b.inputs
    # the stride-2 projections of the later stages stay nodes of their own
    for p in ("res3_0_proj", "res4_0_proj", "res5_0_proj"):
        assert isinstance(g2.by_name[p].layer, ConvBNAct)


def test_names_survive():
    g0 = resnet50().graph
    g = fuse_chain_projection(_chain(g0))
    names = set(g.layer_names())
    for n in g0.layer_names():
        if n.startswith("add_") or n.endswith("_conv1"):
            assert n in names, n
    assert g.output == g0.output


def test_modules_are_shared_not_copied():
    m = resnet50()
    g1 = _chain(m.graph)
    before = g1.by_name["add_1__chain"].layer
    (n,) = _projs(fuse_chain_projection(g1))
    assert n.layer.proj is m.graph.by_name["res2_0_proj"].layer
    assert n.layer.expand is before.expand
    assert n.layer.expand.conv is m.graph.by_name["res2_0_conv3"].layer
    assert n.layer.reduce is m.graph.by_name["res2_1_conv1"].layer
    picks = [c.name for c in fuse_chain_projection(g1).nodes
             if c.inputs == [n.name]]
    assert picks == ["add_1", "res2_1_conv1"]
    # the unfused graph is still valid and unchanged
    assert "res2_0_proj" in m.graph.by_name
    assert sum(isinstance(x.layer, AddAct) for x in m.graph.nodes) == 16


def test_forward_matches_unfused():
    m = resnet50()
    x = torch.randn(1, 64, 64, 3)
    with torch.no_grad():
        want = m(x)
        got = GraphModel(fuse_chain_projection(_chain(m.graph)))(x)
    assert torch.allclose(got, want, atol=1e-5)


def test_stage_executor_applies_the_pass():
    from defer_amd.parallel.pipeline import StageExecutor

    m = resnet50()
    x = torch.randn(1, 64, 64, 3)
    with torch.no_grad():
        want = m(x)
    ex = StageExecutor(GraphModel(m.graph), "cpu", torch.float32)
    assert len(_projs(ex.model.graph)) == 1
    with torch.no_grad():
        got = ex.run(x)
    assert torch.allclose(got, want, atol=1e-5)
    off = StageExecutor(GraphModel(m.graph), "cpu", torch.float32,
                        chain=False)
    assert len(_projs(off.model.graph)) == 0
    assert "res2_0_proj" in off.model.graph.by_name


def test_defer_cuts_outputs_unchanged():
    m = resnet50()
    stages = m.graph.split(DEFER_8STAGE_CUTS)
    assert len(stages) == 8
    fused = [fuse_chain_projection(_chain(s)) for s in stages]
    # res2_0 lies wholly inside the first stage (the first cut is add_2)
    assert [len(_projs(g)) for g in fused] == [1, 0, 0, 0, 0, 0, 0, 0]
    x = torch.randn(1, 64, 64, 3)
    with torch.no_grad():
        want = m(x)
        y = x
        for s, g in zip(stages, fused):
            assert g.output == s.output and g.output in g.by_name
            y = g.forward(y)
    assert torch.allclose(y, want, atol=1e-5)


def _block(proj, proj_inputs=None, chained=True, extra=(), output=None):
    """x -> a(1x1) -> c3(1x1, none); add_1 = relu(c3 + proj(x)); then the
    next block's conv1 when chained."""
    nodes = [
        GraphNode("a", ConvBNAct(16, 8, 1, 1, 0, "relu"), ["input"]),
        GraphNode("c3", ConvBNAct(8, 32, 1, 1, 0, "none"), ["a"]),
        GraphNode("proj", proj, proj_inputs or ["input"]),
        GraphNode("add_1", AddAct("relu"), ["c3", "proj"]),
    ]
    if chained:
        nodes.append(GraphNode("nxt", ConvBNAct(32, 8, 1, 1, 0, "relu"),
                               ["add_1"]))
    nodes.extend(extra)
    return LayerGraph(nodes, output=output)


def test_matching_toy_block_folds_and_agrees():
    g0 = _block(ConvBNAct(16, 32, 1, 1, 0, "none"))
    g = fuse_chain_projection(_chain(g0))
    (n,) = _projs(g)
    assert n.inputs == ["a", "input"]
    assert "proj" not in g.by_name
    x = torch.randn(2, 5, 5, 16)
    with torch.no_grad():
        assert torch.allclose(g.forward(x), g0.forward(x), atol=1e-5)


def test_non_matches_left_alone():
    s2 = [
        GraphNode("a", ConvBNAct(16, 8, 1, 2, 0, "relu"), ["input"]),
        GraphNode("c3", ConvBNAct(8, 32, 1, 1, 0, "none"), ["a"]),
        GraphNode("proj", ConvBNAct(16, 32, 1, 2, 0, "none"), ["input"]),
        GraphNode("add_1", AddAct("relu"), ["c3", "proj"]),
        GraphNode("nxt", ConvBNAct(32, 8, 1, 1, 0, "relu"), ["add_1"]),
    ]
    second = [
        GraphNode("side", ConvBNAct(32, 8, 1, 1, 0, "relu"), ["proj"]),
        GraphNode("out", AddAct("relu"), ["nxt", "side"]),
    ]
    cases = {
        "stride-2 proj": LayerGraph(s2),
        "3x3 proj": _block(ConvBNAct(16, 32, 3, 1, 1, "none")),
        "proj with an activation": _block(ConvBNAct(16, 32, 1, 1, 0,
                                                    "relu")),
        "proj with a second consumer": _block(
            ConvBNAct(16, 32, 1, 1, 0, "none"), extra=second),
        "unchained add": _block(ConvBNAct(16, 32, 1, 1, 0, "none"),
                                chained=False),
    }
    x = torch.randn(1, 6, 6, 16)
    for why, g0 in cases.items():
        g1 = _chain(g0)
        g2 = fuse_chain_projection(g1)
        assert len(_projs(g2)) == 0, why
        assert g2.layer_names() == g1.layer_names(), why
        assert "proj" in g2.by_name, why
        with torch.no_grad():
            assert torch.equal(g2.forward(x), g1.forward(x)), why
    # the chained cases did chain: the pass, not the matcher before it,
    # declined them
    for why in ("stride-2 proj", "3x3 proj", "proj with an activation",
                "proj with a second consumer"):
        assert any(type(n.layer) is ChainedExpandReduce
                   for n in _chain(cases[why]).nodes), why


def test_proj_that_is_the_stage_output_left_alone():
    # the stage hands the projection itself on (a cut placed on it)
    g0 = _block(ConvBNAct(16, 32, 1, 1, 0, "none"), output="proj")
    g1 = _chain(g0)
    g2 = fuse_chain_projection(g1)
    assert len(_projs(g2)) == 0
    assert g2.layer_names() == g1.layer_names()
    x = torch.randn(1, 6, 6, 16)
    with torch.no_grad():
        assert torch.equal(g2.forward(x), g1.forward(x))
