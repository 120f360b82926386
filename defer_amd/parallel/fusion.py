"""Stage-graph fusion passes (applied by StageExecutor at load time).

The HIP conv kernel epilogue supports a fused residual add + activation
(conv.hip: HAS_RES template arg), so the pattern

    c = ConvBNAct(act="none")(x);  y = AddAct(act)(c, skip)

collapses into one kernel launch: y = conv(x, residual=skip, act=act).
This removes one full read+write round trip of the conv output per
residual block (16 blocks in ResNet50 — ~9% of forward time unfused).

A second pass, fuse_expand_reduce, chains that fused node with the next
block's 1x1 conv1 (ops.conv1x1_chain): add_k is the widest tensor of the
block and conv1 reads it straight back, so one kernel computes both and
add_k is never re-read.

fuse_chain_projection then folds a 1x1/s1 projection shortcut (res2_0_proj
of the ResNets) into that chained node (ops.conv1x1_chain_proj): the kernel
makes the shortcut from the block input per tile, and the projection's
output, as wide as add_k, is neither written nor read.

A third pass, fuse_conv_pool, merges a conv whose only consumer is a
max-pool into one node (ops.conv_bn_act_maxpool): for the 7x7/s2 stem of
the ResNets and DenseNet121 the HIP kernel then writes only the pooled
tensor, a quarter of the conv activation it would otherwise write and
read back.

Cut-point names are preserved: the fused node takes the AddAct node's
(for fuse_conv_pool: the pool's) name, so partition boundaries at `add_N`
(test/test.py:18) and `pool1` still resolve. Fusion happens per stage
AFTER partitioning.
"""

from typing import List

import torch.nn as nn

from defer_amd.graph import GraphNode, LayerGraph
from defer_amd.models.layers import AddAct, ConvBNAct, MaxPool


class FusedConvAddAct(nn.Module):
    """conv(x) + residual, activation applied after the add (the conv
    module itself is left untouched so the unfused graph stays valid)."""

    def __init__(self, conv: ConvBNAct, act: str):
        super().__init__()
        self.conv = conv
        self.act = act

    def forward(self, x, residual):
        from defer_amd import ops

        c = self.conv
        return ops.conv2d_bn_act(
            x, c.weight.to(x.dtype), c.scale, c.bias, stride=c.stride,
            padding=c.padding, act=self.act, residual=residual)


def fuse_residual_adds(graph: LayerGraph) -> LayerGraph:
    """Rewrite conv(act=none) -> AddAct pairs into FusedConvAddAct."""
    consumers = {}
    for n in graph.nodes:
        for p in n.inputs:
            consumers.setdefault(p, []).append(n.name)
    out_name = graph.output

    nodes: List[GraphNode] = []
    by_name = {n.name: n for n in graph.nodes}
    fused_away = set()
    for n in graph.nodes:
        if n.name in fused_away:
            continue
        lay = n.layer
        if isinstance(lay, AddAct):
            # find a conv parent eligible for fusion
            for idx, p in enumerate(n.inputs):
                pn = by_name.get(p)
                if (pn is not None and isinstance(pn.layer, ConvBNAct)
                        and pn.layer.act == "none"
                        and consumers.get(p, []) == [n.name]
                        and p != out_name):
                    other = n.inputs[1 - idx]
                    fused = FusedConvAddAct(pn.layer, lay.act)
                    # replace: drop conv node, AddAct node becomes fused
                    nodes = [m for m in nodes if m.name != p]
                    nodes.append(GraphNode(n.name, fused,
                                           [pn.inputs[0], other]))
                    fused_away.add(p)
                    break
            else:
                nodes.append(n)
            continue
        nodes.append(n)
    return LayerGraph(nodes, output=graph.output)


class ChainedExpandReduce(nn.Module):
    """add_k = act(conv3(x) + skip) and the next block's conv1(add_k) in
    one call; returns the (add_k, conv1) tuple. The original modules stay
    referenced (not copied), so parameters are shared with the unfused
    graph."""

    def __init__(self, expand: FusedConvAddAct, reduce: ConvBNAct):
        super().__init__()
        self.expand = expand
        self.reduce = reduce

    def forward(self, x, residual):
        from defer_amd import ops

        c3, c1 = self.expand.conv, self.reduce
        return ops.conv1x1_chain(
            x, c3.weight.to(x.dtype), c3.scale, c3.bias, residual,
            self.expand.act, c1.weight.to(x.dtype), c1.scale, c1.bias,
            c1.act)


class _Pick(nn.Module):
    """Select one item of a tuple-valued node (nodes carry one value)."""

    def __init__(self, index: int):
        super().__init__()
        self.index = index

    def forward(self, t):
        return t[self.index]

    def extra_repr(self):
        return f"item {self.index}"


def _is_pointwise(c: ConvBNAct) -> bool:
    return c.kernel == 1 and c.stride == 1 and c.padding == 0


# The chain, projection and stem-pool kernels apply ReLU or nothing. A conv
# with another activation (MobileNetV2's ReLU6) stays out of those passes;
# fuse_residual_adds takes any, since it goes through conv2d_bn_act.
_CHAIN_ACTS = ("relu", "none")


def fuse_expand_reduce(graph: LayerGraph) -> LayerGraph:
    """Rewrite FusedConvAddAct(1x1) -> ConvBNAct(1x1, single input) pairs
    into one ChainedExpandReduce node plus two picks that keep the
    original node names. add_k may have other consumers and may be the
    graph output; a conv1 outside this graph is simply not matched."""
    consumers = {}
    for n in graph.nodes:
        for p in n.inputs:
            consumers.setdefault(p, []).append(n)

    partner = {}                       # add_k name -> conv1 node
    for n in graph.nodes:
        if not (isinstance(n.layer, FusedConvAddAct)
                and _is_pointwise(n.layer.conv)
                and n.layer.act in _CHAIN_ACTS):
            continue
        for c in consumers.get(n.name, []):
            if (isinstance(c.layer, ConvBNAct) and _is_pointwise(c.layer)
                    and c.layer.act in _CHAIN_ACTS
                    and c.inputs == [n.name] and not c.kwargs):
                partner[n.name] = c
                break
    taken = {c.name for c in partner.values()}

    nodes: List[GraphNode] = []
    for n in graph.nodes:
        if n.name in taken:
            continue                   # emitted right after its add_k
        c = partner.get(n.name)
        if c is None:
            nodes.append(n)
            continue
        pair = n.name + "__chain"
        nodes.append(GraphNode(pair, ChainedExpandReduce(n.layer, c.layer),
                               list(n.inputs), dict(n.kwargs)))
        nodes.append(GraphNode(n.name, _Pick(0), [pair]))
        nodes.append(GraphNode(c.name, _Pick(1), [pair]))
    return LayerGraph(nodes, output=graph.output)


class ChainedExpandReduceProj(ChainedExpandReduce):
    """ChainedExpandReduce whose skip is a 1x1/s1 projection conv of xp
    (the first block of a stride-1 stage): the projection joins the call
    (ops.conv1x1_chain_proj), so its output is never a tensor of its own.
    .proj is the original module, shared like .expand and .reduce."""

    def __init__(self, expand: FusedConvAddAct, reduce: ConvBNAct,
                 proj: ConvBNAct):
        super().__init__(expand, reduce)
        self.proj = proj

    def forward(self, x, xp):
        from defer_amd import ops

        c3, c1, cp = self.expand.conv, self.reduce, self.proj
        return ops.conv1x1_chain_proj(
            x, c3.weight.to(x.dtype), c3.scale, c3.bias, xp,
            cp.weight.to(x.dtype), cp.scale, cp.bias, self.expand.act,
            c1.weight.to(x.dtype), c1.scale, c1.bias, c1.act)


def fuse_chain_projection(graph: LayerGraph) -> LayerGraph:
    """Fold a projection shortcut into its ChainedExpandReduce node: the
    node's residual input must be a 1x1/s1/p0 ConvBNAct without activation
    that takes one input, feeds this node and nothing else and is not the
    graph output. The node then takes [b, the projection's input] and the
    projection's node goes; names, picks and the two other modules stay.
    A stride-2 projection, one with another consumer and one whose add is
    not chained (its conv1 lives in the next stage) are left alone."""
    consumers = {}
    for n in graph.nodes:
        for p in n.inputs:
            consumers.setdefault(p, []).append(n)
    by_name = {n.name: n for n in graph.nodes}

    folded = {}                        # chain node name -> proj node
    for n in graph.nodes:
        if not (type(n.layer) is ChainedExpandReduce and len(n.inputs) == 2
                and not n.kwargs):
            continue
        p = by_name.get(n.inputs[1])
        if (p is not None and type(p.layer) is ConvBNAct
                and _is_pointwise(p.layer) and p.layer.act == "none"
                and len(p.inputs) == 1 and not p.kwargs
                and consumers.get(p.name, []) == [n]
                and p.name != graph.output):
            folded[n.name] = p
    gone = {p.name for p in folded.values()}

    nodes: List[GraphNode] = []
    for n in graph.nodes:
        if n.name in gone:
            continue
        p = folded.get(n.name)
        if p is None:
            nodes.append(n)
            continue
        layer = ChainedExpandReduceProj(n.layer.expand, n.layer.reduce,
                                        p.layer)
        nodes.append(GraphNode(n.name, layer, [n.inputs[0], p.inputs[0]]))
    return LayerGraph(nodes, output=graph.output)


class FusedConvPool(nn.Module):
    """pool(conv(x)) in one call. Both original modules stay referenced
    (not copied), so parameters are shared with the unfused graph."""

    def __init__(self, conv: ConvBNAct, pool: MaxPool):
        super().__init__()
        self.conv = conv
        self.pool = pool

    def forward(self, x):
        from defer_amd import ops

        c, q = self.conv, self.pool
        return ops.conv_bn_act_maxpool(
            x, c.weight.to(x.dtype), c.scale, c.bias, c.stride, c.padding,
            c.act, q.kernel, q.stride, q.padding)


def _is_stem_pool(c: ConvBNAct, q: MaxPool) -> bool:
    return (c.cin == 3 and c.cout == 64 and c.kernel == 7 and c.stride == 2
            and c.padding == 3 and c.act == "relu"
            and (q.kernel, q.stride, q.padding) == (3, 2, 1))


def fuse_conv_pool(graph: LayerGraph) -> LayerGraph:
    """Rewrite ConvBNAct -> MaxPool pairs into one FusedConvPool node that
    takes the pool's name. The conv must feed the pool and nothing else,
    take no residual and not be the graph output; a pool in another stage
    is simply not matched. Only the geometry the fused kernel serves is
    rewritten (_is_stem_pool); VGG's 3x3 conv -> 2x2/p0 pool pairs would
    run the op's two launches anyway and are left as they are."""
    consumers = {}
    for n in graph.nodes:
        for p in n.inputs:
            consumers.setdefault(p, []).append(n)

    partner = {}                       # conv name -> pool node
    for n in graph.nodes:
        if not (type(n.layer) is ConvBNAct and len(n.inputs) == 1
                and n.layer.act in _CHAIN_ACTS
                and not n.kwargs and n.name != graph.output):
            continue
        cs = consumers.get(n.name, [])
        if (len(cs) == 1 and type(cs[0].layer) is MaxPool
                and cs[0].inputs == [n.name] and not cs[0].kwargs
                and _is_stem_pool(n.layer, cs[0].layer)):
            partner[n.name] = cs[0]
    pools = {q.name: c for c, q in partner.items()}

    by_name = {n.name: n for n in graph.nodes}
    nodes: List[GraphNode] = []
    for n in graph.nodes:
        if n.name in partner:
            continue                   # folded into its pool's node
        c = pools.get(n.name)
        if c is None:
            nodes.append(n)
            continue
        conv = by_name[c]
        nodes.append(GraphNode(n.name, FusedConvPool(conv.layer, n.layer),
                               list(conv.inputs)))
    return LayerGraph(nodes, output=graph.output)
