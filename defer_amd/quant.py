"""Post-training fp8 (OCP e4m3) quantisation of a LayerGraph.

quantize_graph(graph, calib_inputs) returns a new LayerGraph in which every
convolution the fp8 kernel serves (csrc/conv_fp8.hip: Cin % 16 == 0, Cout %
16 == 0, act none / relu / relu6) runs on e4m3 bytes:

  1. the unquantised graph runs on the calibration inputs and the amax of
     every tensor is recorded;
  2. fuse_residual_adds folds conv -> AddAct pairs, so a residual add is the
     conv's epilogue (the fused node keeps the add's name);
  3. each eligible ConvBNAct / FusedConvAddAct becomes a ConvBNActFP8 with
     per-output-channel weight scales (amax / 448) and static per-tensor
     activation scales (amax / 448). It writes e4m3 when every reader of its
     output is a converted conv (as input or as residual), bf16 otherwise; a
     QuantizeFP8 node `<producer>_fp8` goes in wherever a bf16 tensor feeds a
     converted conv.

Everything else keeps running as it was (the 3-channel stem and its pool,
GAP, Dense, Softmax). Node names are kept, so cut-point names stay valid.
The original modules are not modified.
"""

from typing import Dict, Iterable, List, Optional, Tuple

import torch

from defer_amd.graph import GraphNode, LayerGraph
from defer_amd.models.layers import ConvBNAct, ConvBNActFP8, QuantizeFP8
from defer_amd.parallel.fusion import FusedConvAddAct, fuse_residual_adds

E4M3_MAX = 448.0
_ACTS = ("none", "relu", "relu6")


def _conv_of(layer) -> Optional[Tuple[ConvBNAct, str]]:
    """(conv, act) of a node the pass looks at, None for any other layer."""
    if isinstance(layer, FusedConvAddAct):
        return layer.conv, layer.act
    if isinstance(layer, ConvBNAct):
        return layer, layer.act
    return None


def _kept_reason(conv: ConvBNAct, act: str) -> Optional[str]:
    """Why the fp8 kernel does not serve this conv, None when it does."""
    if conv.cin % 16 or conv.cout % 16:
        return f"channels {conv.cin}->{conv.cout} are not multiples of 16"
    if act not in _ACTS:
        return f"act={act!r} has no fp8 epilogue"
    if conv.stride not in (1, 2) or not 0 <= conv.padding <= conv.kernel // 2:
        return f"stride {conv.stride} / padding {conv.padding} not served"
    return None


def _graph_of(graph) -> LayerGraph:
    return graph if isinstance(graph, LayerGraph) else graph.graph


def calibrate_amax(graph: LayerGraph,
                   calib_inputs: Iterable[torch.Tensor]) -> Dict[str, float]:
    """amax of the input and of every node's output over the inputs."""
    amax: Dict[str, float] = {}

    def see(name, t):
        amax[name] = max(amax.get(name, 0.0), float(t.float().abs().max()))

    with torch.no_grad():
        for x in calib_inputs:
            env = {LayerGraph.INPUT: x}
            see(LayerGraph.INPUT, x)
            for n in graph.nodes:
                env[n.name] = n.layer(*[env[p] for p in n.inputs], **n.kwargs)
                see(n.name, env[n.name])
    if not amax:
        raise ValueError("quantize_graph: no calibration inputs")
    return amax


def quantize_graph(graph, calib_inputs) -> LayerGraph:
    graph = _graph_of(graph)
    amax = calibrate_amax(graph, calib_inputs)
    g = fuse_residual_adds(graph)

    def act_scale(name):
        return max(amax[name], 1e-12) / E4M3_MAX

    converted = set()
    for n in g.nodes:
        ca = _conv_of(n.layer)
        if ca is not None and _kept_reason(*ca) is None:
            converted.add(n.name)
    readers: Dict[str, List[str]] = {}
    for n in g.nodes:
        for p in n.inputs:
            readers.setdefault(p, []).append(n.name)
    # a tensor is e4m3 when a converted conv writes it for converted readers
    is_fp8 = {
        n.name for n in g.nodes
        if n.name in converted and n.name != g.output
        and all(r in converted for r in readers.get(n.name, []))}

    nodes: List[GraphNode] = []
    quantised = set()

    def fp8_name(p):
        """The e4m3 form of tensor p, a quantise node added on first use."""
        if p in is_fp8:
            return p
        q = f"{p}_fp8"
        if p not in quantised:
            quantised.add(p)
            nodes.append(GraphNode(q, QuantizeFP8(act_scale(p)), [p]))
        return q

    for n in g.nodes:
        if n.name not in converted:
            nodes.append(n)
            continue
        conv, act = _conv_of(n.layer)
        ins = [fp8_name(p) for p in n.inputs]
        layer = ConvBNActFP8(
            conv, act, x_scale=act_scale(n.inputs[0]),
            res_scale=act_scale(n.inputs[1]) if len(n.inputs) > 1 else None,
            out_scale=act_scale(n.name) if n.name in is_fp8 else None)
        nodes.append(GraphNode(n.name, layer, ins, dict(n.kwargs)))
    return LayerGraph(nodes, output=g.output)


def report(graph) -> List[Tuple[str, str]]:
    """(node name, status) for every node, in graph order: "fp8 -> e4m3" or
    "fp8 -> bf16" for a converted conv, "quantize" for an inserted node,
    "kept: <reason>" for a conv the fp8 kernel does not serve and "kept" for
    every other layer. Given a graph that has not been quantised, it reports
    what quantize_graph would do to its convs (as "fp8") without running
    anything."""
    g = _graph_of(graph)
    if not any(isinstance(n.layer, (ConvBNActFP8, QuantizeFP8))
               for n in g.nodes):
        g = fuse_residual_adds(g)
    rows = []
    for n in g.nodes:
        lay = n.layer
        ca = _conv_of(lay)
        if isinstance(lay, ConvBNActFP8):
            rows.append((n.name, "fp8 -> bf16" if lay.out_scale is None
                         else "fp8 -> e4m3"))
        elif isinstance(lay, QuantizeFP8):
            rows.append((n.name, "quantize"))
        elif ca is not None:
            why = _kept_reason(*ca)
            rows.append((n.name, "fp8" if why is None else f"kept: {why}"))
        else:
            rows.append((n.name, "kept"))
    return rows
