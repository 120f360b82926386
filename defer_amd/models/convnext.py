"""ConvNeXt built as a defer_amd LayerGraph.

The convnet that took the ResNets' place: a 4x4/s4 patchify stem, four
stages of blocks with 2x2/s2 downsampling between them, LayerNorm over the
channels instead of BatchNorm and GELU instead of ReLU. A block is

    7x7 depthwise conv -> LayerNorm -> 1x1 d -> 4d + GELU -> 1x1 4d -> d
    -> layer scale -> + input

and runs as DepthwiseConv7x7, LayerNormC, PointwiseGelu, a 1x1 ConvBNAct
and AddAct. The layer scale gamma is folded into the last conv, as BN is
elsewhere: its `scale` is gamma and its `bias` the conv bias times gamma,
which keeps the parameter count of the unfolded block. Random init sets
gamma to 1 where ConvNeXt trains from 1e-6, so that the residual branches
carry weight in a benchmark on random weights; activations stay O(1)
because every block renormalises its branch.

Node names follow Keras (`convnext_tiny_stage_s_block_b_depthwise_conv`,
`_layernorm`, `_pointwise_conv_1`, `_pointwise_conv_2`; the stem and the
downsampling blocks, Sequentials there, are `_stem_conv`, `_stem_layernorm`,
`_downsampling_block_k_layernorm`, `_downsampling_block_k_conv`), and every
block ends in a `..._add`, a cut point.
"""

from typing import List, Sequence

from defer_amd.graph import GraphModel, GraphNode, LayerGraph
from defer_amd.models.layers import (AddAct, ConvBNAct, Dense,
                                     DepthwiseConv7x7, GlobalAvgPool,
                                     LayerNormC, PointwiseGelu, Softmax)


def _convnext(depths: Sequence[int], dims: Sequence[int], name: str,
              num_classes: int = 1000, include_top: bool = True) -> GraphModel:
    nodes: List[GraphNode] = []

    def N(node, layer, inputs):
        nodes.append(GraphNode(f"{name}_{node}", layer, inputs))
        return nodes[-1].name

    x = N("stem_conv", ConvBNAct(3, dims[0], kernel=4, stride=4, padding=0,
                                 act="none", bn=False), ["input"])
    x = N("stem_layernorm", LayerNormC(dims[0]), [x])
    for s, (depth, d) in enumerate(zip(depths, dims)):
        if s > 0:
            p = f"downsampling_block_{s - 1}"
            x = N(f"{p}_layernorm", LayerNormC(dims[s - 1]), [x])
            x = N(f"{p}_conv", ConvBNAct(dims[s - 1], d, kernel=2, stride=2,
                                         padding=0, act="none", bn=False),
                  [x])
        for b in range(depth):
            p = f"stage_{s}_block_{b}"
            y = N(f"{p}_depthwise_conv", DepthwiseConv7x7(d), [x])
            y = N(f"{p}_layernorm", LayerNormC(d), [y])
            y = N(f"{p}_pointwise_conv_1", PointwiseGelu(d, 4 * d), [y])
            y = N(f"{p}_pointwise_conv_2",
                  ConvBNAct(4 * d, d, 1, 1, 0, "none"), [y])
            x = N(f"{p}_add", AddAct("none"), [y, x])
    if include_top:
        x = N("head_gap", GlobalAvgPool(), [x])
        x = N("head_layernorm", LayerNormC(dims[-1]), [x])
        x = N("head_dense", Dense(dims[-1], num_classes), [x])
        x = N("softmax", Softmax(), [x])
    return GraphModel(LayerGraph(nodes, output=x), name=name)


def convnext_tiny(num_classes: int = 1000,
                  include_top: bool = True) -> GraphModel:
    return _convnext((3, 3, 9, 3), (96, 192, 384, 768), "convnext_tiny",
                     num_classes, include_top)
