"""MobileNetV2 built as a defer_amd LayerGraph.

The standard edge model: inverted residual blocks of a 1x1 expand conv, a
3x3 depthwise conv and a linear 1x1 project conv, ReLU6 after the first
two. Its cost is streaming-bound (the depthwise layers have no reduction
over channels) where the ResNets' is MFMA-bound. Node names follow Keras
(`block_k_expand`, `block_k_depthwise`, `block_k_project`, `block_k_add`),
as the ResNets follow it for `add_N`; the identity blocks' `block_k_add`
and every `block_k_project` are cut points.
"""

from typing import List

from defer_amd.graph import GraphModel, GraphNode, LayerGraph
from defer_amd.models.layers import (AddAct, ConvBNAct, Dense,
                                     DepthwiseConvBNAct, GlobalAvgPool,
                                     Softmax)

# (expansion t, output channels c, repeats n, stride of the first repeat s)
MOBILENET_V2_TABLE = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2),
                      (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2),
                      (6, 320, 1, 1))


def mobilenet_v2(num_classes: int = 1000,
                 include_top: bool = True) -> GraphModel:
    nodes: List[GraphNode] = []

    def N(name, layer, inputs):
        nodes.append(GraphNode(name, layer, inputs))
        return name

    x = N("Conv1", ConvBNAct(3, 32, kernel=3, stride=2, padding=1,
                             act="relu6"), ["input"])
    cin = 32
    k = 0                               # Keras block index
    for t, c, n, s in MOBILENET_V2_TABLE:
        for i in range(n):
            stride = s if i == 0 else 1
            p = "expanded_conv" if k == 0 else f"block_{k}"
            hidden = cin * t
            y = x
            if t != 1:
                y = N(f"{p}_expand",
                      ConvBNAct(cin, hidden, 1, 1, 0, "relu6"), [y])
            y = N(f"{p}_depthwise",
                  DepthwiseConvBNAct(hidden, 3, stride, 1, "relu6"), [y])
            y = N(f"{p}_project", ConvBNAct(hidden, c, 1, 1, 0, "none"), [y])
            if stride == 1 and cin == c:
                y = N(f"{p}_add", AddAct("none"), [y, x])
            x, cin = y, c
            k += 1
    x = N("Conv_1", ConvBNAct(cin, 1280, 1, 1, 0, "relu6"), [x])
    if include_top:
        x = N("global_average_pooling2d", GlobalAvgPool(), [x])
        x = N("predictions", Dense(1280, num_classes), [x])
        x = N("softmax", Softmax(), [x])
    return GraphModel(LayerGraph(nodes, output=x), name="mobilenetv2")
