"""MobileNetV2 and MobileNetV3-Large built as defer_amd LayerGraphs.

The standard edge model: inverted residual blocks of a 1x1 expand conv, a
3x3 depthwise conv and a linear 1x1 project conv, ReLU6 after the first
two. Its cost is streaming-bound (the depthwise layers have no reduction
over channels) where the ResNets' is MFMA-bound. Node names follow Keras
(`block_k_expand`, `block_k_depthwise`, `block_k_project`, `block_k_add`),
as the ResNets follow it for `add_N`; the identity blocks' `block_k_add`
and every `block_k_project` are cut points.

MobileNetV3-Large keeps the inverted residual and adds a squeeze-excite
block between the depthwise and the project conv of 8 of its 15 blocks,
5x5 depthwise kernels in 7 of them and hardswish in the stem, the later
blocks and the head. Its Keras names are `expanded_conv_k/expand` and so on;
here `/` is `_`, since names become module names and dump file names:
`expanded_conv_k_expand`, `_depthwise`, `_squeeze_excite`, `_project`,
`_add` (block 0 is `expanded_conv_...` without a number and has no expand).
"""

from typing import List

from defer_amd.graph import GraphModel, GraphNode, LayerGraph
from defer_amd.models.layers import (AddAct, ConvBNAct, Dense,
                                     DepthwiseConvBNAct, GlobalAvgPool,
                                     Hardswish, Softmax, SqueezeExcite)

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


# (depthwise kernel, expanded channels, output channels, squeeze-excite,
#  activation, stride)
_RE, _HS = "relu", "hardswish"
MOBILENET_V3_LARGE_TABLE = (
    (3, 16, 16, 0, _RE, 1), (3, 64, 24, 0, _RE, 2), (3, 72, 24, 0, _RE, 1),
    (5, 72, 40, 1, _RE, 2), (5, 120, 40, 1, _RE, 1), (5, 120, 40, 1, _RE, 1),
    (3, 240, 80, 0, _HS, 2), (3, 200, 80, 0, _HS, 1), (3, 184, 80, 0, _HS, 1),
    (3, 184, 80, 0, _HS, 1), (3, 480, 112, 1, _HS, 1),
    (3, 672, 112, 1, _HS, 1), (5, 672, 160, 1, _HS, 2),
    (5, 960, 160, 1, _HS, 1), (5, 960, 160, 1, _HS, 1))


def make_divisible(v: float, divisor: int = 8) -> int:
    """v rounded to the nearest multiple of `divisor`, at least `divisor`
    and never more than 10% below v (the MobileNet papers' rule)."""
    new = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new < 0.9 * v:
        new += divisor
    return new


def mobilenet_v3_large(num_classes: int = 1000,
                       include_top: bool = True) -> GraphModel:
    nodes: List[GraphNode] = []

    def N(name, layer, inputs):
        nodes.append(GraphNode(name, layer, inputs))
        return name

    x = N("Conv", ConvBNAct(3, 16, kernel=3, stride=2, padding=1, act=_HS),
          ["input"])
    cin = 16
    for k, (kernel, hidden, c, se, act, stride) in enumerate(
            MOBILENET_V3_LARGE_TABLE):
        p = "expanded_conv" if k == 0 else f"expanded_conv_{k}"
        y = x
        if hidden != cin:
            y = N(f"{p}_expand", ConvBNAct(cin, hidden, 1, 1, 0, act), [y])
        y = N(f"{p}_depthwise",
              DepthwiseConvBNAct(hidden, kernel, stride, kernel // 2, act),
              [y])
        if se:
            y = N(f"{p}_squeeze_excite",
                  SqueezeExcite(hidden, make_divisible(hidden / 4)), [y])
        y = N(f"{p}_project", ConvBNAct(hidden, c, 1, 1, 0, "none"), [y])
        if stride == 1 and cin == c:
            y = N(f"{p}_add", AddAct("none"), [y, x])
        x, cin = y, c
    x = N("Conv_1", ConvBNAct(cin, 960, 1, 1, 0, _HS), [x])
    if include_top:
        x = N("global_average_pooling2d", GlobalAvgPool(), [x])
        x = N("Conv_2", Dense(960, 1280), [x])
        x = N("Conv_2_hard_swish", Hardswish(), [x])
        x = N("predictions", Dense(1280, num_classes), [x])
        x = N("softmax", Softmax(), [x])
    return GraphModel(LayerGraph(nodes, output=x), name="mobilenetv3large")
