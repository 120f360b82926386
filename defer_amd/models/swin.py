"""Swin Transformer (V1) built as a defer_amd LayerGraph.

The hierarchical vision transformer: ConvNeXt's stage layout (a 4x4/s4
patchify stem, four stages, the map halved and the channels doubled between
them) with ViT's pre-norm block, whose attention acts inside window x window
tiles of the map and, in every second block, on the map shifted by half a
window. A block is

    LayerNorm -> qkv linear -> (shifted-)window attention -> proj linear -> + input
    LayerNorm -> linear d -> 4d + GELU -> linear 4d -> d -> + input

The map stays a 4-D NHWC tensor [N, H, W, C] from the stem to the head, so a
linear layer is the 1x1 ConvBNAct, the MLP's first layer PointwiseGelu and
the residual adds AddAct, which fuse into the conv before them. Two layers
are Swin's own. WindowAttention (ops.window_attention,
csrc/window_attention.hip) reads q, k and v in place from the qkv conv's
[N, H, W, 3C] output and does the roll, the window partition, the
relative-position bias, the mask and their inverses in its addressing.
Patch merging between stages is PatchMerge (ops.patch_merge, the gather of
each 2x2 patch into 4C channels), LayerNormC(4C) and a bias-free linear
4C -> 2C. The head dim is 32 everywhere, LayerNorm's eps 1e-5, and a block
does not shift where the map is no larger than the window (the last stage at
224), as in torchvision.

Node names are `{name}_patch_embed`, `_patch_layernorm`,
`_stage_{s}_block_{b}_{ln1, qkv, attn, proj, add_1, ln2, mlp_1, mlp_2,
add_2}`, `_merge_{s}_{gather, ln, reduce}` (in front of stage s),
`_head_layernorm`, `_head_gap`, `_head_dense` and `_softmax`; every `_add_1`
and `_add_2` is a cut point. The parameter counts are torchvision's
(swin_t: 28,288,354).
"""

from typing import List, Sequence

from defer_amd.graph import GraphModel, GraphNode, LayerGraph
from defer_amd.models.layers import (AddAct, ConvBNAct, Dense, GlobalAvgPool,
                                     LayerNormC, PatchMerge, PointwiseGelu,
                                     Softmax, WindowAttention)

_EPS = 1e-5


def _swin(depths: Sequence[int], dim: int, heads: Sequence[int],
          window: int = 7, image: int = 224, patch: int = 4,
          mlp_ratio: int = 4, name: str = "swin", num_classes: int = 1000,
          include_top: bool = True) -> GraphModel:
    if len(depths) != len(heads):
        raise ValueError(f"{len(depths)} depths for {len(heads)} heads")
    side = image // patch
    if image % patch or side % (window << (len(depths) - 1)):
        raise ValueError(
            f"image={image}: every stage's map must be a multiple of "
            f"window={window}")
    nodes: List[GraphNode] = []

    def N(node, layer, inputs):
        nodes.append(GraphNode(f"{name}_{node}", layer, inputs))
        return nodes[-1].name

    def lin(cin, cout, bias=True):
        return ConvBNAct(cin, cout, 1, 1, 0, "none", bn=False, bias=bias)

    x = N("patch_embed", ConvBNAct(3, dim, kernel=patch, stride=patch,
                                   padding=0, act="none", bn=False),
          ["input"])
    x = N("patch_layernorm", LayerNormC(dim, _EPS), [x])
    d = dim
    for s, (depth, h) in enumerate(zip(depths, heads)):
        if h * 32 != d:
            raise ValueError(f"stage {s}: {h} heads of 32 are not dim {d}")
        if s > 0:
            p = f"merge_{s}"
            x = N(f"{p}_gather", PatchMerge(), [x])
            x = N(f"{p}_ln", LayerNormC(2 * d, _EPS), [x])
            x = N(f"{p}_reduce", lin(2 * d, d, bias=False), [x])
        for b in range(depth):
            p = f"stage_{s}_block_{b}"
            shift = window // 2 if b % 2 and side > window else 0
            y = N(f"{p}_ln1", LayerNormC(d, _EPS), [x])
            y = N(f"{p}_qkv", lin(d, 3 * d), [y])
            y = N(f"{p}_attn", WindowAttention(h, window, shift), [y])
            y = N(f"{p}_proj", lin(d, d), [y])
            x = N(f"{p}_add_1", AddAct("none"), [y, x])
            y = N(f"{p}_ln2", LayerNormC(d, _EPS), [x])
            y = N(f"{p}_mlp_1", PointwiseGelu(d, mlp_ratio * d), [y])
            y = N(f"{p}_mlp_2", lin(mlp_ratio * d, d), [y])
            x = N(f"{p}_add_2", AddAct("none"), [y, x])
        d, side = 2 * d, side // 2
    if include_top:
        x = N("head_layernorm", LayerNormC(d // 2, _EPS), [x])
        x = N("head_gap", GlobalAvgPool(), [x])
        x = N("head_dense", Dense(d // 2, num_classes), [x])
        x = N("softmax", Softmax(), [x])
    return GraphModel(LayerGraph(nodes, output=x), name=name)


def swin_t(num_classes: int = 1000, include_top: bool = True) -> GraphModel:
    return _swin((2, 2, 6, 2), 96, (3, 6, 12, 24), name="swin_t",
                 num_classes=num_classes, include_top=include_top)


def swin_s(num_classes: int = 1000, include_top: bool = True) -> GraphModel:
    return _swin((2, 2, 18, 2), 96, (3, 6, 12, 24), name="swin_s",
                 num_classes=num_classes, include_top=include_top)


def swin_b(num_classes: int = 1000, include_top: bool = True) -> GraphModel:
    return _swin((2, 2, 18, 2), 128, (4, 8, 16, 32), name="swin_b",
                 num_classes=num_classes, include_top=include_top)
