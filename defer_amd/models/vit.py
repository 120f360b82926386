"""Vision Transformer built as a defer_amd LayerGraph.

A patchify stem (a patch x patch / stride patch conv), a class token and a
learned position embedding, `depth` pre-norm transformer blocks, and a
LayerNorm + linear head on the class token. A block is

    LayerNorm -> qkv linear -> multi-head attention -> proj linear -> + input
    LayerNorm -> linear d -> 4d + GELU -> linear 4d -> d -> + input

The token sequence stays a 4-D NHWC tensor [N, 1, T, C] from the embedding
to the head, so a linear layer over the channels is the 1x1 ConvBNAct (no
BN: `scale` is None, `bias` the linear bias) that the convnets use, the MLP's
first layer is ConvNeXt's PointwiseGelu, the residual adds are AddAct (and
fuse into the conv before them), and the codecs see the activation shapes
they know. The one layer the convnets lack is Attention (ops.attention,
csrc/attention.hip), which reads q, k and v in place from the qkv conv's
[N, 1, T, 3C] output: no split, permute or head transpose is ever made.

Node names are `{name}_patch_embed`, `_embed`, `_block_{b}_{ln1, qkv, attn,
proj, add_1, ln2, mlp_1, mlp_2, add_2}`, `_class_token`, `_head_layernorm`,
`_head_dense` and `_softmax`; every `_add_1` and `_add_2` is a cut point.
The parameter counts are torchvision's (vit_b_16: 86,567,656).
"""

from typing import List

from defer_amd.graph import GraphModel, GraphNode, LayerGraph
from defer_amd.models.layers import (AddAct, Attention, ClassToken, ConvBNAct,
                                     Dense, LayerNormC, PointwiseGelu,
                                     Softmax, TokenEmbed)


def _vit(depth: int, dim: int, heads: int, patch: int, image: int,
         mlp_ratio: int = 4, name: str = "vit", num_classes: int = 1000,
         include_top: bool = True) -> GraphModel:
    if image % patch:
        raise ValueError(f"patch={patch} does not divide image={image}")
    nodes: List[GraphNode] = []

    def N(node, layer, inputs):
        nodes.append(GraphNode(f"{name}_{node}", layer, inputs))
        return nodes[-1].name

    def lin(cin, cout):
        return ConvBNAct(cin, cout, 1, 1, 0, "none", bn=False)

    x = N("patch_embed", ConvBNAct(3, dim, kernel=patch, stride=patch,
                                   padding=0, act="none", bn=False),
          ["input"])
    x = N("embed", TokenEmbed(1 + (image // patch) ** 2, dim), [x])
    for b in range(depth):
        p = f"block_{b}"
        y = N(f"{p}_ln1", LayerNormC(dim), [x])
        y = N(f"{p}_qkv", lin(dim, 3 * dim), [y])
        y = N(f"{p}_attn", Attention(heads), [y])
        y = N(f"{p}_proj", lin(dim, dim), [y])
        x = N(f"{p}_add_1", AddAct("none"), [y, x])
        y = N(f"{p}_ln2", LayerNormC(dim), [x])
        y = N(f"{p}_mlp_1", PointwiseGelu(dim, mlp_ratio * dim), [y])
        y = N(f"{p}_mlp_2", lin(mlp_ratio * dim, dim), [y])
        x = N(f"{p}_add_2", AddAct("none"), [y, x])
    if include_top:
        x = N("class_token", ClassToken(), [x])
        x = N("head_layernorm", LayerNormC(dim), [x])
        x = N("head_dense", Dense(dim, num_classes), [x])
        x = N("softmax", Softmax(), [x])
    return GraphModel(LayerGraph(nodes, output=x), name=name)


def vit_b16(num_classes: int = 1000, include_top: bool = True) -> GraphModel:
    return _vit(12, 768, 12, 16, 224, name="vit_b16",
                num_classes=num_classes, include_top=include_top)


def vit_s16(num_classes: int = 1000, include_top: bool = True) -> GraphModel:
    return _vit(12, 384, 6, 16, 224, name="vit_s16",
                num_classes=num_classes, include_top=include_top)
