"""Lower an FX-imported torch model onto the project's NHWC HIP layers.

`from_torch` keeps `nn.Conv2d`, `nn.BatchNorm2d`, `nn.Linear` and friends
as leaf modules: an imported model runs in NCHW through PyTorch's own
kernels and reaches none of the HIP path. `lower_torch` rewrites the same
FX graph into the layer classes the model zoo is made of (`ConvBNAct`,
`AddAct`, `MaxPool`, `Dense`, ...), so the kernels, the fusion passes of
`parallel/fusion.py` and the partitioner's cost model all apply.

The user's convention is kept: the graph takes the NCHW tensor the torch
model takes and returns the tensor it would return. Inside, every 4-D
value carries a layout tag. The graph input and the outputs of nodes that
stayed torch code ("islands") are NCHW, the outputs of lowered 4-D ops are
NHWC; where a consumer needs the other layout one conversion node per
(value, layout) is inserted, named `<producer>__nhwc` / `<producer>__nchw`,
and shared between consumers.

The patterns:

    Conv2d [+ BatchNorm2d] [+ ReLU | ReLU6 | Hardswish]
                                                   -> ConvBNAct
    depthwise Conv2d [+ BatchNorm2d] [+ ReLU | ReLU6 | Hardswish]
        (groups == in == out channels, 3x3 or 5x5, stride 1 or 2,
         padding <= k // 2, C % 8 == 0)            -> DepthwiseConvBNAct
    v * hardsigmoid(conv1x1(relu(conv1x1(pool(v)))))
        (squeeze-excite, see below)                -> SqueezeExcite
    BatchNorm2d [+ ReLU]                           -> BNAct
    a + b [+ ReLU]                                 -> AddAct
    Linear [+ ReLU]                                -> Dense
    ReLU anywhere else                             -> Relu
    ReLU6 anywhere else                            -> Relu6
    Hardswish anywhere else                        -> Hardswish
    MaxPool2d / AvgPool2d                          -> MaxPool / AvgPool
    AdaptiveAvgPool2d(1) or F.adaptive_avg_pool2d(x, 1) + flatten,
        mean over dims (2, 3)                      -> GlobalAvgPool
    cat over dim 1, flatten into Linear, softmax   -> Concat, Flatten, Softmax

ReLU6 is `nn.ReLU6`, `F.relu6`, `nn.Hardtanh(0., 6.)` or
`F.hardtanh(x, 0., 6.)`. Every other grouped conv (groups between 1 and C,
a channel multiplier) stays an island. Hardswish is `nn.Hardswish` or
`F.hardswish`, in place or not.

Squeeze-excite is a `mul` (`a * b`, `torch.mul`, `a.mul(b)`, either operand
order) of a 4-D value v with the chain `AdaptiveAvgPool2d(1)` |
`F.adaptive_avg_pool2d(v, 1)` | `v.mean((2, 3), keepdim=True)` -> 1x1
Conv2d C -> Cr -> ReLU or nothing -> 1x1 Conv2d Cr -> C -> `nn.Hardsigmoid`
| `F.hardsigmoid`, bias optional on both convs, in which every node has the
next as its only consumer and C % 8 == 0. Any other such chain (a sigmoid
gate, a SiLU between the convs, a value of the chain read elsewhere) stays
islands, with the reason on its pooling node.

A pattern (conv [+ BN] [+ ReLU], add [+ ReLU], linear [+ ReLU], ...) is
fused only through intermediates with exactly one consumer, and the fused
node takes the name of the pattern's last node, so a cut name that refers
to the pattern's output stays valid. A pattern is lowered only where the
HIP op accepts its shape in both compute dtypes (the `TORCH_CHECK`s of
`csrc/bindings.cpp`); anything else stays an island, with the reason
recorded in the `TorchIsland` that wraps it.

In-place ops: torch writes an in-place ReLU, ReLU6, Hardswish or `a += b`
into its input,
so a later reader of that tensor sees the result. The lowered ops are out
of place; such a node, when its input has other readers, is emitted on
its own and the input's name is rebound to its output for everything that
follows. Other in-place ops stay islands and act on their own NCHW copy.

Inference only: lowered layers own folded copies of the parameters, and
the model is traced and folded on the CPU.
"""

import operator
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from defer_amd.graph import (GraphNode, LayerGraph, fx_call_layer,
                             fx_node_names, fx_trace)
from defer_amd.models import layers as L

NCHW, NHWC = "nchw", "nhwc"

# what the HIP ops take in BOTH compute dtypes (csrc/bindings.cpp): the
# bf16 kernels move 8 elements per lane and the fp32 ones 4, so the bf16
# rule covers both, except for the conv's Cout and the linear's N, which
# only the fp32 kernels constrain
_VEC = 8            # bn_act / pools / global_avg_pool: C; add_act / relu:
#                     numel; bf16 linear: K (fp32: K % 4)
_COUT_VEC = 4       # fp32 conv: Cout % 4; fp32 linear: N % 4
_MAX_NO_SCALE = 8192    # conv without a scale vector: cached ones[8192]
_DW_KERNELS = (3, 5)    # depthwise conv (csrc/dwconv.hip): square kernels,
_DW_STRIDES = (1, 2)    # strides, 0 <= padding <= k // 2, C % _VEC == 0


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _square(v) -> Optional[int]:
    a, b = _pair(v)
    return a if a == b and isinstance(a, int) else None


class _Lowering:
    def __init__(self, model: nn.Module, input_shape):
        import torch.fx as fx
        from torch.fx.passes.shape_prop import ShapeProp

        self.g, self.modules = fx_trace(model)
        self.names = fx_node_names(self.g)
        self.by_fx_name = {n.name: n for n in self.g.nodes}
        off_cpu = {str(t.device) for t in list(model.parameters())
                   + list(model.buffers()) if t.device.type != "cpu"}
        if off_cpu:
            raise ValueError(
                "lower_torch traces shapes and folds parameters on the CPU, "
                f"but the model has tensors on {sorted(off_cpu)}: call "
                "model.cpu() first (StageExecutor moves the lowered graph "
                "to its device)")
        with torch.no_grad():
            p0 = next(model.parameters(), None)
            x = torch.zeros(*input_shape,
                            dtype=p0.dtype if p0 is not None
                            and p0.is_floating_point() else torch.float32)
            ShapeProp(fx.GraphModule(model, self.g)).propagate(x)
        self.nodes: List[GraphNode] = []
        # fx node -> {layout tag: LayerGraph node name}; the tag is NCHW or
        # NHWC for a 4-D value and None for every other value
        self.vals: Dict[object, Dict[Optional[str], str]] = {}
        self.done = set()           # fx nodes taken in by an earlier pattern
        self.flat_chw: Dict[object, Tuple[int, int, int]] = {}

    # ------------------------------------------------------------- helpers
    def shape(self, n) -> Optional[tuple]:
        tm = n.meta.get("tensor_meta")
        return tuple(tm.shape) if hasattr(tm, "shape") else None

    def rank(self, n) -> int:
        s = self.shape(n)
        return -1 if s is None else len(s)

    def mod(self, n):
        return self.modules[n.target] if n.op == "call_module" else None

    def use(self, n, layout: Optional[str]) -> str:
        """The LayerGraph name of value `n` in `layout`, inserting the
        conversion node on first need."""
        d = self.vals[n]
        if None in d:
            return d[None]
        if layout not in d:
            src = next(iter(d.values()))
            name = f"{src}__{layout}"
            layer = L.ToNHWC() if layout == NHWC else L.ToNCHW()
            self.nodes.append(GraphNode(name, layer, [src]))
            d[layout] = name
        return d[layout]

    def emit(self, last, layer, inputs: List[str], layout, chain):
        name = self.names[last.name]
        self.nodes.append(GraphNode(name, layer, inputs))
        self.vals[last] = {layout: name}
        self.done.update(chain)

    def sole_user(self, n):
        return next(iter(n.users)) if len(n.users) == 1 else None

    def removable(self, n) -> bool:
        m = self.mod(n)
        if isinstance(m, nn.Identity):
            return True
        return isinstance(m, (nn.Dropout, nn.Dropout2d)) and not m.training

    def real_users(self, n) -> list:
        """Users of `n`, looking through the nodes that lowering removes."""
        out = []
        for u in n.users:
            out.extend(self.real_users(u) if self.removable(u) else [u])
        return out

    def is_relu(self, n, of) -> bool:
        if not n.args or n.args[0] is not of:
            return False
        if n.op == "call_module":
            return type(self.mod(n)) is nn.ReLU
        if n.op == "call_function":
            return n.target in (torch.relu, F.relu, torch.relu_, F.relu_)
        return n.op == "call_method" and n.target in ("relu", "relu_")

    @staticmethod
    def _arg(n, i, name, default):
        return n.args[i] if len(n.args) > i else n.kwargs.get(name, default)

    def is_relu6(self, n, of) -> bool:
        """nn.ReLU6, F.relu6, nn.Hardtanh(0., 6.), F.hardtanh(x, 0., 6.)"""
        if not n.args or n.args[0] is not of:
            return False
        if n.op == "call_module":
            m = self.mod(n)
            if type(m) is nn.ReLU6:
                return True
            return (type(m) is nn.Hardtanh and m.min_val == 0
                    and m.max_val == 6)
        if n.op != "call_function":
            return False
        if n.target is F.relu6:
            return True
        return (n.target in (F.hardtanh, F.hardtanh_)
                and self._arg(n, 1, "min_val", -1.0) == 0
                and self._arg(n, 2, "max_val", 1.0) == 6)

    def is_hardswish(self, n, of) -> bool:
        """nn.Hardswish or F.hardswish, in place or not"""
        if not n.args or n.args[0] is not of:
            return False
        if n.op == "call_module":
            return type(self.mod(n)) is nn.Hardswish
        return n.op == "call_function" and n.target is F.hardswish

    def mutates_input(self, n) -> bool:
        """An in-place ReLU, ReLU6, Hardswish or `a += b`: torch writes the
        result into args[0], so every LATER reader of that tensor sees it."""
        if n.op == "call_module":
            m = self.mod(n)
            return (type(m) in (nn.ReLU, nn.ReLU6, nn.Hardtanh, nn.Hardswish)
                    and m.inplace)
        if n.op == "call_function":
            if n.target in (torch.relu_, F.relu_, F.hardtanh_,
                            operator.iadd):
                return True
            if n.target in (F.relu, F.relu6, F.hardswish):
                return bool(self._arg(n, 1, "inplace", False))
            return n.target is F.hardtanh and bool(
                self._arg(n, 3, "inplace", False))
        return n.op == "call_method" and n.target == "relu_"

    def rebind_mutated(self, n):
        """After an in-place node `n` was emitted on its own: the tensor it
        wrote into (args[0], and every alias of it) now names n's output,
        as it does in torch. Readers that came before n already took the
        old value. Fused patterns never need this: they fuse only through
        values with a single consumer."""
        if self.mutates_input(n) and n.args[0] in self.vals:
            d = self.vals[n.args[0]]
            new = dict(self.vals[n])
            d.clear()
            d.update(new)
            self.vals[n] = d

    def relu_after(self, n):
        """The ReLU that is `n`'s only consumer (the producer's kernel can
        then apply it), or None."""
        u = self.sole_user(n)
        return u if u is not None and self.is_relu(u, n) else None

    def act_after(self, n):
        """(node, "relu" | "relu6" | "hardswish") for the activation that is
        `n`'s only consumer, for the convs, whose kernels apply any of them;
        (None, "none") otherwise."""
        u = self.sole_user(n)
        if u is not None and self.is_relu(u, n):
            return u, "relu"
        if u is not None and self.is_relu6(u, n):
            return u, "relu6"
        if u is not None and self.is_hardswish(u, n):
            return u, "hardswish"
        return None, "none"

    def is_flatten1(self, n, of) -> bool:
        """flatten(of, 1): nn.Flatten(), torch.flatten(x, 1), x.flatten(1)"""
        if not n.args or n.args[0] is not of:
            return False
        m = self.mod(n)
        if m is not None:
            return (type(m) is nn.Flatten and m.start_dim == 1
                    and m.end_dim in (-1, self.rank(of) - 1))
        if not ((n.op == "call_function" and n.target is torch.flatten)
                or (n.op == "call_method" and n.target == "flatten")):
            return False
        start = n.args[1] if len(n.args) > 1 else n.kwargs.get("start_dim", 0)
        end = n.args[2] if len(n.args) > 2 else n.kwargs.get("end_dim", -1)
        return start == 1 and end in (-1, self.rank(of) - 1)

    def linear_reason(self, n) -> Optional[str]:
        m = self.mod(n)
        s = self.shape(n.args[0])
        if s is None or len(s) != 2:
            return "Linear on a value that is not 2-D"
        if m.in_features % _VEC:
            return (f"Linear in_features={m.in_features}: the bf16 linear "
                    f"needs K % {_VEC} == 0")
        if m.out_features % _COUT_VEC:
            return (f"Linear out_features={m.out_features}: the fp32 linear "
                    f"needs N % {_COUT_VEC} == 0")
        if m.out_features > _MAX_NO_SCALE:
            return (f"Linear out_features={m.out_features}: the bf16 linear "
                    f"passes no scale and takes at most N = {_MAX_NO_SCALE}")
        return None

    # ------------------------------------------------------------ patterns
    def lower_conv(self, n) -> Optional[str]:
        m = self.mod(n)
        s = self.shape(n.args[0])
        if s is None or len(s) != 4:
            return "Conv2d on a value that is not 4-D"
        depthwise = (m.groups > 1 and m.groups == m.in_channels
                     and m.groups == m.out_channels)
        if m.groups != 1 and not depthwise:
            return (f"grouped conv (groups={m.groups}, {m.in_channels} -> "
                    f"{m.out_channels} channels): only depthwise convs "
                    "(groups == in == out channels) are lowered")
        if _pair(m.dilation) != (1, 1):
            return f"dilated conv (dilation={tuple(m.dilation)})"
        if m.padding_mode != "zeros":
            return f"padding_mode={m.padding_mode!r}"
        k, st = _square(m.kernel_size), _square(m.stride)
        pad = None if isinstance(m.padding, str) else _square(m.padding)
        if k is None or st is None or pad is None:
            return (f"conv geometry kernel={m.kernel_size} stride={m.stride} "
                    f"padding={m.padding}: needs a square kernel and equal "
                    "stride and padding in both dims")
        if depthwise:
            c = m.groups
            if k not in _DW_KERNELS or st not in _DW_STRIDES or pad > k // 2:
                return (f"depthwise conv (groups={c}) kernel={k} stride={st} "
                        f"padding={pad}: the depthwise kernel takes "
                        f"{_DW_KERNELS} kernels, strides {_DW_STRIDES} and "
                        "padding <= kernel // 2")
            if c % _VEC:
                return (f"depthwise conv (groups={c}): the bf16 depthwise "
                        f"kernel needs C % {_VEC} == 0")
        elif m.out_channels % _COUT_VEC:
            return (f"Conv2d out_channels={m.out_channels}: the fp32 conv "
                    f"needs Cout % {_COUT_VEC} == 0")
        if s[2] + 2 * pad < k or s[3] + 2 * pad < k:
            return "conv kernel larger than the padded input"
        chain, last = [n], n
        bn = None
        u = self.sole_user(n)
        if (u is not None and type(self.mod(u)) is nn.BatchNorm2d
                and u.args[0] is n and _bn_foldable(self.mod(u))):
            bn = self.mod(u)
            chain.append(u)
            last = u
        if bn is None and m.out_channels > _MAX_NO_SCALE:
            return (f"Conv2d out_channels={m.out_channels} without a "
                    f"BatchNorm: more than {_MAX_NO_SCALE}")
        r, act = self.act_after(last)
        if r is not None:
            chain.append(r)
            last = r
        w = m.weight.detach()
        if depthwise:
            layer = L.DepthwiseConvBNAct(m.groups, kernel=k, stride=st,
                                         padding=pad, act=act,
                                         bn=bn is not None)
            layer.weight = nn.Parameter(                # [C,1,R,S] -> RSC
                w[:, 0].permute(1, 2, 0).contiguous().float())
        else:
            layer = L.ConvBNAct(m.in_channels, m.out_channels, kernel=k,
                                stride=st, padding=pad, act=act,
                                bn=bn is not None)
            layer.weight = nn.Parameter(
                w.permute(0, 2, 3, 1).contiguous().float())  # OIHW -> OHWI
        b = (m.bias.detach().double() if m.bias is not None
             else torch.zeros(m.out_channels, dtype=torch.float64))
        if bn is not None:
            scale, shift = _bn_fold(bn)
            layer.scale = nn.Parameter(scale.float())
            b = shift + b * scale                # beta + (b - mean) * scale
        layer.bias = nn.Parameter(b.float())
        self.emit(last, layer, [self.use(n.args[0], NHWC)], NHWC, chain)
        return None

    def lower_bn(self, n) -> Optional[str]:
        m = self.mod(n)
        s = self.shape(n.args[0])
        if s is None or len(s) != 4:
            return "BatchNorm2d on a value that is not 4-D"
        if not _bn_foldable(m):
            return "BatchNorm2d without running statistics"
        if s[1] % _VEC:
            return f"BatchNorm2d on C={s[1]}: bn_act needs C % {_VEC} == 0"
        chain, last = [n], n
        r = self.relu_after(n)
        if r is not None:
            chain.append(r)
            last = r
        layer = L.BNAct(s[1], act="relu" if r is not None else "none")
        scale, shift = _bn_fold(m)
        layer.scale = nn.Parameter(scale.float())
        layer.bias = nn.Parameter(shift.float())
        self.emit(last, layer, [self.use(n.args[0], NHWC)], NHWC, chain)
        return None

    def lower_add(self, n) -> Optional[str]:
        import torch.fx as fx

        if (len(n.args) != 2 or n.kwargs
                or not all(isinstance(a, fx.Node) for a in n.args)):
            return "add of something other than two tensors"
        a, b = n.args
        sa, sb = self.shape(a), self.shape(b)
        if sa is None or sa != sb or len(sa) != 4:
            return "add of values that are not 4-D of one shape"
        numel = sa[0] * sa[1] * sa[2] * sa[3]
        if numel % _VEC:
            return f"add of {numel} elements: add_act needs numel % {_VEC} == 0"
        chain, last = [n], n
        # `a += b` whose `a` is read again later: the sum itself must stay
        # a value (those readers see it), so the ReLU is not taken in
        shared = self.mutates_input(n) and len(a.users) > 1
        r = None if shared else self.relu_after(n)
        if r is not None:
            chain.append(r)
            last = r
        self.emit(last, L.AddAct("relu" if r is not None else "none"),
                  [self.use(a, NHWC), self.use(b, NHWC)], NHWC, chain)
        if shared:
            self.rebind_mutated(n)
        return None

    def lower_relu(self, n) -> Optional[str]:
        s = self.shape(n)
        if s is None:
            return "ReLU of a value of unknown shape"
        numel = 1
        for d in s:
            numel *= d
        if numel % _VEC:
            return f"ReLU of {numel} elements: relu needs numel % {_VEC} == 0"
        layout = NHWC if len(s) == 4 else None
        self.emit(n, L.Relu(), [self.use(n.args[0], layout)], layout, [n])
        self.rebind_mutated(n)
        return None

    def lower_relu6(self, n, what="ReLU6", op="relu6",
                    layer=L.Relu6) -> Optional[str]:
        """A ReLU6, or a Hardswish (same numel rule), on its own."""
        s = self.shape(n)
        if s is None:
            return f"{what} of a value of unknown shape"
        numel = 1
        for d in s:
            numel *= d
        if numel % _VEC:
            return (f"{what} of {numel} elements: {op} needs "
                    f"numel % {_VEC} == 0")
        layout = NHWC if len(s) == 4 else None
        self.emit(n, layer(), [self.use(n.args[0], layout)], layout, [n])
        self.rebind_mutated(n)
        return None

    def lower_hardswish(self, n) -> Optional[str]:
        return self.lower_relu6(n, "Hardswish", "hardswish", L.Hardswish)

    # ------------------------------------------------------ squeeze-excite
    def _what(self, n) -> str:
        m = self.mod(n)
        return type(m).__name__ if m is not None else getattr(
            n.target, "__name__", str(n.target))

    def is_pool_to_1x1(self, n) -> bool:
        """AdaptiveAvgPool2d(1), F.adaptive_avg_pool2d(v, 1) or
        v.mean((2, 3), keepdim=True) of a 4-D value v"""
        import torch.fx as fx

        if not n.args or not isinstance(n.args[0], fx.Node):
            return False
        s = self.shape(n.args[0])
        if s is None or len(s) != 4:
            return False
        m = self.mod(n)
        if type(m) is nn.AdaptiveAvgPool2d:
            return _pair(m.output_size) == (1, 1)
        if n.op == "call_function" and n.target is F.adaptive_avg_pool2d:
            return _pair(self._arg(n, 1, "output_size", None)) == (1, 1)
        if ((n.op == "call_function" and n.target is torch.mean)
                or (n.op == "call_method" and n.target == "mean")):
            dim = self._arg(n, 1, "dim", None)
            return (isinstance(dim, (tuple, list))
                    and sorted(d % 4 for d in dim) == [2, 3]
                    and bool(self._arg(n, 2, "keepdim", False))
                    and n.kwargs.get("dtype") is None)
        return False

    def is_fc_conv(self, n, of) -> bool:
        """a 1x1 / stride 1 / no padding, ungrouped Conv2d of `of`"""
        m = self.mod(n)
        return (type(m) is nn.Conv2d and len(n.args) == 1
                and n.args[0] is of and _pair(m.kernel_size) == (1, 1)
                and _pair(m.stride) == (1, 1) and m.groups == 1
                and not isinstance(m.padding, str)
                and _pair(m.padding) == (0, 0)
                and _pair(m.dilation) == (1, 1))

    def is_mul_of(self, n, a, b) -> bool:
        if not self.is_mul(n):
            return False
        return (len(n.args) == 2 and not n.kwargs
                and (n.args == (a, b) or n.args == (b, a)))

    def is_mul(self, n) -> bool:
        return ((n.op == "call_function"
                 and n.target in (operator.mul, torch.mul))
                or (n.op == "call_method" and n.target == "mul"))

    def feeds_mul_with(self, n, v, depth=6) -> bool:
        """Some value made from `n` within `depth` nodes is multiplied with
        `v`: what tells a squeeze-excite from any other pooled branch (an
        image-pooling branch, a conv head after the global pool)."""
        if depth == 0:
            return False
        return any((self.is_mul(u) and v in u.args)
                   or self.feeds_mul_with(u, v, depth - 1) for u in n.users)

    def lower_squeeze_excite(self, n):
        """`n` pools a 4-D value v to 1x1. False when this is no
        squeeze-excite, that is when no 1x1 conv reads the pool or nothing
        made from it is multiplied with v (the caller goes on with the other
        patterns); None when the chain was lowered, else why it was not."""
        elsewhere = ("squeeze-excite: the output of {} is read by more than "
                     "the next node of the chain")
        v = n.args[0]
        if (not any(self.is_fc_conv(u, n) for u in n.users)
                or not self.feeds_mul_with(n, v)):
            return False
        c1 = self.sole_user(n)
        if c1 is None or not self.is_fc_conv(c1, n):
            return elsewhere.format(self._what(n))
        chain = [n, c1]
        u = self.sole_user(c1)
        if u is None:
            return elsewhere.format("the first conv")
        act = "none"
        if self.is_relu(u, c1):
            act = "relu"
            chain.append(u)
            c2 = self.sole_user(u)
            if c2 is None:
                return elsewhere.format("the ReLU")
        else:
            c2 = u
        if not self.is_fc_conv(c2, chain[-1]):
            return (f"squeeze-excite with {self._what(c2)} after its first "
                    "conv: squeeze_excite takes a ReLU or nothing there")
        chain.append(c2)
        gate = self.sole_user(c2)
        if gate is None:
            return elsewhere.format("the second conv")
        if not (gate.args and gate.args[0] is c2
                and (type(self.mod(gate)) is nn.Hardsigmoid
                     or (gate.op == "call_function"
                         and gate.target is F.hardsigmoid))):
            return (f"squeeze-excite with the gate {self._what(gate)}: "
                    "squeeze_excite has the hardsigmoid gate only")
        chain.append(gate)
        mul = self.sole_user(gate)
        if mul is None:
            return elsewhere.format("the gate")
        if not self.is_mul_of(mul, gate, v):
            return ("squeeze-excite whose gate is not multiplied with the "
                    "pooled value")
        chain.append(mul)
        m1, m2 = self.mod(c1), self.mod(c2)
        c, cr = m1.in_channels, m1.out_channels
        if (m2.in_channels, m2.out_channels) != (cr, c):
            return (f"squeeze-excite convs {c} -> {cr} and "
                    f"{m2.in_channels} -> {m2.out_channels} do not pair up")
        if c % _VEC:
            return (f"squeeze-excite on C={c}: squeeze_excite needs "
                    f"C % {_VEC} == 0")
        layer = L.SqueezeExcite(c, cr, act=act, gate="hardsigmoid")
        for w, b, m in (("w1", "b1", m1), ("w2", "b2", m2)):
            setattr(layer, w, nn.Parameter(   # [Cout, Cin, 1, 1] -> 2-D
                m.weight.detach().float().reshape(
                    m.out_channels, m.in_channels).clone()))
            if m.bias is not None:
                setattr(layer, b, nn.Parameter(
                    m.bias.detach().float().clone()))
        self.emit(mul, layer, [self.use(v, NHWC)], NHWC, chain)
        return None

    def lower_pool(self, n) -> Optional[str]:
        m = self.mod(n)
        kind = type(m).__name__
        s = self.shape(n.args[0])
        if s is None or len(s) != 4:
            return f"{kind} on a value that is not 4-D"
        k = _square(m.kernel_size)
        st = _square(m.kernel_size if m.stride is None else m.stride)
        pad = _square(m.padding)
        if k is None or st is None or pad is None:
            return f"{kind} that is not square"
        if m.ceil_mode:
            return f"{kind} with ceil_mode=True"
        if isinstance(m, nn.MaxPool2d):
            if _pair(m.dilation) != (1, 1) or m.return_indices:
                return "MaxPool2d with dilation or return_indices"
            layer = L.MaxPool(k, st, pad)
        else:
            if pad != 0 and m.count_include_pad:
                return ("padded AvgPool2d with count_include_pad=True: the "
                        "HIP kernel counts valid taps only")
            if m.divisor_override is not None:
                return "AvgPool2d with divisor_override"
            layer = L.AvgPool(k, st, pad)
        if s[1] % _VEC:
            return f"{kind} on C={s[1]}: the pools need C % {_VEC} == 0"
        self.emit(n, layer, [self.use(n.args[0], NHWC)], NHWC, [n])
        return None

    def lower_gap(self, n, chain) -> Optional[str]:
        """chain: [AdaptiveAvgPool2d(1), flatten] or [mean(dim=(2, 3))]"""
        s = self.shape(n.args[0])
        if s[1] % _VEC:
            return (f"global average pool on C={s[1]}: global_avg_pool "
                    f"needs C % {_VEC} == 0")
        self.emit(chain[-1], L.GlobalAvgPool(), [self.use(n.args[0], NHWC)],
                  None, chain)
        return None

    def lower_adaptive(self, n) -> Optional[str]:
        """nn.AdaptiveAvgPool2d(1) or F.adaptive_avg_pool2d(x, 1)"""
        import torch.fx as fx

        m = self.mod(n)
        size = (m.output_size if m is not None
                else self._arg(n, 1, "output_size", None))
        if not n.args or not isinstance(n.args[0], fx.Node):
            return "adaptive_avg_pool2d of something other than a tensor"
        s = self.shape(n.args[0])
        if s is None or len(s) != 4 or _pair(size) != (1, 1):
            return "AdaptiveAvgPool2d other than a 4-D value to 1x1"
        u = self.sole_user(n)
        if u is None or not self.is_flatten1(u, n):
            return "AdaptiveAvgPool2d(1) that is not followed by a flatten"
        return self.lower_gap(n, [n, u])

    def lower_mean(self, n) -> Optional[str]:
        import torch.fx as fx

        if not n.args or not isinstance(n.args[0], fx.Node):
            return "mean of something other than a tensor"
        s = self.shape(n.args[0])
        dim = n.args[1] if len(n.args) > 1 else n.kwargs.get("dim")
        keep = n.args[2] if len(n.args) > 2 else n.kwargs.get("keepdim",
                                                             False)
        if (s is None or len(s) != 4 or keep
                or not isinstance(dim, (tuple, list))
                or sorted(d % 4 for d in dim) != [2, 3]
                or n.kwargs.get("dtype") is not None):
            return "mean other than over dims (2, 3) of a 4-D value"
        return self.lower_gap(n, [n])

    def lower_cat(self, n) -> Optional[str]:
        import torch.fx as fx

        xs = n.args[0] if n.args else n.kwargs.get("tensors")
        dim = n.args[1] if len(n.args) > 1 else n.kwargs.get("dim", 0)
        if (not isinstance(xs, (tuple, list)) or not xs
                or not all(isinstance(a, fx.Node) and self.rank(a) == 4
                           for a in xs) or dim not in (1, -3)):
            return "cat other than of 4-D values over dim 1"
        self.emit(n, L.Concat(), [self.use(a, NHWC) for a in xs], NHWC, [n])
        return None

    def lower_flatten(self, n) -> Optional[str]:
        src = n.args[0]
        s = self.shape(src)
        if s is None or len(s) != 4:
            return "flatten of a value that is not 4-D"
        users = self.real_users(n)
        for u in users:
            if not (type(self.mod(u)) is nn.Linear and len(u.args) == 1):
                return ("flatten of a 4-D value that feeds something other "
                        "than Linear layers")
            why = self.linear_reason(u)
            if why is not None:
                return "flatten into a Linear that stays torch code: " + why
        self.emit(n, L.Flatten(), [self.use(src, NHWC)], None, [n])
        self.flat_chw[n] = tuple(s[1:])
        return None

    def lower_linear(self, n) -> Optional[str]:
        m = self.mod(n)
        why = self.linear_reason(n)
        if why is not None:
            return why
        chain, last = [n], n
        # Dense applies its ReLU with ops.relu on the [M, N] output, which
        # has that op's own rule; otherwise the ReLU is left to lower_relu
        r = self.relu_after(n)
        if r is not None and (self.shape(n)[0] * m.out_features) % _VEC:
            r = None
        if r is not None:
            chain.append(r)
            last = r
        layer = L.Dense(m.in_features, m.out_features,
                        bias=m.bias is not None,
                        act="relu" if r is not None else "none")
        w = m.weight.detach().float()
        chw = self.flat_chw.get(n.args[0])
        if chw is not None and chw[1] * chw[2] > 1:
            # the torch model flattened (c, h, w), Flatten gives (h, w, c)
            w = w.reshape(w.shape[0], *chw).permute(0, 2, 3, 1)
            w = w.reshape(w.shape[0], -1)
        layer.weight = nn.Parameter(w.contiguous().clone())
        if m.bias is not None:
            layer.bias = nn.Parameter(m.bias.detach().float().clone())
        self.emit(last, layer, [self.use(n.args[0], None)], None, chain)
        return None

    def lower_softmax(self, n) -> Optional[str]:
        s = self.shape(n.args[0]) if n.args else None
        m = self.mod(n)
        if m is not None:
            dim = m.dim
        else:
            dim = n.args[1] if len(n.args) > 1 else n.kwargs.get("dim")
            if len(n.args) > 2 or n.kwargs.get("dtype") is not None:
                dim = None
        if s is None or len(s) != 2 or dim not in (1, -1):
            return "softmax other than over the last dim of a 2-D value"
        self.emit(n, L.Softmax(), [self.use(n.args[0], None)], None, [n])
        return None

    # ---------------------------------------------------------------- main
    def try_lower(self, n) -> Optional[str]:
        """None when `n` (and what it fuses with) was lowered, else why
        it stays an island."""
        m = self.mod(n)
        if self.is_pool_to_1x1(n):
            why = self.lower_squeeze_excite(n)
            if why is not False:
                return why
        if m is not None:
            if type(m) is nn.Conv2d:
                return self.lower_conv(n)
            if type(m) is nn.BatchNorm2d:
                return self.lower_bn(n)
            if type(m) in (nn.MaxPool2d, nn.AvgPool2d):
                return self.lower_pool(n)
            if type(m) is nn.AdaptiveAvgPool2d:
                return self.lower_adaptive(n)
            if type(m) is nn.Linear:
                return self.lower_linear(n)
            if type(m) is nn.Softmax:
                return self.lower_softmax(n)
        elif n.op == "call_function":
            if n.target in (operator.add, operator.iadd, torch.add):
                return self.lower_add(n)
            if n.target is torch.cat:
                return self.lower_cat(n)
            if n.target is torch.mean:
                return self.lower_mean(n)
            if n.target in (F.softmax, torch.softmax):
                return self.lower_softmax(n)
            if n.target is F.adaptive_avg_pool2d:
                return self.lower_adaptive(n)
        elif n.op == "call_method":
            if n.target == "mean":
                return self.lower_mean(n)
            if n.target == "softmax":
                return self.lower_softmax(n)
        if n.args and self.is_relu(n, n.args[0]):
            return self.lower_relu(n)
        if n.args and self.is_relu6(n, n.args[0]):
            return self.lower_relu6(n)
        if n.args and self.is_hardswish(n, n.args[0]):
            return self.lower_hardswish(n)
        if n.args and self.is_flatten1(n, n.args[0]):
            return self.lower_flatten(n)
        return f"no lowering for {self._what(n)}"

    def island(self, n, reason: str):
        layer, refs = fx_call_layer(n, self.modules)
        ins = [self.use(self.by_fx_name[r], NCHW) for r in refs]
        self.emit(n, L.TorchIsland(layer, reason), ins,
                  NCHW if self.rank(n) == 4 else None, [n])
        self.rebind_mutated(n)

    def run(self) -> LayerGraph:
        import torch.fx as fx

        seen_input = False
        for n in self.g.nodes:
            if n.op == "placeholder":
                if seen_input:
                    raise ValueError("only single-input models are supported")
                seen_input = True
                self.vals[n] = {NCHW if self.rank(n) == 4 else None:
                                LayerGraph.INPUT}
            elif n.op == "get_attr":
                raise ValueError("get_attr nodes not supported; wrap "
                                 "constants in a module")
            elif n.op == "output":
                out = n.args[0]
                if not isinstance(out, fx.Node):
                    raise ValueError("only single-output models are "
                                     "supported")
                return LayerGraph(self.nodes, output=self.use(out, NCHW))
            elif n in self.done:
                continue
            elif self.removable(n):
                src = n.args[0]
                self.vals[n] = self.vals[src]
                if src in self.flat_chw:
                    self.flat_chw[n] = self.flat_chw[src]
            else:
                why = self.try_lower(n)
                if why is not None:
                    self.island(n, why)
        raise ValueError("graph had no output node")


def _bn_foldable(m: nn.BatchNorm2d) -> bool:
    return (not m.training and m.running_mean is not None
            and m.running_var is not None)


def _bn_fold(m: nn.BatchNorm2d):
    """(scale, shift) in float64: scale = gamma / sqrt(var + eps),
    shift = beta - mean * scale."""
    var = m.running_var.detach().double()
    mean = m.running_mean.detach().double()
    gamma = (m.weight.detach().double() if m.weight is not None
             else torch.ones_like(var))
    beta = (m.bias.detach().double() if m.bias is not None
            else torch.zeros_like(var))
    scale = gamma / torch.sqrt(var + m.eps)
    return scale, beta - mean * scale


def lowering_report(graph: LayerGraph) -> List[Tuple[str, str]]:
    """(node name, "lowered" or the reason the node stayed torch code) for
    every node of a lowered graph, in graph order."""
    return [(n.name, n.layer.reason if isinstance(n.layer, L.TorchIsland)
             else "lowered") for n in graph.nodes]


def lower_torch(model: nn.Module, input_shape,
                strict: bool = False) -> LayerGraph:
    """Lower a traceable single-input torch model (an `nn.Module`, which an
    `fx.GraphModule` is too) into a LayerGraph of defer_amd layers.

    `input_shape` is the model's own NCHW input shape; the shapes that
    decide legality are traced from it on the CPU, so the batch size given
    here should have the divisibility of the batch sizes that will run
    (numel rules of add_act and relu). The graph takes and returns what
    the model takes and returns. strict=True raises one ValueError listing
    every node that would stay torch code, with its reason."""
    if not isinstance(model, nn.Module):
        raise TypeError(f"cannot lower {type(model)!r}: expected an "
                        "nn.Module or fx.GraphModule")
    if model.training:
        raise ValueError(
            "lower_torch folds BatchNorm statistics and drops Dropout: "
            "call model.eval() first (inference only)")
    graph = _Lowering(model, tuple(input_shape)).run()
    if strict:
        kept = [(n, r) for n, r in lowering_report(graph) if r != "lowered"]
        if kept:
            raise ValueError(
                "lower_torch(strict=True): these nodes stay torch code: "
                + "; ".join(f"{n}: {r}" for n, r in kept))
    return graph
