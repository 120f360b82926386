"""Layer modules for defer_amd models.

Each layer is a thin nn.Module over `defer_amd.ops` (HIP kernels on GPU,
fp32 PyTorch reference on CPU). These are the in-repo replacements for the
Keras layer zoo the reference executes via model.predict (node.py:106):
Conv2D/BatchNorm/ReLU -> ConvBNAct (BN folded at init), DepthwiseConv2D/
BatchNorm/ReLU6 -> DepthwiseConvBNAct, the squeeze-excite block of
MobileNetV3 -> SqueezeExcite, Add(+ReLU) ->
AddAct, MaxPooling2D -> MaxPool, GlobalAveragePooling2D -> GlobalAvgPool,
Dense -> Dense, softmax -> Softmax.

Activations are NHWC; conv weights are [Cout, R, S, Cin] (OHWI), chosen so
the implicit-GEMM K dimension (r, s, c) is contiguous per output channel:
the MFMA kernel's B^T fragment read is then a dense row read, and the
global->LDS staging of a [BN][BK] weight tile is fully coalesced.
"""

import math

import torch
import torch.nn as nn

from defer_amd import ops


class ConvBNAct(nn.Module):
    """Conv2d + folded inference BatchNorm + optional ReLU, ReLU6 or
    hardswish, fused.

    BN folding: y = conv(x) * scale + bias with scale = gamma/sqrt(var+eps),
    bias = beta - mean*scale. Random init keeps BN-ish statistics so
    activations stay O(1) through deep stacks (bench uses random-init
    weights per BASELINE.json).
    """

    def __init__(self, cin, cout, kernel=3, stride=1, padding=None,
                 act="relu", bn=True):
        super().__init__()
        self.cin, self.cout = cin, cout
        self.kernel, self.stride = kernel, stride
        self.padding = (kernel // 2) if padding is None else padding
        self.act = act
        fan_in = cin * kernel * kernel
        w = torch.randn(cout, kernel, kernel, cin) * math.sqrt(2.0 / fan_in)
        self.weight = nn.Parameter(w)
        self.scale = nn.Parameter(torch.ones(cout)) if bn else None
        self.bias = nn.Parameter(torch.zeros(cout))

    def forward(self, x, residual=None):
        return ops.conv2d_bn_act(
            x, self.weight.to(x.dtype), self.scale, self.bias,
            stride=self.stride, padding=self.padding, act=self.act,
            residual=residual)

    def extra_repr(self):
        return (f"{self.cin}->{self.cout} k{self.kernel} s{self.stride} "
                f"p{self.padding} act={self.act}")

    def flops_per_pixel(self):
        return 2 * self.kernel * self.kernel * self.cin * self.cout


class DepthwiseConvBNAct(nn.Module):
    """Depthwise Conv2d (one filter per channel) + folded inference
    BatchNorm + optional ReLU / ReLU6, fused: the 3x3 layer between the
    expand and project 1x1 convs of a MobileNetV2 block. The weight is
    [R, S, C], channels last like the activation, and has 3 dims, so
    StageExecutor casts it to the compute dtype with the conv weights."""

    def __init__(self, c, kernel=3, stride=1, padding=None, act="relu6",
                 bn=True):
        super().__init__()
        self.c = c
        self.kernel, self.stride = kernel, stride
        self.padding = (kernel // 2) if padding is None else padding
        self.act = act
        w = torch.randn(kernel, kernel, c) * math.sqrt(2.0 / (kernel * kernel))
        self.weight = nn.Parameter(w)
        self.scale = nn.Parameter(torch.ones(c)) if bn else None
        self.bias = nn.Parameter(torch.zeros(c))

    def forward(self, x):
        return ops.dwconv2d_bn_act(
            x, self.weight.to(x.dtype), self.scale, self.bias,
            stride=self.stride, padding=self.padding, act=self.act)

    def extra_repr(self):
        return (f"depthwise {self.c} k{self.kernel} s{self.stride} "
                f"p{self.padding} act={self.act}")

    def flops_per_pixel(self):
        return 2 * self.kernel * self.kernel * self.c


class SqueezeExcite(nn.Module):
    """Squeeze-excite: x * gate(fc2(act(fc1(mean over H, W of x)))), one
    graph node with one input (ops.squeeze_excite; csrc/se.hip on the GPU).
    fc1 is c -> cr and fc2 cr -> c, the 1x1 convs of the torch and Keras
    blocks. Both weights are 2-D, so StageExecutor casts them to the compute
    dtype with the conv weights; the biases are 1-D and stay fp32."""

    def __init__(self, c, cr, act="relu", gate="hardsigmoid"):
        super().__init__()
        ops._act_code(act, ops._RELU_OR_NONE)
        if gate not in ops._SE_GATES:
            raise ValueError(
                f"gate={gate!r}: expected one of {list(ops._SE_GATES)}")
        self.c, self.cr = c, cr
        self.act, self.gate = act, gate
        self.w1 = nn.Parameter(torch.randn(cr, c) * math.sqrt(2.0 / c))
        self.b1 = nn.Parameter(torch.zeros(cr))
        self.w2 = nn.Parameter(torch.randn(c, cr) * math.sqrt(1.0 / cr))
        self.b2 = nn.Parameter(torch.zeros(c))

    def forward(self, x):
        return ops.squeeze_excite(
            x, self.w1.to(x.dtype), self.b1, self.w2.to(x.dtype), self.b2,
            act=self.act, gate=self.gate)

    def extra_repr(self):
        return (f"squeeze_excite={self.c}->{self.cr}->{self.c} "
                f"act={self.act} gate={self.gate}")

    def flops_per_image(self):
        """The two FCs; the pool and the scale are passes over the tensor,
        which the partitioner costs by their bytes."""
        return 4 * self.c * self.cr


class AddAct(nn.Module):
    """Residual add + activation — the reference's `add_N` cut layers
    (test/test.py:18) with the ReLU that follows them fused in."""

    def __init__(self, act="relu"):
        super().__init__()
        self.act = act

    def forward(self, a, b):
        return ops.add_act(a, b, act=self.act)


class MaxPool(nn.Module):
    def __init__(self, kernel=3, stride=2, padding=1):
        super().__init__()
        self.kernel, self.stride, self.padding = kernel, stride, padding

    def forward(self, x):
        return ops.maxpool2d(x, self.kernel, self.stride, self.padding)


class AvgPool(nn.Module):
    """Average pooling (DenseNet transition 2x2/2)."""

    def __init__(self, kernel=2, stride=2, padding=0):
        super().__init__()
        self.kernel, self.stride, self.padding = kernel, stride, padding

    def forward(self, x):
        return ops.avgpool2d(x, self.kernel, self.stride, self.padding)


class Concat(nn.Module):
    """Channel concat of NHWC inputs (DenseNet dense connections).
    GPU path is strided device copies, no torch compute kernels."""

    def forward(self, *xs):
        return ops.concat_channels(xs)


class BNActConv(nn.Module):
    """Pre-activation composite BN -> ReLU -> Conv (DenseNet layer
    ordering; torchvision DenseLayer norm/relu/conv). Inference BN is a
    folded per-channel scale/bias applied by the standalone bn_act HIP
    kernel; the conv runs without epilogue BN."""

    def __init__(self, cin, cout, kernel=1, stride=1, padding=0,
                 out_bn=False):
        super().__init__()
        self.cin, self.cout = cin, cout
        self.kernel, self.stride, self.padding = kernel, stride, padding
        fan_in = cin * kernel * kernel
        w = torch.randn(cout, kernel, kernel, cin) \
            * math.sqrt(2.0 / fan_in)
        self.weight = nn.Parameter(w)
        self.scale = nn.Parameter(torch.ones(cin))
        self.bias = nn.Parameter(torch.zeros(cin))
        # out_bn: this layer ALSO owns the next composite's folded
        # BN-ReLU, applied to the conv output (DenseNet norm2 folds
        # into c1's epilogue; conv2 then runs as a plain 3x3)
        self.out_bn = out_bn
        if out_bn:
            self.out_scale = nn.Parameter(torch.ones(cout))
            self.out_bias = nn.Parameter(torch.zeros(cout))

    def forward(self, x):
        if self.kernel == 1 and self.stride == 1 and self.padding == 0:
            # fused single-pass path (the standalone bn_act round-trips
            # were 57% of the DenseNet step before fusion)
            return ops.conv1x1_prebn(
                x, self.weight.to(x.dtype),
                self.scale.float(), self.bias.float(),
                self.out_scale.float() if self.out_bn else None,
                self.out_bias.float() if self.out_bn else None)
        z = ops.batchnorm_apply(x, self.scale, self.bias, act="relu")
        y = ops.conv2d_bn_act(z, self.weight.to(x.dtype), None, None,
                              stride=self.stride,
                              padding=self.padding, act="none")
        if self.out_bn:
            y = ops.batchnorm_apply(y, self.out_scale, self.out_bias,
                                    act="relu")
        return y

    def extra_repr(self):
        return (f"bn-relu-conv {self.cin}->{self.cout} k{self.kernel} "
                f"s{self.stride} p{self.padding}")

    def flops_per_pixel(self):
        return 2 * self.kernel * self.kernel * self.cin * self.cout


class BNAct(nn.Module):
    """Standalone folded-BN + activation (DenseNet final norm5)."""

    def __init__(self, c, act="relu"):
        super().__init__()
        self.act = act
        self.scale = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))

    def forward(self, x):
        return ops.batchnorm_apply(x, self.scale, self.bias, self.act)


class GlobalAvgPool(nn.Module):
    def forward(self, x):
        return ops.global_avg_pool(x)


class Flatten(nn.Module):
    """NHWC -> (N, H*W*C). Matches Keras Flatten under channels_last
    (the reference's VGG19 head flattens 7x7x512 -> 25088); a reshape of
    a contiguous NHWC tensor, so free on GPU."""

    def forward(self, x):
        return x.reshape(x.shape[0], -1)


class Dense(nn.Module):
    def __init__(self, cin, cout, bias=True, act="none"):
        super().__init__()
        ops._act_code(act, ops._RELU_OR_NONE)
        self.cin, self.cout = cin, cout
        self.act = act
        self.weight = nn.Parameter(
            torch.randn(cout, cin) * math.sqrt(1.0 / cin))
        self.bias = nn.Parameter(torch.zeros(cout)) if bias else None

    def forward(self, x):
        y = ops.linear(x, self.weight.to(x.dtype), self.bias)
        if self.act == "relu":
            y = ops.relu(y)
        return y


class Softmax(nn.Module):
    def forward(self, x):
        return ops.softmax(x)


class Relu(nn.Module):
    """A ReLU that no conv, BN, add or dense layer could take in."""

    def forward(self, x):
        return ops.relu(x)


class Relu6(nn.Module):
    """A ReLU6 that no conv or depthwise conv could take in."""

    def forward(self, x):
        return ops.relu6(x)


class Hardswish(nn.Module):
    """A hardswish that no conv or depthwise conv could take in."""

    def forward(self, x):
        return ops.hardswish(x)


class ToNHWC(nn.Module):
    """NCHW -> NHWC at the border of a lowered torch model: its input, and
    the output of a layer that stayed torch code (defer_amd.lower)."""

    def forward(self, x):
        return ops.to_nhwc(x.contiguous())


class ToNCHW(nn.Module):
    """NHWC -> NCHW: the inverse border, into torch code or out of the
    model, so the user gets the tensor their model would have given."""

    def forward(self, x):
        return ops.to_nchw(x.contiguous())


class TorchIsland(nn.Module):
    """A piece of a torch model that was not lowered and runs as torch
    code, in NCHW, among defer_amd layers. `inner` is the leaf module or
    the function layer `from_torch` would have built; `reason` says why it
    stayed. StageExecutor casts matrices to the compute dtype and vectors
    to fp32, which a plain torch module (bf16 weight, fp32 bias) rejects:
    a module island therefore follows its input, casting its own floating
    parameters and buffers to the incoming dtype when that changes."""

    def __init__(self, inner, reason=""):
        super().__init__()
        if isinstance(inner, nn.Module):
            self.inner = inner
        else:
            self.inner = None
            self._fn = inner
        self.reason = reason
        self._dtype = None

    def forward(self, *args):
        if self.inner is None:
            return self._fn(*args)
        dt = next((a.dtype for a in args if torch.is_tensor(a)
                   and a.is_floating_point()), None)
        if dt is not None and dt != self._dtype:
            self.inner.to(dt)
            self._dtype = dt
        return self.inner(*args)

    def extra_repr(self):
        return f"kept: {self.reason}"
