"""A small plain-torch (NCHW) MobileNetV3, written the way torchvision
writes it, and one-block nets for every spelling of hardswish and of the
squeeze-excite chain, for the lowering tests. A helper module, not a
conftest."""

import torch
import torch.nn as nn
import torch.nn.functional as F


class SqueezeExcitation(nn.Module):
    """torchvision.ops.misc.SqueezeExcitation: 1x1 convs with bias as the
    two FCs, `scale * input` at the end."""

    def __init__(self, input_channels, squeeze_channels, activation=nn.ReLU,
                 scale_activation=nn.Hardsigmoid):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(input_channels, squeeze_channels, 1)
        self.fc2 = nn.Conv2d(squeeze_channels, input_channels, 1)
        self.activation = activation()
        self.scale_activation = scale_activation()

    def _scale(self, input):
        scale = self.avgpool(input)
        scale = self.fc1(scale)
        scale = self.activation(scale)
        scale = self.fc2(scale)
        return self.scale_activation(scale)

    def forward(self, input):
        scale = self._scale(input)
        return scale * input


class Conv2dNormActivation(nn.Sequential):
    """torchvision's, with MobileNetV3's arguments: conv (no bias),
    BatchNorm2d and an in-place activation (None: no activation)."""

    def __init__(self, cin, cout, kernel_size=3, stride=1, groups=1,
                 activation_layer=nn.Hardswish):
        layers = [nn.Conv2d(cin, cout, kernel_size, stride,
                            (kernel_size - 1) // 2, groups=groups,
                            bias=False),
                  nn.BatchNorm2d(cout)]
        if activation_layer is not None:
            layers.append(activation_layer(inplace=True))
        super().__init__(*layers)


class InvertedResidual(nn.Module):
    """torchvision.models.mobilenetv3.InvertedResidual."""

    def __init__(self, inp, kernel, expanded, oup, use_se, use_hs, stride,
                 se_channels=8):
        super().__init__()
        self.use_res_connect = stride == 1 and inp == oup
        act = nn.Hardswish if use_hs else nn.ReLU
        layers = []
        if expanded != inp:
            layers.append(Conv2dNormActivation(inp, expanded, 1,
                                               activation_layer=act))
        layers.append(Conv2dNormActivation(expanded, expanded, kernel,
                                           stride, groups=expanded,
                                           activation_layer=act))
        if use_se:
            layers.append(SqueezeExcitation(expanded, se_channels))
        layers.append(Conv2dNormActivation(expanded, oup, 1,
                                           activation_layer=None))
        self.block = nn.Sequential(*layers)

    def forward(self, input):
        result = self.block(input)
        if self.use_res_connect:
            result += input
        return result


class TinyMobileNetV3(nn.Module):
    """A hardswish stem, three inverted residuals (ReLU with squeeze-excite
    and a 5x5 kernel at stride 2; hardswish with squeeze-excite and the
    identity add; hardswish without squeeze-excite), the last 1x1 conv and
    torchvision's head: avgpool, flatten, Linear, Hardswish, Dropout,
    Linear. Meant for a 2x3x32x32 input: both squeeze-excites pool 8x8."""

    def __init__(self, classes=8):
        super().__init__()
        self.features = nn.Sequential(
            Conv2dNormActivation(3, 8, stride=2),
            InvertedResidual(8, 5, 16, 16, True, False, 2),
            InvertedResidual(16, 3, 32, 16, True, True, 1, se_channels=6),
            InvertedResidual(16, 3, 24, 16, False, True, 1),
            Conv2dNormActivation(16, 32, kernel_size=1))
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(
            nn.Linear(32, 64), nn.Hardswish(inplace=True),
            nn.Dropout(0.2, inplace=True), nn.Linear(64, classes))

    def forward(self, x):
        x = self.features(x)
        x = self.avgpool(x)
        x = torch.flatten(x, 1)
        return self.classifier(x)


SE_BLOCKS = ((16, 8), (32, 6))      # (c, cr) of TinyMobileNetV3, in order


def integerize_v3(model, seed=0):
    """Integer parameters for TinyMobileNetV3 under which, for an input of
    multiples of 3 (int_input_v3), every hardswish argument is a multiple
    of 3 (so <= -3, 0 or >= 3: hardswish is exact there) and every gate
    argument is a multiple of 3 (so the hardsigmoid is exactly 0, 0.5 or 1).

    Conv and Linear weights are -1 / 0 / +1 with about two non-zeros per
    output, biases 0 or 3. BN: running_var + eps = 4 and gamma = 2, so the
    folded scale is 1; mean and beta are -3 / 0 / 3. Where the input of a
    layer is not a multiple of 3 the weights make up for it:
      - fc1 of a squeeze-excite reads means over 8x8, multiples of 3/64,
        and has weights of +-64; so has the Linear after the last pool;
      - the project conv after a squeeze-excite reads multiples of 3/2
        (gate 0.5) and has weights of +-2.
    In every fc2 channel 0 has weight 0 and bias 0 (gate 0.5 for sure),
    channel 1 bias 3 (gate 1) and channel 2 bias -3 (gate 0)."""
    gen = torch.Generator().manual_seed(seed)

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=gen).float()

    def sparse(m, nonzeros, mult=1.0):
        fan_in = m.weight[0].numel()
        keep = torch.rand(m.weight.shape, generator=gen) \
            < min(1.0, nonzeros / fan_in)
        m.weight.copy_((ints(m.weight.shape, 0, 1) * 2 - 1) * keep * mult)
        if m.bias is not None:
            m.bias.copy_(ints(m.bias.shape, 0, 1) * 3)

    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                sparse(m, 2.0)
            elif isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.eps = 1.0
                m.running_var.fill_(3.0)
                m.running_mean.copy_(ints((c,), -1, 1) * 3)
                m.bias.copy_(ints((c,), -1, 1) * 3)
                m.weight.fill_(2.0)
        for blk in model.modules():
            if isinstance(blk, InvertedResidual):
                mods = list(blk.block)
                for i, m in enumerate(mods):
                    if isinstance(m, SqueezeExcitation):
                        sparse(m.fc1, 2.0, 64.0)
                        m.fc2.weight[:3] = 0
                        m.fc2.bias[:3] = torch.tensor([0.0, 3.0, -3.0])
                        mods[i + 1][0].weight.mul_(2.0)
        sparse(model.classifier[0], 2.0, 64.0)
    return model


def int_input_v3(shape, seed=0):
    gen = torch.Generator().manual_seed(2000 + seed)
    return torch.randint(-1, 2, shape, generator=gen).float() * 3


class HardswishNet(nn.Module):
    """conv [-> BN] -> one hardswish spelling -> mean -> fc. `after_pool`
    puts a max-pool between the conv and the activation, so the activation
    cannot fuse into the conv; `depthwise` makes the conv before it a
    depthwise one."""

    def __init__(self, how, after_pool=False, depthwise=False, bn=False):
        super().__init__()
        self.how = how
        self.c0 = nn.Conv2d(3, 8, 3, padding=1) if depthwise else None
        self.conv = (nn.Conv2d(8, 8, 3, padding=1, groups=8) if depthwise
                     else nn.Conv2d(3, 8, 3, padding=1))
        self.bn = nn.BatchNorm2d(8) if bn else None
        self.pool = nn.MaxPool2d(2) if after_pool else None
        self.act = {"module": nn.Hardswish(),
                    "module_inplace": nn.Hardswish(inplace=True)}.get(how)
        self.fc = nn.Linear(8, 8)

    def forward(self, x):
        if self.c0 is not None:
            x = torch.relu(self.c0(x))
        x = self.conv(x)
        if self.bn is not None:
            x = self.bn(x)
        if self.pool is not None:
            x = self.pool(x)
        if self.act is not None:
            x = self.act(x)
        elif self.how == "functional":
            x = F.hardswish(x)
        elif self.how == "functional_inplace":
            x = F.hardswish(x, inplace=True)
        elif self.how == "functional_inplace_pos":
            x = F.hardswish(x, True)
        else:
            raise ValueError(self.how)
        return self.fc(x.mean(dim=(2, 3)))


HARDSWISH_SPELLINGS = ("module", "module_inplace", "functional",
                       "functional_inplace", "functional_inplace_pos")


class InplaceHardswishShared(nn.Module):
    """An in-place hardswish of a value that is read again afterwards: the
    later reader must see the activated value, as in torch."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 8, 3, padding=1)
        self.pool = nn.MaxPool2d(2)
        self.act = nn.Hardswish(inplace=True)
        self.fc = nn.Linear(8, 8)

    def forward(self, x):
        x = self.pool(self.conv(x))
        y = self.act(x)
        return self.fc((x + y).mean(dim=(2, 3)))


class SeNet(nn.Module):
    """conv-relu to `c` channels, one squeeze-excite written out with the
    chosen spellings, mean, fc.

    pool: "module" | "functional" | "mean"; mul: "scale_first" | "x_first"
    | "torch" | "method"; act: "relu" | "relu_inplace" | "none" | "silu";
    gate: "module" | "functional" | "sigmoid"; bias: on both convs or not;
    reuse: None, or the chain value ("pooled" | "hidden" | "gate") that is
    also added to the output, so it has a second reader."""

    def __init__(self, c=8, cr=4, pool="module", mul="scale_first",
                 act="relu", gate="module", bias=True, reuse=None):
        super().__init__()
        self.pool, self.mul, self.act, self.gate = pool, mul, act, gate
        self.reuse = reuse
        self.c1 = nn.Conv2d(3, c, 3, padding=1)
        self.avg = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(c, cr, 1, bias=bias)
        self.fc2 = nn.Conv2d(cr, c, 1, bias=bias)
        self.act1 = nn.ReLU(inplace=act == "relu_inplace")
        self.silu = nn.SiLU()
        self.hsig = nn.Hardsigmoid()
        self.fc = nn.Linear(c, 8)

    def forward(self, x):
        v = torch.relu(self.c1(x))
        if self.pool == "module":
            s = self.avg(v)
        elif self.pool == "functional":
            s = F.adaptive_avg_pool2d(v, 1)
        else:
            s = v.mean((2, 3), keepdim=True)
        z = self.fc1(s)
        if self.act in ("relu", "relu_inplace"):
            z = self.act1(z)
        elif self.act == "silu":
            z = self.silu(z)
        a = self.fc2(z)
        if self.gate == "module":
            g = self.hsig(a)
        elif self.gate == "functional":
            g = F.hardsigmoid(a)
        else:
            g = torch.sigmoid(a)
        if self.mul == "scale_first":
            y = g * v
        elif self.mul == "x_first":
            y = v * g
        elif self.mul == "torch":
            y = torch.mul(g, v)
        else:
            y = v.mul(g)
        y = y.mean(dim=(2, 3))
        if self.reuse is not None:
            extra = {"pooled": s, "hidden": None, "gate": g}[self.reuse]
            if extra is None:           # Cr != C: read z through its mean
                y = y + z.mean()
            else:
                y = y + extra.flatten(1)
        return self.fc(y)
