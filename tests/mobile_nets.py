"""A small plain-torch (NCHW) MobileNetV2, written the way torchvision
writes it, for the lowering tests. A helper module, not a conftest."""

import torch
import torch.nn as nn
import torch.nn.functional as F


class Conv2dNormActivation(nn.Sequential):
    """torchvision.ops.misc.Conv2dNormActivation with its MobileNetV2
    arguments: conv (no bias), BatchNorm2d, ReLU6(inplace=True)."""

    def __init__(self, cin, cout, kernel_size=3, stride=1, groups=1):
        super().__init__(
            nn.Conv2d(cin, cout, kernel_size, stride, (kernel_size - 1) // 2,
                      groups=groups, bias=False),
            nn.BatchNorm2d(cout),
            nn.ReLU6(inplace=True))


class InvertedResidual(nn.Module):
    """torchvision.models.mobilenetv2.InvertedResidual."""

    def __init__(self, inp, oup, stride, expand_ratio):
        super().__init__()
        hidden = inp * expand_ratio
        self.use_res_connect = stride == 1 and inp == oup
        layers = []
        if expand_ratio != 1:
            layers.append(Conv2dNormActivation(inp, hidden, kernel_size=1))
        layers.extend([
            Conv2dNormActivation(hidden, hidden, stride=stride,
                                 groups=hidden),
            nn.Conv2d(hidden, oup, 1, 1, 0, bias=False),
            nn.BatchNorm2d(oup)])
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        if self.use_res_connect:
            return x + self.conv(x)
        return self.conv(x)


class TinyMobileNetV2(nn.Module):
    """Stem, three inverted residuals of widths 8 / 16 (one without an
    expand conv, one with stride 2, one with the identity add), the last
    1x1 conv, and torchvision's head: F.adaptive_avg_pool2d, torch.flatten,
    Dropout, Linear. Meant for a 2x3x32x32 input."""

    def __init__(self, classes=8):
        super().__init__()
        self.features = nn.Sequential(
            Conv2dNormActivation(3, 8, stride=2),
            InvertedResidual(8, 16, 1, 1),       # t = 1: no expand, no add
            InvertedResidual(16, 16, 2, 2),      # stride 2
            InvertedResidual(16, 16, 1, 2),      # identity add
            Conv2dNormActivation(16, 32, kernel_size=1))
        self.classifier = nn.Sequential(nn.Dropout(0.2),
                                        nn.Linear(32, classes))

    def forward(self, x):
        x = self.features(x)
        x = F.adaptive_avg_pool2d(x, (1, 1))
        x = torch.flatten(x, 1)
        return self.classifier(x)


class Relu6Net(nn.Module):
    """conv -> one ReLU6 spelling -> mean -> fc. `how` picks the spelling;
    `after_pool` puts a max-pool between the conv and the activation, so
    the activation cannot fuse into the conv."""

    def __init__(self, how, after_pool=False):
        super().__init__()
        self.how = how
        self.conv = nn.Conv2d(3, 8, 3, padding=1)
        self.pool = nn.MaxPool2d(2) if after_pool else None
        self.act = {"module": nn.ReLU6(), "module_inplace": nn.ReLU6(True),
                    "hardtanh": nn.Hardtanh(0., 6.)}.get(how)
        self.fc = nn.Linear(8, 8)

    def forward(self, x):
        x = self.conv(x)
        if self.pool is not None:
            x = self.pool(x)
        if self.act is not None:
            x = self.act(x)
        elif self.how == "functional":
            x = F.relu6(x)
        elif self.how == "functional_inplace":
            x = F.relu6(x, inplace=True)
        elif self.how == "f_hardtanh":
            x = F.hardtanh(x, 0., 6.)
        elif self.how == "f_hardtanh_kw":
            x = F.hardtanh(x, min_val=0., max_val=6.)
        else:
            raise ValueError(self.how)
        return self.fc(x.mean(dim=(2, 3)))


RELU6_SPELLINGS = ("module", "module_inplace", "hardtanh", "functional",
                   "functional_inplace", "f_hardtanh", "f_hardtanh_kw")


class DepthwiseNet(nn.Module):
    """conv-relu to `c` channels, one depthwise-style conv given by
    **conv_kw (groups = c), mean, fc."""

    def __init__(self, c=8, cout=None, **conv_kw):
        super().__init__()
        cout = c if cout is None else cout
        self.c1 = nn.Conv2d(3, c, 3, padding=1)
        self.dw = nn.Conv2d(c, cout, groups=c, **conv_kw)
        self.fc = nn.Linear(cout, 8)

    def forward(self, x):
        x = torch.relu(self.c1(x))
        x = F.relu6(self.dw(x))
        return self.fc(x.mean(dim=(2, 3)))
