"""Small plain-torch (NCHW) nets for the lowering tests, written the way
users and torchvision write them. A helper module, not a conftest."""

import copy

import torch
import torch.nn as nn


class Bottleneck(nn.Module):
    """torchvision's Bottleneck: ONE self.relu called three times, an
    in-place `+=` for the skip and an optional conv-bn downsample."""

    def __init__(self, cin, mid, cout, downsample=False):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv2 = nn.Conv2d(mid, mid, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.conv3 = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if downsample:
            self.downsample = nn.Sequential(
                nn.Conv2d(cin, cout, 1, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


class TVBlock(nn.Module):
    """Stem conv-bn-relu-maxpool, two bottlenecks (the first with a
    downsample), AdaptiveAvgPool2d(1), torch.flatten, fc. Widths 8/16/32;
    meant for a 2x3x32x32 input."""

    def __init__(self, classes=16):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 16, 3, padding=1, bias=True)
        self.bn1 = nn.BatchNorm2d(16)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.block1 = Bottleneck(16, 8, 32, downsample=True)
        self.block2 = Bottleneck(32, 8, 32)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(32, classes)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.block2(self.block1(x))
        x = torch.flatten(self.avgpool(x), 1)
        return self.fc(x)


class VGGHead(nn.Module):
    """Two conv-relu, maxpool, nn.Flatten over 8x4x4 (for a 2x3x8x8
    input), Linear-ReLU-Linear, softmax. The flatten order matters: the
    first Linear sees (c, h, w) columns in torch and (h, w, c) in NHWC."""

    def __init__(self, classes=8):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(8, 8, 3, padding=1), nn.ReLU(inplace=True),
            nn.MaxPool2d(2))
        self.flatten = nn.Flatten()
        self.classifier = nn.Sequential(
            nn.Linear(8 * 4 * 4, 16), nn.ReLU(inplace=True), nn.Dropout(),
            nn.Linear(16, classes))
        self.softmax = nn.Softmax(dim=1)

    def forward(self, x):
        return self.softmax(self.classifier(self.flatten(self.features(x))))


class CatNet(nn.Module):
    """The DenseNet-style net of test_defer_concat_dag_model (every block
    consumes the 3-channel input through torch.cat), with a head whose
    width the HIP linear takes."""

    def __init__(self):
        super().__init__()
        self.c1 = nn.Conv2d(3, 8, 3, padding=1)
        self.c2 = nn.Conv2d(11, 8, 3, padding=1)    # cat(x, f1)
        self.c3 = nn.Conv2d(19, 8, 3, padding=1)    # cat(x, f1, f2)
        self.head = nn.Linear(8, 8)

    def forward(self, x):
        f1 = torch.relu(self.c1(x))
        f2 = torch.relu(self.c2(torch.cat([x, f1], dim=1)))
        f3 = torch.relu(self.c3(torch.cat([x, f1, f2], dim=1)))
        return self.head(f3.mean(dim=(2, 3)))


class IslandNet(nn.Module):
    """conv-relu, a grouped conv and a Sigmoid (neither has a HIP op),
    conv-relu, mean, fc."""

    def __init__(self):
        super().__init__()
        self.c1 = nn.Conv2d(3, 8, 3, padding=1)
        self.grouped = nn.Conv2d(8, 8, 3, padding=1, groups=2)
        self.sig = nn.Sigmoid()
        self.c2 = nn.Conv2d(8, 16, 3, padding=1)
        self.fc = nn.Linear(16, 8)

    def forward(self, x):
        x = torch.relu(self.c1(x))
        x = self.sig(self.grouped(x))
        x = torch.relu(self.c2(x))
        return self.fc(x.mean(dim=(2, 3)))


class TwelveNet(nn.Module):
    """A 12-channel conv (legal: Cout % 4) into a max-pool (illegal: the
    pools need C % 8)."""

    def __init__(self):
        super().__init__()
        self.c1 = nn.Conv2d(3, 12, 3, padding=1)
        self.pool = nn.MaxPool2d(2)
        self.c2 = nn.Conv2d(12, 8, 3, padding=1)
        self.fc = nn.Linear(8, 8)

    def forward(self, x):
        x = self.pool(torch.relu(self.c1(x)))
        x = torch.relu(self.c2(x))
        return self.fc(x.mean(dim=(2, 3)))


class AvgPoolNet(nn.Module):
    """conv-relu, a padded 3x3/s2 AvgPool2d, mean, fc."""

    def __init__(self, count_include_pad):
        super().__init__()
        self.c1 = nn.Conv2d(3, 8, 3, padding=1)
        self.pool = nn.AvgPool2d(3, stride=2, padding=1,
                                 count_include_pad=count_include_pad)
        self.fc = nn.Linear(8, 8)

    def forward(self, x):
        x = self.pool(torch.relu(self.c1(x)))
        return self.fc(x.mean(dim=(2, 3)))


def randomize_bn(model, gen):
    """Non-trivial running statistics and affine terms for every BN."""
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            c = m.num_features
            m.running_mean.copy_(torch.randn(c, generator=gen) * 0.5)
            m.running_var.copy_(torch.rand(c, generator=gen) + 0.5)
            m.weight.data.copy_(torch.rand(c, generator=gen) + 0.5)
            m.bias.data.copy_(torch.randn(c, generator=gen) * 0.5)
    return model


def integerize(model, seed=0):
    """Small-integer parameters under which every product and sum of the
    forward pass is an integer far below 2^24, so fp32 arithmetic is exact
    in any summation order.

    Weights are -1 / 0 / +1 with about three non-zeros per output, biases
    0..2 (positive, to keep the ReLUs alive). BN: running_var + eps = 4
    exactly (torch rejects eps = 0, so eps = 1 and running_var = 3),
    integer mean and beta, gamma 2 or 4, so the folded scale gamma / 2 is
    1 or 2."""
    gen = torch.Generator().manual_seed(seed)

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=gen).float()

    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                fan_in = m.weight[0].numel()
                keep = torch.rand(m.weight.shape, generator=gen) \
                    < min(1.0, 3.0 / fan_in)
                m.weight.copy_(ints(m.weight.shape, 0, 1) * 2 - 1)
                m.weight.mul_(keep)
                if m.bias is not None:
                    m.bias.copy_(ints(m.bias.shape, 0, 2))
            elif isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.eps = 1.0
                m.running_var.fill_(3.0)
                m.running_mean.copy_(ints((c,), -1, 1))
                m.bias.copy_(ints((c,), 0, 2))
                m.weight.copy_(ints((c,), 1, 2) * 2)
    return model


def int_input(shape, seed=0):
    gen = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(-2, 3, shape, generator=gen).float()


def as_double(model):
    return copy.deepcopy(model).double()
