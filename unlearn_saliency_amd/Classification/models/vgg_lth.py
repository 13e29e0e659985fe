"""VGG-16 with BatchNorm and the one-layer head of the lottery-ticket code base, state_dict-compatible with the
reference (Classification/models/VGG_LTH.py:46-94, 209-217).

The module tree is the reference's: `features` is one nn.Sequential of Conv2d(bias=True) / BatchNorm2d / ReLU /
MaxPool2d entries at the same indices, then `avgpool`, `classifier` and `normalize` — so `named_parameters()` yields the
same 54 names / shapes / order (the flat index the saliency ranking runs over) and `state_dict()` the same keys.
Only configuration "D" is registered (`vgg16_bn_lth`); the constructor takes any configuration list, and the
classifier reads as many channels as the last convolution writes.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .resnet_cifar import CIFAR10_MEAN, CIFAR10_STD, NormalizeByChannelMeanStd

CFG_D = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512)


def make_layers(cfg) -> nn.Sequential:
    layers, cin = [], 3
    for v in cfg:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.BatchNorm2d(v), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers)


class VGG(nn.Module):
    def __init__(self, cfg=CFG_D, num_classes: int = 10, init_weights: bool = True):
        super().__init__()
        widths = [v for v in cfg if v != "M"]
        if not widths:
            raise ValueError("VGG: the configuration holds no convolution")
        self.features = make_layers(cfg)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.classifier = nn.Linear(widths[-1], num_classes)
        self.normalize = NormalizeByChannelMeanStd(CIFAR10_MEAN, CIFAR10_STD)
        if init_weights:
            self._initialize_weights()

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.constant_(m.bias, 0)

    fused_bn = False    # set by unlearn_saliency_amd.norm.use_fused_bn
    fused_head = False  # set by unlearn_saliency_amd.cls_head.use_fused_head
    own_pool = True     # with fused_bn: MaxPool2d entries on K24 (False: the library's pooling; an A/B switch of tests)

    def _fused_features(self, x):
        """`features` with every (Conv2d, BatchNorm2d, ReLU) triple as conv -> one fused BN+ReLU node and every
        MaxPool2d(2, 2) on K24; any other entry runs as the module it is."""
        from ...norm import fused_bn_act
        from ...pool import maxpool2x2
        mods = list(self.features)
        i = 0
        while i < len(mods):
            m = mods[i]
            if (isinstance(m, nn.Conv2d) and i + 2 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm2d)
                    and isinstance(mods[i + 2], nn.ReLU)):
                x = fused_bn_act(m(x), mods[i + 1], relu=True)
                i += 3
                continue
            if (self.own_pool and type(m) is nn.MaxPool2d and m.kernel_size in (2, (2, 2)) and m.stride in (2, (2, 2))
                    and m.padding in (0, (0, 0)) and m.dilation in (1, (1, 1)) and not m.ceil_mode
                    and not m.return_indices):
                x = maxpool2x2(x)
            else:
                x = m(x)
            i += 1
        return x

    def feature_maps(self, x):
        """The last feature map [B, C, H, W]: what the average pool of the head reads."""
        x = self.normalize(x)
        return self._fused_features(x) if self.fused_bn else self.features(x)

    def forward(self, x):
        return self.classifier(torch.flatten(self.avgpool(self.feature_maps(x)), 1))

    def forward_loss(self, x, target, meters=None):
        """(mean cross-entropy, logits.detach()) of a batch; with `use_fused_head` the head is K23."""
        from ...cls_head import forward_loss
        return forward_loss(self, x, target, meters)


def vgg16_bn_lth(num_classes: int = 10, **kw) -> VGG:
    """Configuration "D" with BatchNorm.  As in the reference, there is no ImageNet variant of this network: its
    constructor takes no `imagenet` argument, so asking for one is a TypeError."""
    if kw.pop("imagenet", False):
        raise TypeError("VGG.__init__() got an unexpected keyword argument 'imagenet'")
    return VGG(CFG_D, num_classes=num_classes, **kw)
