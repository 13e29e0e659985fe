"""`model_dict` registry, as the reference exposes it (Classification/models/__init__.py:6-14).
ResNet-18 and VGG-16-BN (`vgg16_bn_lth`) are built here; other names raise with a pointer to the scope table."""
from .resnet_cifar import NormalizeByChannelMeanStd, ResNetCifar, resnet18
from .vgg_lth import VGG, vgg16_bn_lth


class _ModelDict(dict):
    def __missing__(self, key):
        raise KeyError(f"architecture {key!r} is outside the hot-path scope of this build (SURVEY.md §2 C7: "
                       "only resnet18 and vgg16_bn_lth are built)")


model_dict = _ModelDict(resnet18=resnet18, vgg16_bn_lth=vgg16_bn_lth)
