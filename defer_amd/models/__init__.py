from defer_amd.models.resnet import (DEFER_8STAGE_CUTS, resnet50,  # noqa: F401
                                     resnet101, resnet152,
                                     resnext50_32x4d, resnext101_64x4d)
from defer_amd.models.convnext import convnext_tiny  # noqa: F401
from defer_amd.models.densenet import densenet121  # noqa: F401
from defer_amd.models.mobilenet import (mobilenet_v2,  # noqa: F401
                                        mobilenet_v3_large)
from defer_amd.models.swin import swin_b, swin_s, swin_t  # noqa: F401
from defer_amd.models.vgg import vgg19, vgg19_gap  # noqa: F401
from defer_amd.models.vit import vit_b16, vit_s16  # noqa: F401

MODELS = {"resnet50": resnet50, "resnet101": resnet101,
          "resnet152": resnet152, "resnext50_32x4d": resnext50_32x4d,
          "resnext101_64x4d": resnext101_64x4d, "vgg19": vgg19,
          "vgg19_gap": vgg19_gap, "densenet121": densenet121,
          "mobilenetv2": mobilenet_v2,
          "mobilenetv3large": mobilenet_v3_large,
          "convnext_tiny": convnext_tiny,
          "vit_b16": vit_b16, "vit_s16": vit_s16,
          "swin_t": swin_t, "swin_s": swin_s, "swin_b": swin_b}
