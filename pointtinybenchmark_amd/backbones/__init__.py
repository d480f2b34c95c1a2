from .resnet import ResNet, ResNeXt  # noqa: F401
from .res2net import Res2Net  # noqa: F401
from .regnet import RegNet  # noqa: F401
from .resnest import ResNeSt  # noqa: F401
from .mobilenet_v2 import MobileNetV2  # noqa: F401
from .hrnet import HRNet  # noqa: F401
from .darknet import Darknet  # noqa: F401
