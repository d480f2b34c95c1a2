from .fpn import FPN  # noqa: F401
from .pafpn import PAFPN  # noqa: F401
from .bfp import BFP, NeckSequence  # noqa: F401
from .hrfpn import HRFPN  # noqa: F401
from .ct_resnet_neck import CTResNetNeck  # noqa: F401
