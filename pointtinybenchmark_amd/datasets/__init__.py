"""Data side feeding the hot path: annotation parsing of CocoFmtDataset and the device tail of the
image pipeline (resize, test-time tiles / scales / flips, flip, normalise, pad, batch, channels-last)."""
from .cocofmt import CocoFmtDataset  # noqa: F401
from .pipeline import GpuImagePipeline, GpuTestTimeAug  # noqa: F401
from .loader import BatchLoader  # noqa: F401
from .sampler import DistributedGroupSampler  # noqa: F401
from .tiles import generate_corner_dataset, image_tiles  # noqa: F401
