from .resnet import ResNet, ResNeXt  # noqa: F401
