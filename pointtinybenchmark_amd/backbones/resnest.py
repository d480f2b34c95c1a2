"""ResNeSt backbone (T/mmdet/models/backbones/resnest.py): the ResNetV1d bottleneck whose 3x3 conv is a split-attention conv of radix 2
-- a 3x3 of w -> 2w channels in two groups + bn0 + ReLU (u), a per-image attention over the two splits from the pooled sum of the splits
(fc1 + bn1 + ReLU + fc2 + radix softmax), the attention-weighted sum of the splits (v) -- and whose stride sits in an AvgPool2d(3, 2, 1)
behind it (``avd_layer``) in the stride-2 first blocks of stages 2-4.  w = planes (groups = 1); the stage outputs keep ResNet's 256 .. 2048.

The 3x3 runs on the dense kernels: one dense w -> 2w conv whose (2w, w, 3, 3) weight holds the reference-shaped (2w, w/2, 3, 3) parameter in
its two diagonal blocks and exact zeros elsewhere (ops.splat_dense_weight; no refresh job, the pack lapses with the weight epoch).  Every
instance is stride 1, so the Winograd kernels with their fused scale / bias / ReLU epilogue take it; the price is twice the grouped layer's
FLOPs.  The split attention itself is csrc/splat.hip (ops.splat_gap / splat_attn / splat_apply: the pooled map's input never reaches
memory).

Built here: the forward (eval-mode BatchNorm, fp32 compute mode), through ``forward`` and the locators' lazy path, with the forward-only
fused shortcut, and the recorded forward (``tape=``) whose backward rule is training.BackwardEngine._resnest_block_backward.
Refused, each naming its key: ``radix`` != 2, ``groups`` != 1, ``avg_down_stride=False`` with style='pytorch' (a strided grouped conv2),
``dilations`` != 1, the bf16 compute mode (``radix``), BatchNorm batch statistics inside the blocks (``norm_eval``), and what ResNet
refuses (dcn, plugins, with_cp, a trainable deep stem, stem_channels != 64)."""
import torch
import torch.nn as nn

from .. import ops
from ..layers import folded_bn, packed_conv
from ..registry import BACKBONES
from .resnet import ResNet, _Block


def inter_channels(width, radix=2, reduction_factor=4):
    """Channels of the attention MLP's hidden layer (resnest.py:78)."""
    return max(width * radix // reduction_factor, 32)


def unsupported_reason(radix=2, groups=1, reduction_factor=4, avg_down_stride=True, style='pytorch', dilations=(1, 1, 1, 1)):
    """None when the split-attention kernels take this setting, else why not, naming the key."""
    if radix != ops.SPLAT_RADIX:
        return 'radix=%r: the split-attention kernels (csrc/splat.hip) are built for radix=2' % (radix,)
    if groups != 1:
        return 'groups=%r: the ResNeSt block is built for groups=1 (cardinality 1, width = planes)' % (groups,)
    if not (isinstance(reduction_factor, int) and reduction_factor >= 1):
        return 'reduction_factor=%r: a positive integer' % (reduction_factor,)
    if not avg_down_stride and style == 'pytorch':
        return "avg_down_stride=False with style='pytorch' puts the stride on the grouped 3x3 conv2, which is not built: keep " \
            "avg_down_stride=True (the stride in the block's 3x3 average pool) or style='caffe' (the stride on conv1)"
    if any(int(d) != 1 for d in dilations):
        return 'dilations=%r: a ResNeSt backbone runs at dilation 1 in every stage' % (tuple(dilations),)
    return None


def _not_mixed(radix):
    return NotImplementedError('a ResNeSt backbone (radix=%d) runs in the fp32 compute mode only: the bf16 compute mode (mixed precision) '
                               'has no split attention' % radix)


_BATCH_STATS = 'BatchNorm batch statistics inside a ResNeSt block (norm_eval=False with a stage that is not frozen): the split-attention ' \
    'blocks run with eval-mode BatchNorm only -- keep norm_eval=True'


class _SplitAttention(nn.Module):
    """SplitAttentionConv2d's parameters under its names (resnest.py:40-112): conv, bn0, fc1 (bias), bn1, fc2 (bias)."""

    def __init__(self, width, radix, reduction_factor, norm):
        super().__init__()
        inter = inter_channels(width, radix, reduction_factor)
        self.radix, self.channels, self.inter = radix, width, inter
        self.conv = nn.Conv2d(width, width * radix, 3, 1, 1, groups=radix, bias=False)
        self.bn0 = norm(width * radix)
        self.fc1 = nn.Conv2d(width, inter, 1)
        self.bn1 = norm(inter)
        self.fc2 = nn.Conv2d(inter, width * radix, 1)


class _ResNeStBlock(_Block):
    """Bottleneck of ResNeSt (resnest.py:153-273).  Registration order conv1, bn1, conv2 (conv, bn0, fc1, bn1, fc2), conv3, bn3,
    downsample -- the reference's state-dict order; there is no bn2, and the ``avd_layer`` pool has no parameters.  ``pool``: the block
    average-pools v (3x3 / 2 / padding 1) -- style 'pytorch' with stride 2; style 'caffe' puts the stride on conv1 and no block pools."""
    kind = 'resnest'

    def __init__(self, inplanes, planes, stride, downsample, norm, style, radix, reduction_factor):
        nn.Module.__init__(self)
        s1 = stride if style == 'caffe' else 1
        self.width, self.stride, self.pool = planes, stride, style == 'pytorch' and stride > 1
        self.conv1 = nn.Conv2d(inplanes, planes, 1, s1, bias=False)
        self.bn1 = norm(planes)
        self.conv2 = _SplitAttention(planes, radix, reduction_factor, norm)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = norm(planes * 4)
        self.downsample = downsample

    def _norms(self):
        return [self.bn1, self.conv2.bn0, self.conv2.bn1, self.bn3] + ([self.ds_bn] if self.downsample is not None else [])

    def conv2_pack(self, cache):
        """conv2.conv on the dense kernels: the block-diagonal (2w, w, 3, 3) weight's pack.  (No refresh job: it lapses with the weight
        epoch and rebuilds from the refreshed parameter.)"""
        conv = self.conv2.conv
        return cache.get(('st_pc2', id(conv)), [conv.weight], lambda: ops.PackedConv(ops.splat_dense_weight(conv.weight), 1, 1))

    def run(self, cache, x, save=None):
        if self.batch_stats():
            raise NotImplementedError(_BATCH_STATS)
        if x.dtype != torch.float32:
            raise _not_mixed(self.conv2.radix)
        sa = self.conv2
        s1, b1 = folded_bn(cache, self.bn1)
        o1 = ops.conv2d(x, packed_conv(cache, self.conv1), scale=s1, bias=b1, relu=True)
        s0, b0 = folded_bn(cache, sa.bn0)
        u = ops.conv2d(o1, self.conv2_pack(cache), scale=s0, bias=b0, relu=True)          # (N, H, W, 2w)
        g = ops.splat_gap(u)
        sm, bm = folded_bn(cache, sa.bn1)
        r = ops.splat_attn(g, sa.fc1.weight, sa.fc1.bias, sm, bm, sa.fc2.weight, sa.fc2.bias, record=save is not None)
        att, z = r if save is not None else (r, None)
        o = ops.splat_apply(u, att, pool=self.pool)
        out, xp = self.conv3_shortcut(cache, x, o, self.conv3.out_channels, save is not None)
        if save is not None:
            save.update(block=self, x=x, xp=xp, o1=o1, u=u, g=g, z=z, att=att, o=o, out=out)
        return out


@BACKBONES.register_module()
class ResNeSt(ResNet):
    """ResNeSt (resnest.py:276-321): ``ResNeSt(depth in {50, 101, 152, 200}, groups=1, base_width=4, radix=2, reduction_factor=4,
    avg_down_stride=True, **ResNetV1d kwargs)``; the constructor always builds deep_stem=True, avg_down=True (ResNetV1d).  State-dict
    keys and shapes are the reference's: ``stem.*``, and per block conv1, bn1, conv2.conv, conv2.bn0, conv2.fc1, conv2.bn1, conv2.fc2,
    conv3, bn3, downsample.*."""
    arch_settings = {50: ('bottleneck', (3, 4, 6, 3)), 101: ('bottleneck', (3, 4, 23, 3)), 152: ('bottleneck', (3, 8, 36, 3)),
                     200: ('bottleneck', (3, 24, 36, 3))}

    def __init__(self, groups=1, base_width=4, radix=2, reduction_factor=4, avg_down_stride=True, deep_stem=True, avg_down=True, **kwargs):
        why = unsupported_reason(radix, groups, reduction_factor, avg_down_stride, kwargs.get('style', 'pytorch'),
                                 tuple(kwargs.get('dilations', (1, 1, 1, 1)))[:kwargs.get('num_stages', 4)])
        if why is not None:
            raise NotImplementedError(why)
        self.base_width = base_width                      # (groups stays ResNet's 1: width = planes)
        self.radix, self.reduction_factor, self.avg_down_stride = radix, reduction_factor, bool(avg_down_stride)
        # (what the detectors' set_compute_dtype, the trainers' constructors and autograd_bridge.unsupported_reason report)
        self.fp32_only = str(_not_mixed(radix))
        super().__init__(deep_stem=True, avg_down=True, **kwargs)

    def _make_block(self, kind, inplanes, planes, stride, downsample, norm, style, base_channels, first, dilation=1):
        return _ResNeStBlock(inplanes, planes, stride, downsample, norm, style, self.radix, self.reduction_factor)

    def _check_mode(self):
        if self.compute_dtype != torch.float32:
            raise _not_mixed(self.radix)
        super()._check_mode()
        for name in self.res_layers:
            for blk in getattr(self, name):
                if blk.batch_stats():
                    raise NotImplementedError(_BATCH_STATS)
