"""Res2Net backbone (T/mmdet/models/backbones/res2net.py): the bottleneck ResNet whose 3x3 conv is a hierarchy of ``scales - 1`` dense
3x3 convs of ``width -> width`` channels over the slices of conv1's output (width = floor(planes * base_width / base_channels): 26 / 52 /
104 / 208 at 26w4s), on the deep stem and the average-pool shortcuts of ResNetV1d.  The stage outputs keep ResNet's 256 .. 2048.

A block keeps two internal NHWC maps, conv1's output and the concatenated 3x3 output, at pitch Cp = roundup(width * scales, 32) -- the
dense 1x1 kernels take channel counts that are multiples of 32 -- whose pad channels hold exact zeros: conv1's pack has zero rows and a
zero folded scale / shift above width * scales, conv3's pack zero K columns there (both are built from the reference-shaped parameters and
lapse with the weight epoch).  The 3x3 chain runs on channel slices of the two maps in place (csrc/res2net.hip: ops.res2_conv reads
slice i of conv1's output, plus slice i - 1 of the concatenated map in a 'normal' block, and writes slice i of the concatenated map);
there is no split / contiguous / cat copy.  The last slice is copied, or in a stride-2 'stage' block average-pooled, by ops.res2_pool.

Built here: the forward (eval-mode BatchNorm, fp32 compute mode), through ``forward`` and the locators' lazy path, with the forward-only
fused shortcut (ops.conv2d_dual), and the recorded forward (``tape=``) whose backward rule is training.BackwardEngine._bottle2neck_backward.
Refused, each naming its key: the bf16 compute mode (``scales``), BatchNorm batch statistics inside the blocks (``norm_eval``), any
``dilations`` other than 1 (the slice kernels have no dilated form), and what ResNet refuses (dcn, plugins, with_cp, a trainable deep
stem)."""
import math

import torch
import torch.nn as nn

from .. import ops
from ..layers import folded_bn, folded_bn_padded, packed_conv_padded
from ..registry import BACKBONES
from .resnet import ResNet, _Block

SETTINGS = ((26, 4), (26, 6), (26, 8), (14, 8), (48, 2))      # the published (base_width, scales)


def slice_width(planes, base_width=26, base_channels=64):
    """Channels of one slice of a Bottle2neck (res2net.py:32)."""
    return int(math.floor(planes * (base_width / base_channels)))


def unsupported_reason(scales, base_width, base_channels=64, num_stages=4):
    """None when the slice kernels take this setting, else why not.  The rule: 2 <= scales <= 8, and at every stage the slice width
    floor(planes * base_width / base_channels) is even and at most 512 (the kernels move float2: every slice starts 8-byte aligned)."""
    if not (isinstance(scales, int) and 2 <= scales <= ops.RES2_MAX_SCALES):
        return 'scales=%r with base_width=%r: the Res2Net slice kernels (csrc/res2net.hip) are built for 2 <= scales <= %d' \
            % (scales, base_width, ops.RES2_MAX_SCALES)
    for i in range(num_stages):
        w = slice_width(base_channels * 2 ** i, base_width, base_channels)
        if not ops.res2_width_ok(w):
            return 'scales=%r with base_width=%r gives slices of %d channels at stage %d: the Res2Net slice kernels (csrc/res2net.hip) ' \
                'take even widths from 2 to %d' % (scales, base_width, w, i + 1, ops.RES2_MAX_WIDTH)
    return None


def _not_mixed(scales):
    return NotImplementedError('a Res2Net backbone (scales=%d) runs in the fp32 compute mode only: the bf16 compute mode (mixed precision) '
                               'has no slice convolution' % scales)


class _Bottle2neck(_Block):
    """Bottle2neck (res2net.py:14-159).  Registration order conv1, bn1, conv3, bn3, downsample, convs, bns -- the reference's
    state-dict order; there is no conv2 / bn2.  stage_type 'stage': the first block of a stage (its convs read their own slice alone, and
    at stride 2 the last slice is average-pooled); 'normal': every other block."""
    kind = 'bottle2neck'

    def __init__(self, inplanes, planes, stride, downsample, norm, scales, base_width, base_channels, stage_type):
        nn.Module.__init__(self)
        width = slice_width(planes, base_width, base_channels)
        self.scales, self.width, self.stage_type, self.stride = scales, width, stage_type, stride
        self.conv1 = nn.Conv2d(inplanes, width * scales, 1, 1, bias=False)
        self.bn1 = norm(width * scales)
        self.conv3 = nn.Conv2d(width * scales, planes * 4, 1, bias=False)
        self.bn3 = norm(planes * 4)
        self.downsample = downsample
        self.convs = nn.ModuleList([nn.Conv2d(width, width, 3, stride, 1, bias=False) for _ in range(scales - 1)])
        self.bns = nn.ModuleList([norm(width) for _ in range(scales - 1)])

    def _norms(self):
        return [self.bn1, self.bn3] + list(self.bns) + ([self.ds_bn] if self.downsample is not None else [])

    def run(self, cache, x, save=None):
        if self.batch_stats():
            raise NotImplementedError('BatchNorm batch statistics inside a Res2Net block (norm_eval=False with a stage that is not frozen): '
                                      'the Bottle2neck blocks run with eval-mode BatchNorm only -- keep norm_eval=True')
        if x.dtype != torch.float32:
            raise _not_mixed(self.scales)
        s, w, stride = self.scales, self.width, self.stride
        Wd = s * w
        Cp = ops.pad32(Wd)
        # the 1x1 layers around the padded pitch: packs and folds with exact zeros in the pad rows / columns
        pc1 = packed_conv_padded(cache, self.conv1, Cp, self.conv1.in_channels)
        s1, b1 = folded_bn_padded(cache, self.bn1, Cp)
        o1 = ops.conv2d(x, pc1, scale=s1, bias=b1, relu=True)                 # (N, H, W, Cp); channels >= Wd are relu(0 * 0 + 0) = 0
        N, H, W, _ = o1.shape
        OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
        # the concatenated map: the chain and the last slice write [0, Wd), the pad channels stay 0
        alloc = torch.zeros if Cp != Wd else torch.empty
        cat = alloc((N, OH, OW, Cp), device=x.device, dtype=torch.float32)
        for i in range(s - 1):
            conv, bn = self.convs[i], self.bns[i]
            pk = cache.get(('r2_pack', id(conv)), [conv.weight], lambda conv=conv: ops.Res2Pack(conv.weight))
            si, bi = folded_bn(cache, bn)
            carry = i > 0 and self.stage_type == 'normal'                      # y[i - 1] + spx[i], summed on load
            ops.res2_conv(o1, i * w, pk, cat, i * w, stride=stride, add=cat if carry else None, add_off=(i - 1) * w if carry else 0,
                          scale=si, bias=bi, relu=True)
        ops.res2_pool(o1, (s - 1) * w, cat, (s - 1) * w, w, stride)            # stride 2 ('stage' blocks only): the 3x3 average
        out, xp = self.conv3_shortcut(cache, x, cat, self.conv3.out_channels, save is not None)
        if save is not None:
            save.update(block=self, x=x, xp=xp, o1=o1, cat=cat, out=out)
        return out


@BACKBONES.register_module()
class Res2Net(ResNet):
    """Res2Net (res2net.py:241-326): ``Res2Net(scales=4, base_width=26, depth in {50, 101, 152}, **ResNet kwargs)``.  The constructor
    always builds style='pytorch', deep_stem=True, avg_down=True, whatever is passed (res2net.py:313-319).  State-dict keys and shapes are
    the reference's: ``stem.*``, and per block conv1, bn1, conv3, bn3, downsample.*, convs.i, bns.i."""
    arch_settings = {50: ('bottleneck', (3, 4, 6, 3)), 101: ('bottleneck', (3, 4, 23, 3)), 152: ('bottleneck', (3, 8, 36, 3))}

    def __init__(self, scales=4, base_width=26, style='pytorch', deep_stem=True, avg_down=True, **kwargs):
        why = unsupported_reason(scales, base_width, kwargs.get('base_channels', 64), kwargs.get('num_stages', 4))
        if why is not None:
            raise NotImplementedError(why)
        dil = tuple(kwargs.get('dilations', (1, 1, 1, 1)))[:kwargs.get('num_stages', 4)]
        assert all(d == 1 for d in dil), \
            'Res2Net dilations=%r is not built: the slice kernels (csrc/res2net.hip) have no dilated form -- every stage runs at dilation 1' % (dil,)
        self.scales = scales
        self.base_width = base_width
        super().__init__(style='pytorch', deep_stem=True, avg_down=True, **kwargs)

    def _make_block(self, kind, inplanes, planes, stride, downsample, norm, style, base_channels, first, dilation=1):
        return _Bottle2neck(inplanes, planes, stride, downsample, norm, self.scales, self.base_width, base_channels,
                            'stage' if first else 'normal')

    def _check_mode(self):
        if self.compute_dtype != torch.float32:
            raise _not_mixed(self.scales)
        super()._check_mode()
        for name in self.res_layers:
            for blk in getattr(self, name):
                if blk.batch_stats():
                    raise NotImplementedError('BatchNorm batch statistics inside a Res2Net block (norm_eval=False with a stage that is '
                                              'not frozen): the Bottle2neck blocks run with eval-mode BatchNorm only -- keep norm_eval=True')
