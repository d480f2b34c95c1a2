"""RegNet backbone (T/mmdet/models/backbones/regnet.py): a ResNet whose stage widths, depths and group widths come from the RegNet
parameters (w0, wa, wm, group_w, depth, bot_mul), built from ResNeXt bottlenecks with ``expansion = 1`` -- conv1 inplanes -> W (1x1),
conv2 W -> W (3x3 in W / group_w groups), conv3 W -> W (1x1) -- behind a stem of ONE 3x3 / stride 2 conv, 3 -> 32, + BN + ReLU and no
max-pool.  Every stage strides (``strides=(2, 2, 2, 2)``), so the outputs sit at strides 4 .. 32 like ResNet's.

Widths that are no multiple of 32 (regnetx_1.6gf: 72, 168, 408, 912; 3.2gf: 432, 1008; 4.0gf: all four; 6.4gf: all four): every map of
such a block -- its input, conv1's and conv2's outputs, its output -- is an NHWC buffer at pitch Cp = roundup(C, 32) whose pad channels
[C, Cp) are exact zeros.  The 1x1 (and dense 3x3) layers run on packs with zero rows / columns and folded BatchNorms with zero scale /
shift in the pad (relu(0 * 0 + 0 + 0) = 0); the grouped 3x3 runs at the pitch (csrc/conv_group.hip: pad channels never read, written as
+0.0 by the kernel); residual add, ReLU and the avg_down pool run on the padded map.  ``forward`` returns views of the reference's
shapes (N, C, H, W) that carry their buffer (ops.as_nchw_padded), which the FPN reads in place.  Blocks whose widths are all multiples
of 32 (regnetx_400mf / 800mf, the first two stages of 3.2gf) are the ResNeXt block's code with another width rule.

fp32 compute mode and eval-mode BatchNorm only: the bf16 compute mode is refused naming ``arch``, batch statistics naming ``norm_eval``.
The recorded forward (``tape=``) feeds training.BackwardEngine._regnet_block_backward and the stem rule of _backward_stem
(csrc/stem3x3_bwd.hip)."""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..layers import _PackCache, _pack_job, folded_bn, folded_bn_padded, packed_conv, packed_conv_padded
from ..registry import BACKBONES
from .resnet import ResNet, _Block, block_width

ARCH_KEYS = ('w0', 'wa', 'wm', 'group_w', 'depth', 'bot_mul')


def generate_regnet(initial_width, width_slope, width_parameter, depth, divisor=8):
    """Per-block widths and the number of stages (regnet.py:251-281), numpy float math in the reference's operation order."""
    assert width_slope >= 0
    assert initial_width > 0
    assert width_parameter > 1
    assert initial_width % divisor == 0
    widths_cont = np.arange(depth) * width_slope + initial_width
    ks = np.round(np.log(widths_cont / initial_width) / np.log(width_parameter))
    widths = initial_width * np.power(width_parameter, ks)
    widths = np.round(np.divide(widths, divisor)) * divisor
    num_stages = len(np.unique(widths))
    return widths.astype(int).tolist(), num_stages


def quantize_float(number, divisor):
    """The closest non-zero int divisible by divisor (regnet.py:283-294)."""
    return int(round(number / divisor) * divisor)


def adjust_width_group(widths, bottleneck_ratio, groups):
    """Widths made divisible by their group widths (regnet.py:296-319)."""
    bottleneck_width = [int(w * b) for w, b in zip(widths, bottleneck_ratio)]
    groups = [min(g, w_bot) for g, w_bot in zip(groups, bottleneck_width)]
    bottleneck_width = [quantize_float(w_bot, g) for w_bot, g in zip(bottleneck_width, groups)]
    widths = [int(w_bot / b) for w_bot, b in zip(bottleneck_width, bottleneck_ratio)]
    return widths, groups


def get_stages_from_blocks(widths):
    """(stage widths, blocks per stage) of a per-block width list (regnet.py:321-341)."""
    width_diff = [width != width_prev for width, width_prev in zip(widths + [0], [0] + widths)]
    stage_widths = [width for width, diff in zip(widths, width_diff[:-1]) if diff]
    stage_blocks = np.diff([depth for depth, diff in zip(range(len(width_diff)), width_diff) if diff]).tolist()
    return stage_widths, stage_blocks


def stage_layout(arch):
    """(stage_widths, group_widths, stage_blocks) of an arch dict, as the reference's constructor derives them (regnet.py:123-141)."""
    widths, num_stages = generate_regnet(arch['w0'], arch['wa'], arch['wm'], arch['depth'])
    stage_widths, stage_blocks = get_stages_from_blocks(widths)
    group_widths = [arch['group_w'] for _ in range(num_stages)]
    ratio = [arch['bot_mul'] for _ in range(num_stages)]
    stage_widths, group_widths = adjust_width_group(stage_widths, ratio, group_widths)
    return stage_widths, group_widths, stage_blocks[:num_stages]


_BATCH_STATS = 'BatchNorm batch statistics in a RegNet backbone (norm_eval=False with a stage or the stem that is not frozen): its blocks ' \
    'and its stem run with eval-mode BatchNorm only -- keep norm_eval=True'


class _RegBottleneck(_Block):
    """The ResNeXt Bottleneck with expansion 1 (regnet.py:165-167, resnext.py:11-84).  kind 'bottleneck': every width a multiple of 32,
    the ResNeXt block's code; kind 'regnet': maps at pitch roundup(C, 32), see the module docstring."""

    def __init__(self, inplanes, planes, stride, downsample, norm, style, group_w):
        nn.Module.__init__(self)
        groups = planes // group_w
        width = block_width(planes, groups, group_w, planes)          # (resnext.py:28-32 with base_channels = planes)
        s1, s2 = (1, stride) if style == 'pytorch' else (stride, 1)
        self.conv1 = nn.Conv2d(inplanes, width, 1, s1, bias=False)
        self.bn1 = norm(width)
        self.conv2 = nn.Conv2d(width, width, 3, s2, 1, groups=groups, bias=False)
        self.bn2 = norm(width)
        self.conv3 = nn.Conv2d(width, planes, 1, bias=False)
        self.bn3 = norm(planes)
        self.downsample = downsample
        self.inplanes, self.planes, self.width = inplanes, planes, width
        self.kind = 'bottleneck' if inplanes % 32 == 0 and planes % 32 == 0 and width % 32 == 0 else 'regnet'

    def conv2_pack(self, cache, Wp):
        """conv2 at pitch Wp: the grouped kernel's pack (refreshed in place after an optimizer step), or with one group a dense one."""
        conv = self.conv2
        if conv.groups == 1:
            return packed_conv_padded(cache, conv, Wp, Wp)
        w = conv.weight
        return cache.get(('rg_pc2', id(conv), Wp), [w], lambda: ops.PackedConv(w, conv.stride[0], 1, groups=conv.groups, pitch=Wp),
                         lambda pc: _pack_job(pc, w))

    def run(self, cache, x, save=None):
        if self.batch_stats():      # (here, not only in RegNet._check_mode: the refusal must not depend on the entry point)
            raise NotImplementedError(_BATCH_STATS)
        if self.kind == 'bottleneck':
            return super().run(cache, x, save)
        assert x.dtype == torch.float32
        Ip, Wp, Pp = ops.pad32(self.inplanes), ops.pad32(self.width), ops.pad32(self.planes)
        assert x.shape[-1] == Ip, (tuple(x.shape), self.inplanes)
        s1, b1 = folded_bn_padded(cache, self.bn1, Wp)
        o1 = ops.conv2d(x, packed_conv_padded(cache, self.conv1, Wp, Ip), scale=s1, bias=b1, relu=True)
        if self.conv2.groups == 1:
            s2, b2 = folded_bn_padded(cache, self.bn2, Wp)
        else:
            s2, b2 = folded_bn(cache, self.bn2)          # (the grouped kernel reads the real channels' entries alone)
        o2 = ops.conv2d(o1, self.conv2_pack(cache, Wp), scale=s2, bias=b2, relu=True)
        out, xp = self.conv3_shortcut(cache, x, o2, Pp, save is not None)
        if save is not None:
            save.update(block=self, x=x, xp=xp, o1=o1, o2=o2, out=out)
        return out


@BACKBONES.register_module()
class RegNet(ResNet):
    """RegNet (regnet.py:12-355): ``RegNet(arch='regnetx_3.2gf')`` or ``arch=dict(w0=, wa=, wm=, group_w=, depth=, bot_mul=)``.  State-
    dict keys and shapes are the reference's: conv1 / bn1 (the stem), layer{1..4}.{i}.conv1 / bn1 / conv2 / bn2 / conv3 / bn3 /
    downsample.*.  Built: group widths in ops.GROUP_WIDTHS (regnetx_400mf .. 6.4gf), bot_mul = 1.0."""
    arch_settings = {
        'regnetx_400mf': dict(w0=24, wa=24.48, wm=2.54, group_w=16, depth=22, bot_mul=1.0),
        'regnetx_800mf': dict(w0=56, wa=35.73, wm=2.28, group_w=16, depth=16, bot_mul=1.0),
        'regnetx_1.6gf': dict(w0=80, wa=34.01, wm=2.25, group_w=24, depth=18, bot_mul=1.0),
        'regnetx_3.2gf': dict(w0=88, wa=26.31, wm=2.25, group_w=48, depth=25, bot_mul=1.0),
        'regnetx_4.0gf': dict(w0=96, wa=38.65, wm=2.43, group_w=40, depth=23, bot_mul=1.0),
        'regnetx_6.4gf': dict(w0=184, wa=60.83, wm=2.07, group_w=56, depth=17, bot_mul=1.0),
        'regnetx_8.0gf': dict(w0=80, wa=49.56, wm=2.88, group_w=120, depth=23, bot_mul=1.0),
        'regnetx_12gf': dict(w0=168, wa=73.36, wm=2.37, group_w=112, depth=19, bot_mul=1.0),
    }

    def __init__(self, arch, in_channels=3, stem_channels=32, base_channels=32, strides=(2, 2, 2, 2), dilations=(1, 1, 1, 1),
                 out_indices=(0, 1, 2, 3), style='pytorch', deep_stem=False, avg_down=False, frozen_stages=-1, conv_cfg=None,
                 norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None, stage_with_dcn=(False, False, False, False),
                 plugins=None, with_cp=False, zero_init_residual=True, pretrained=None, init_cfg=None):
        nn.Module.__init__(self)
        self.arch = arch
        if isinstance(arch, str):
            assert arch in self.arch_settings, '"arch": "%s" is not one of the arch_settings' % arch
            arch = self.arch_settings[arch]
        elif not isinstance(arch, dict):
            raise ValueError('Expect "arch" to be either a string or a dict, got %s' % type(arch))
        stage_widths, group_widths, stage_blocks = stage_layout(arch)
        num_stages = len(stage_widths)
        assert 1 <= num_stages <= 4
        assert len(strides) == len(dilations) == num_stages
        assert max(out_indices) < num_stages
        assert style in ('pytorch', 'caffe'), style
        if arch['bot_mul'] != 1.0:
            raise NotImplementedError('RegNet arch bot_mul=%r is not built: the RegNetX settings (bot_mul=1.0) are' % (arch['bot_mul'],))
        for i, (w, g) in enumerate(zip(stage_widths, group_widths)):
            if w // g > 1 and g not in ops.GROUP_WIDTHS:
                raise NotImplementedError('RegNet arch group_w=%d (stage %d: %d channels in %d groups of %d): the grouped 3x3 kernels '
                                          '(csrc/conv_group.hip) are built for group widths %s'
                                          % (arch['group_w'], i + 1, w, w // g, g, list(ops.GROUP_WIDTHS)))
        if deep_stem:
            raise NotImplementedError('RegNet with deep_stem=True is not built (the reference\'s RegNet never builds the deep stem its '
                                      '_freeze_stages would then look for)')
        if tuple(dilations) != (1,) * num_stages:
            raise NotImplementedError('RegNet dilations=%r is not built: every stage runs at dilation 1' % (tuple(dilations),))
        for key, val in (('dcn', dcn), ('plugins', plugins)):
            if val is not None:
                raise NotImplementedError('RegNet %s is not built (SURVEY.md §2a row 5)' % key)
        if with_cp:
            raise NotImplementedError('RegNet with_cp=True is not built (SURVEY.md §2a row 5)')
        if (in_channels, stem_channels) != (3, 32):
            raise NotImplementedError('the RegNet stem is built for in_channels=3, stem_channels=32 (csrc/stem_deep.hip), not '
                                      'in_channels=%r, stem_channels=%r' % (in_channels, stem_channels))
        if norm_cfg.get('type') not in ('BN', 'SyncBN'):
            raise NotImplementedError("norm_cfg type %r is not built: the backbone norms are 'BN' (nn.BatchNorm2d) or 'SyncBN' "
                                      "(nn.SyncBatchNorm)" % (norm_cfg.get('type'),))
        bn_kw = {'momentum': norm_cfg['momentum']} if 'momentum' in norm_cfg else {}
        norm_cls = nn.SyncBatchNorm if norm_cfg['type'] == 'SyncBN' else nn.BatchNorm2d

        def norm(c):
            return norm_cls(c, **bn_kw)
        self.stage_widths, self.group_widths, self.stage_blocks = stage_widths, group_widths, stage_blocks
        self.bottleneck_ratio = [arch['bot_mul']] * num_stages
        self.depth, self.num_stages, self.out_indices = sum(stage_blocks), num_stages, tuple(out_indices)
        self.stem_channels, self.base_channels, self.strides, self.dilations = stem_channels, base_channels, strides, dilations
        self.frozen_stages, self.norm_eval = frozen_stages, norm_eval
        self.style, self.deep_stem, self.avg_down = style, False, bool(avg_down)
        self.fp32_only = 'a RegNet backbone (arch=%r) runs in the fp32 compute mode only: the bf16 compute mode has no grouped ' \
            'convolution (groups) and no padded-pitch layers' % (self.arch,)
        self.conv1 = nn.Conv2d(in_channels, stem_channels, 3, 2, 1, bias=False)
        self.bn1 = norm(stem_channels)
        inplanes = stem_channels
        self.res_layers = []
        for i, blocks in enumerate(stage_blocks):
            planes = stage_widths[i]
            layer = []
            for bi in range(blocks):
                stride = strides[i] if bi == 0 else 1
                ds = None
                if bi == 0 and (stride != 1 or inplanes != planes):      # res_layer.py:32-60 with expansion 1
                    if self.avg_down:
                        ds = nn.Sequential(nn.AvgPool2d(kernel_size=stride, stride=stride, ceil_mode=True, count_include_pad=False),
                                           nn.Conv2d(inplanes, planes, 1, 1, bias=False), norm(planes))
                    else:
                        ds = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), norm(planes))
                layer.append(_RegBottleneck(inplanes, planes, stride, ds, norm, style, group_widths[i]))
                inplanes = planes
            name = 'layer%d' % (i + 1)
            self.add_module(name, nn.Sequential(*layer))
            self.res_layers.append(name)
        self.feat_dim = stage_widths[-1]
        self.compute_dtype = torch.float32
        self._cache = _PackCache()
        self.zero_init_residual = zero_init_residual
        self.init_weights()
        self._freeze_stages()

    def _check_mode(self):
        if self.compute_dtype != torch.float32:
            raise NotImplementedError(self.fp32_only)
        if self.batch_stats_active():
            raise NotImplementedError(_BATCH_STATS)

    def stem_train_reason(self):
        """None: this stem (conv 3x3 / 2, 3 -> 32, + bn1 + ReLU) has a backward rule (csrc/stem3x3_bwd.hip) -- given a trainable layer1,
        whose first block hands it its input gradient."""
        if not all(p.requires_grad for p in getattr(self, self.res_layers[0]).parameters()):
            return 'a trainable stem needs a trainable %s (its backward starts from that stage\'s input gradient)' % self.res_layers[0]
        return None

    def run_stem(self, x, tape=None):
        """(N,3,H,W) image -> the NHWC map (N,OH,OW,32) after conv1 + bn1 + ReLU (regnet.py:343-347), both input layouts the same bits.
        tape (list): when conv1 or bn1 trains, one record (``stem=True``, ``regnet=True``) is appended: the input as the kernel read it
        and the output map (its ReLU mask)."""
        self._check_mode()
        c, c1 = self._cache, self.conv1
        rec = None
        if tape is not None and any(p.requires_grad for p in (c1.weight, self.bn1.weight, self.bn1.bias)):
            reason = self.stem_train_reason()
            if reason is not None:
                raise NotImplementedError(reason)
            rec = dict(stem=True, regnet=True, stage=-1)
            tape.append(rec)
        planar = x.dim() == 4 and x.dtype == torch.float32 and x.shape[1] == 3 and x.is_contiguous()
        if not planar:
            # (N,3,H,W) float image -> NHWC4; a 4-channel channels-last view (datasets.GpuImagePipeline output) is taken as is
            x = ops.from_nchw(x) if (x.shape[1] == 4 and x.stride(1) == 1) else ops.nchw_to_nhwc(x)
        s, b = folded_bn(c, self.bn1)
        out = ops.stem3x3s2(x, packed_conv(c, c1), s, b, planar=planar)
        if rec is not None:
            rec.update(x=x, planar=planar, out=out)
        return out

    def stage_channels(self, i):
        return self.stage_widths[i]

    def forward(self, x, tape=None):
        """x: (N,3,H,W) -> tuple of the ``out_indices`` stage outputs, NCHW-shaped (N, stage width, H, W) views of the NHWC buffers;
        a padded stage's view carries its buffer (ops.as_nchw_padded).  tape (list): the training records, in forward order."""
        self._check_mode()
        x = self.run_stem(x, tape)
        outs = []
        for i in range(len(self.res_layers)):
            x = self.run_stage(i, x, tape)
            if i in self.out_indices:
                outs.append(ops.as_nchw_padded(x, self.stage_widths[i]))
        return tuple(outs)
