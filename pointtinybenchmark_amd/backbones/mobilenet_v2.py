"""MobileNetV2 backbone (T/mmdet/models/backbones/mobilenet_v2.py, T/mmdet/models/utils/inverted_residual.py): a stem conv 3x3 / 2,
3 -> 32, seven layers of inverted-residual blocks -- expand 1x1 (+ BN + ReLU6), depthwise 3x3 (+ BN + ReLU6), linear 1x1 (+ BN), with
``x +`` around a block of stride 1 and equal widths -- and conv2, a 1x1 320 -> 1280 (+ BN + ReLU6).  Eight stages: layer1 .. layer7 and
conv2; ``out_indices`` picks among them.

Every map is an NHWC fp32 buffer at pitch Cp = roundup(C, 32) whose pad channels [C, Cp) are exact zeros (widths 16, 24 and 144 are no
multiples of 32).  The 1x1 layers run on the dense conv path with zero-embedded packs and folds (layers.packed_conv_padded /
folded_bn_padded); its epilogue knows ReLU, not ReLU6, so an expand conv (and the stem) writes ReLU(v) and the depthwise kernel clamps at
6 while it loads (csrc/mbv2.hip, ``in_clamp6``) -- no dense kernel changes.  The depthwise output is clamped by its own epilogue; conv2's
ReLU(v) map leaves the backbone, so one in-place pass clamps it (ops.clamp6).  ``forward`` returns views of the reference's shapes
(N, C, H, W) that carry their buffer (ops.as_nchw_padded), which the necks read in place.

fp32 compute mode and eval-mode BatchNorm only: the bf16 compute mode is refused naming ``MobileNetV2``, batch statistics naming
``norm_eval``.  The recorded forward (``tape=``) feeds training.BackwardEngine._mbv2_block_backward, the conv2 rule and the MobileNetV2
stem rule of _backward_stem.  The depthwise packs have no in-place refresh job: they lapse with the weight epoch and are rebuilt from
the parameters (ops.DwPack, one small launch), as the padded dense packs are."""
import torch
import torch.nn as nn

from .. import ops
from ..layers import _PackCache, bump_weight_epoch, folded_bn, folded_bn_padded, packed_conv, packed_conv_padded
from ..registry import BACKBONES

_BatchNorm = nn.modules.batchnorm._BatchNorm

_BATCH_STATS = 'BatchNorm batch statistics in a MobileNetV2 backbone (norm_eval=False with a layer or the stem that is not frozen): its ' \
    'blocks and its stem run with eval-mode BatchNorm only -- keep norm_eval=True'


def make_divisible(value, divisor, min_value=None, min_ratio=0.9):
    """``value`` rounded to a multiple of ``divisor``, never below ``min_ratio`` of it (mmdet/models/utils/make_divisible.py)."""
    if min_value is None:
        min_value = divisor
    new_value = max(min_value, int(value + divisor / 2) // divisor * divisor)
    if new_value < min_ratio * value:
        new_value += divisor
    return new_value


def unsupported_reason(widen_factor=1., conv_cfg=None, norm_cfg=dict(type='BN'), act_cfg=dict(type='ReLU6'), with_cp=False):
    """None when the kernels take this setting, else why not, naming the key."""
    if widen_factor != 1.0:
        return 'widen_factor=%r is not built: the stem kernel is 3 -> 32 (csrc/stem_deep.hip), widen_factor=1.0' % (widen_factor,)
    if act_cfg is None or act_cfg.get('type') != 'ReLU6':
        return "act_cfg=%r is not built: the depthwise kernels (csrc/mbv2.hip) clamp at 6, act_cfg=dict(type='ReLU6')" % (act_cfg,)
    if conv_cfg is not None and conv_cfg.get('type') not in (None, 'Conv2d'):
        return 'conv_cfg=%r is not built: plain Conv2d layers (conv_cfg=None)' % (conv_cfg,)
    if norm_cfg is None or norm_cfg.get('type') not in ('BN', 'SyncBN'):
        return "norm_cfg type %r is not built: the norms are 'BN' (nn.BatchNorm2d) or 'SyncBN' (nn.SyncBatchNorm)" \
            % (None if norm_cfg is None else norm_cfg.get('type'),)
    if with_cp:
        return 'with_cp=True is not built (SURVEY.md §2a row 5)'
    return None


class _ConvBN(nn.Module):
    """mmcv's ConvModule as a parameter holder: ``conv`` (no bias) and ``bn``; the activation lives in the kernels."""

    def __init__(self, cin, cout, k, stride, padding, norm, groups=1):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride, padding, groups=groups, bias=False)
        self.bn = norm(cout)

    def trainable(self):
        return [p for p in (self.conv.weight, self.bn.weight, self.bn.bias) if p.requires_grad]


def dw_pack(cache, conv):
    """The depthwise kernels' pack of ``conv`` (C, 1, 3, 3)."""
    return cache.get(('dw', id(conv)), [conv.weight], lambda: ops.DwPack(conv.weight))


def dw_dgrad_pack(cache, conv, bn):
    """The data-gradient pack: the folded weight scale * w."""
    return cache.get(('dw_dgrad', id(conv)), [conv.weight, bn.weight, bn.running_var],
                     lambda: ops.DwPack(conv.weight, folded_bn(cache, bn)[0]))


def _batch_stats(module, norms):
    return module.training and any(bn.training for bn in norms)


class InvertedResidual(nn.Module):
    """inverted_residual.py:8-123 without se_cfg: expand_conv (absent when ``with_expand_conv`` is False), depthwise_conv, linear_conv."""
    kind = 'mbv2'
    downsample = None

    def __init__(self, in_channels, out_channels, mid_channels, stride, with_expand_conv, norm):
        super().__init__()
        assert stride in (1, 2), 'stride must in [1, 2]. But received %s.' % (stride,)
        self.with_res_shortcut = stride == 1 and in_channels == out_channels
        self.with_expand_conv = with_expand_conv
        if not with_expand_conv:
            assert mid_channels == in_channels
        else:
            self.expand_conv = _ConvBN(in_channels, mid_channels, 1, 1, 0, norm)
        self.depthwise_conv = _ConvBN(mid_channels, mid_channels, 3, stride, 1, norm, groups=mid_channels)
        self.linear_conv = _ConvBN(mid_channels, out_channels, 1, 1, 0, norm)
        self.in_channels, self.mid_channels, self.out_channels, self.stride = in_channels, mid_channels, out_channels, stride

    def conv_modules(self):
        return ([self.expand_conv] if self.with_expand_conv else []) + [self.depthwise_conv, self.linear_conv]

    def batch_stats(self):
        return _batch_stats(self, [m.bn for m in self.conv_modules()])

    def run(self, cache, x, save=None):
        """x: the block input at its pitch -- a linear map, or for layer1.0 the stem's ReLU(v) map.  save (dict): the recorded forward."""
        if self.batch_stats():      # (here, not only in MobileNetV2._check_mode: the refusal must not depend on the entry point)
            raise NotImplementedError(_BATCH_STATS)
        assert x.dtype == torch.float32
        Ip, Mp, Op = ops.pad32(self.in_channels), ops.pad32(self.mid_channels), ops.pad32(self.out_channels)
        assert x.shape[-1] == Ip, (tuple(x.shape), self.in_channels)
        o1 = x
        if self.with_expand_conv:
            ec = self.expand_conv
            s1, b1 = folded_bn_padded(cache, ec.bn, Mp)
            o1 = ops.conv2d(x, packed_conv_padded(cache, ec.conv, Mp, Ip), scale=s1, bias=b1, relu=True)      # ReLU(v): clamped on load
        dw = self.depthwise_conv
        s2, b2 = folded_bn(cache, dw.bn)      # (the depthwise kernel reads the real channels' entries alone)
        o2 = ops.dw_conv(o1, dw_pack(cache, dw.conv), self.stride, scale=s2, bias=b2, in_clamp6=True, relu6=True)
        lc = self.linear_conv
        s3, b3 = folded_bn_padded(cache, lc.bn, Op)
        out = ops.conv2d(o2, packed_conv_padded(cache, lc.conv, Op, Mp), scale=s3, bias=b3,
                         residual=x if self.with_res_shortcut else None)
        if save is not None:
            save.update(block=self, x=x, o1=o1, o2=o2, out=out)
        return out


class _Conv2Stage(_ConvBN):
    """conv2 (1x1, 320 -> 1280, + BN + ReLU6), the eighth stage."""
    kind = 'mbv2_conv2'
    downsample = None

    def batch_stats(self):
        return _batch_stats(self, [self.bn])

    def run(self, cache, x, save=None):
        if self.batch_stats():
            raise NotImplementedError(_BATCH_STATS)
        O, I = self.conv.weight.shape[:2]
        s, b = folded_bn_padded(cache, self.bn, ops.pad32(O))
        out = ops.clamp6(ops.conv2d(x, packed_conv_padded(cache, self.conv, ops.pad32(O), x.shape[-1]), scale=s, bias=b, relu=True))
        if save is not None:
            save.update(block=self, x=x, out=out)
        return out


@BACKBONES.register_module()
class MobileNetV2(nn.Module):
    """MobileNetV2 (mobilenet_v2.py:12-196).  State-dict keys and shapes are the reference's: conv1.conv / conv1.bn,
    layer{1..7}.{j}.expand_conv / depthwise_conv / linear_conv (.conv, .bn), conv2.conv / conv2.bn.  Built: widen_factor = 1.0."""
    # expand_ratio, channel, num_blocks, stride
    arch_settings = [[1, 16, 1, 1], [6, 24, 2, 2], [6, 32, 3, 2], [6, 64, 4, 2], [6, 96, 3, 1], [6, 160, 3, 2], [6, 320, 1, 1]]
    sparse_outputs = True      # out_indices picks among the stages: the k-th output is stage out_indices[k] (training.py, autograd_bridge.py)

    def __init__(self, widen_factor=1., out_indices=(1, 2, 4, 7), frozen_stages=-1, conv_cfg=None, norm_cfg=dict(type='BN'),
                 act_cfg=dict(type='ReLU6'), norm_eval=False, with_cp=False, pretrained=None, init_cfg=None):
        super().__init__()
        assert not (init_cfg and pretrained), 'init_cfg and pretrained cannot be setting at the same time'
        if not (pretrained is None or isinstance(pretrained, str)):
            raise TypeError('pretrained must be a str or None')
        if not set(out_indices).issubset(set(range(0, 8))):
            raise ValueError('out_indices must be a subset of range(0, 8). But received %s' % (out_indices,))
        if frozen_stages not in range(-1, 8):
            raise ValueError('frozen_stages must be in range(-1, 8). But received %s' % (frozen_stages,))
        reason = unsupported_reason(widen_factor, conv_cfg, norm_cfg, act_cfg, with_cp)
        if reason is not None:
            raise NotImplementedError('MobileNetV2 ' + reason)
        bn_kw = {'momentum': norm_cfg['momentum']} if 'momentum' in norm_cfg else {}
        norm_cls = nn.SyncBatchNorm if norm_cfg['type'] == 'SyncBN' else nn.BatchNorm2d
        rg = norm_cfg.get('requires_grad', True)

        def norm(c):
            m = norm_cls(c, **bn_kw)
            for p in m.parameters():
                p.requires_grad = rg
            return m
        self.widen_factor, self.out_indices, self.frozen_stages = widen_factor, tuple(out_indices), frozen_stages
        self.conv_cfg, self.norm_cfg, self.act_cfg = conv_cfg, norm_cfg, act_cfg
        self.norm_eval, self.with_cp, self.pretrained, self.init_cfg = norm_eval, with_cp, pretrained, init_cfg
        self.fp32_only = 'a MobileNetV2 backbone runs in the fp32 compute mode only: the bf16 compute mode has no depthwise convolution ' \
            'and no padded-pitch layers'
        self.in_channels = make_divisible(32 * widen_factor, 8)
        self.conv1 = _ConvBN(3, self.in_channels, 3, 2, 1, norm)
        self.layers, self.stage_widths = [], []
        for i, (expand_ratio, channel, num_blocks, stride) in enumerate(self.arch_settings):
            out_channels = make_divisible(channel * widen_factor, 8)
            blocks = []
            for j in range(num_blocks):
                blocks.append(InvertedResidual(self.in_channels, out_channels, int(round(self.in_channels * expand_ratio)),
                                               stride if j == 0 else 1, expand_ratio != 1, norm))
                self.in_channels = out_channels
            name = 'layer%d' % (i + 1)
            self.add_module(name, nn.Sequential(*blocks))
            self.layers.append(name)
            self.stage_widths.append(out_channels)
        self.out_channel = 1280
        self.add_module('conv2', _Conv2Stage(self.in_channels, self.out_channel, 1, 1, 0, norm))
        self.layers.append('conv2')
        self.stage_widths.append(self.out_channel)
        self.res_layers = self.layers      # the stage list the trainer and the autograd bridge walk
        self.feat_dim = self.out_channel
        self.compute_dtype = torch.float32
        self._cache = _PackCache()
        self.init_weights()

    def init_weights(self):
        """The reference's default init_cfg: Kaiming normal on every conv, BatchNorm weight 1 / bias 0 (mobilenet_v2.py:66-73)."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, _BatchNorm):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        bump_weight_epoch()

    def _freeze_stages(self):      # mobilenet_v2.py:166-174
        if self.frozen_stages >= 0:
            for p in self.conv1.parameters():
                p.requires_grad = False
        for i in range(1, self.frozen_stages + 1):
            layer = getattr(self, 'layer%d' % i)
            layer.eval()
            for p in layer.parameters():
                p.requires_grad = False

    def train(self, mode=True):      # mobilenet_v2.py:187-196
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, _BatchNorm):
                    m.eval()
        return self

    def stage_blocks(self, i):
        """The block-like modules of stage ``i``: a layer's InvertedResiduals, or [conv2]."""
        m = getattr(self, self.layers[i])
        return [m] if isinstance(m, _Conv2Stage) else list(m)

    def stage_channels(self, i):
        return self.stage_widths[i]

    def last_stage(self):
        """The last stage an output is taken from: nothing behind it is computed, and nothing behind it receives a gradient."""
        return max(self.out_indices)

    def batch_stats_active(self):
        return _batch_stats(self.conv1, [self.conv1.bn]) or any(b.batch_stats() for i in range(len(self.layers)) for b in self.stage_blocks(i))

    def _check_mode(self):
        if self.compute_dtype != torch.float32:
            raise NotImplementedError(self.fp32_only)
        if self.batch_stats_active():
            raise NotImplementedError(_BATCH_STATS)

    def stem_parameters(self):
        return list(self.conv1.parameters())

    def stem_train_reason(self):
        """None: the stem (conv 3x3 / 2, 3 -> 32, + BN + ReLU6) has a backward rule (csrc/stem3x3_bwd.hip) -- given a trainable layer1,
        whose block hands it its input gradient."""
        if not all(p.requires_grad for p in self.layer1.parameters()):
            return 'a trainable stem needs a trainable layer1 (its backward starts from that layer\'s input gradient)'
        return None

    def run_stem(self, x, tape=None):
        """(N,3,H,W) image -> the NHWC map (N,OH,OW,32) after conv1 + BN + ReLU: ReLU(v), which layer1.0's depthwise clamps on load.
        tape (list): when the stem trains, one record (``stem=True``, ``mbv2=True``) is appended."""
        self._check_mode()
        c, m = self._cache, self.conv1
        rec = None
        if tape is not None and m.trainable():
            reason = self.stem_train_reason()
            if reason is not None:
                raise NotImplementedError(reason)
            rec = dict(stem=True, mbv2=True, stage=-1)
            tape.append(rec)
        planar = x.dim() == 4 and x.dtype == torch.float32 and x.shape[1] == 3 and x.is_contiguous()
        if not planar:
            x = ops.from_nchw(x) if (x.shape[1] == 4 and x.stride(1) == 1) else ops.nchw_to_nhwc(x)
        s, b = folded_bn(c, m.bn)
        out = ops.stem3x3s2(x, packed_conv(c, m.conv), s, b, planar=planar)
        if rec is not None:
            rec.update(x=x, planar=planar, out=out)
        return out

    def run_stage(self, i, x, tape=None):
        """Stage ``i`` (layer{i+1}, or conv2 for i == 7) on an NHWC map.  tape (list): one record per block with trainable parameters."""
        if self.compute_dtype != torch.float32:
            raise NotImplementedError(self.fp32_only)
        for blk in self.stage_blocks(i):
            rec = None
            if tape is not None and any(p.requires_grad for p in blk.parameters()):
                rec = dict(stage=i)
                tape.append(rec)
            x = blk.run(self._cache, x, rec)
        return x

    def forward(self, x, tape=None):
        """x: (N,3,H,W) -> tuple of the ``out_indices`` stage outputs in stage order, NCHW-shaped (N, stage width, H, W) views of the
        NHWC buffers; a stage of 16 or 24 channels hands over its pitch-32 buffer (ops.as_nchw_padded).  tape (list): the training
        records, in forward order.  Stages behind the last output are not run."""
        self._check_mode()
        x = self.run_stem(x, tape)
        outs = []
        for i in range(self.last_stage() + 1):
            x = self.run_stage(i, x, tape)
            if i in self.out_indices:
                outs.append(ops.as_nchw_padded(x, self.stage_widths[i]))
        return tuple(outs)
