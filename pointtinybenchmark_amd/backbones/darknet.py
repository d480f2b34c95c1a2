"""Darknet backbone (T/mmdet/models/backbones/darknet.py): ``conv1`` (3x3, 3 -> 32, stride 1), then five ``conv_res_block{i}`` -- a
3x3 / stride 2 conv that doubles the width, followed by ResBlocks (1x1 to half the width, 3x3 back, ``out + residual``).  Every conv is
mmcv's ConvModule: conv (no bias) -> BN -> LeakyReLU(negative_slope).  Six stages -- conv1 and the five blocks -- of which
``out_indices`` picks; the default (3, 4, 5) gives 256 / 512 / 1024 channels at strides 8 / 16 / 32.

Every conv runs on the existing dense dispatch (ops.conv2d) in its raw folded-BN form -- scale and bias, no ReLU: those epilogues know
no negative slope and stay as they are.  The activation is one streaming pass (ops.leaky, csrc/darknet.hip): in place after conv1, a
stage's stride-2 conv and a ResBlock's conv1; ``out = leaky(z2) + x`` in one pass after a ResBlock's conv2.  conv1 reads the NHWC4
image in the dense kernel's Cin <= 4 mode.  Every width is a multiple of 32, so no map has a channel pad.

fp32 compute mode and eval-mode BatchNorm only: the bf16 compute mode is refused naming ``Darknet``, batch statistics naming
``norm_eval``.  The recorded forward (``tape=``) keeps a ResBlock's ``z2`` beside its output (the backward mask needs its sign; the
in-place maps need nothing extra: a > 0 exactly when z > 0) and feeds training.BackwardEngine._backward_darknet."""
import torch
import torch.nn as nn

from .. import ops
from ..layers import _PackCache, bump_weight_epoch, folded_bn, packed_conv
from ..registry import BACKBONES

_BatchNorm = nn.modules.batchnorm._BatchNorm

_BATCH_STATS = 'BatchNorm batch statistics in a Darknet backbone (norm_eval=False with a part that is not frozen, in training mode): ' \
    'its layers run with eval-mode BatchNorm only -- keep norm_eval=True'


def unsupported_reason(conv_cfg=None, norm_cfg=dict(type='BN'), act_cfg=dict(type='LeakyReLU', negative_slope=0.1)):
    """None when the kernels take this setting, else why not, naming the key."""
    slope = None if act_cfg is None else act_cfg.get('negative_slope', 0.01)
    if act_cfg is None or act_cfg.get('type') != 'LeakyReLU' or not isinstance(slope, (int, float)) or not 0 <= slope < 1:
        return "act_cfg=%r is not built: the activation pass (csrc/darknet.hip) is a LeakyReLU with 0 <= negative_slope < 1, " \
            "act_cfg=dict(type='LeakyReLU', negative_slope=0.1)" % (act_cfg,)
    if conv_cfg is not None and conv_cfg.get('type') not in (None, 'Conv2d'):
        return 'conv_cfg=%r is not built: plain Conv2d layers (conv_cfg=None)' % (conv_cfg,)
    if norm_cfg is None or norm_cfg.get('type') not in ('BN', 'SyncBN'):
        return "norm_cfg type %r is not built: the norms are 'BN' (nn.BatchNorm2d) or 'SyncBN' (nn.SyncBatchNorm)" \
            % (None if norm_cfg is None else norm_cfg.get('type'),)
    return None


def arch_reason(layers, channels):
    """None when the kernels take this ``arch_settings`` entry, else why not."""
    if len(layers) != len(channels) or not layers:
        return 'arch_settings entry has %d layer counts for %d channel pairs' % (len(layers), len(channels))
    prev = 32
    for i, (n, (cin, cout)) in enumerate(zip(layers, channels)):
        if cin != prev:
            return 'arch_settings stage %d reads %d channels where the stage before it writes %d (conv1 writes 32)' % (i + 1, cin, prev)
        if cout % 64 != 0 or cout <= 0:
            return "arch_settings stage %d has width %d: a stage width is a multiple of 64 (the ResBlock's half width feeds the dense " \
                'kernels, which take multiples of 32)' % (i + 1, cout)
        if n < 0:
            return 'arch_settings stage %d has %d ResBlocks' % (i + 1, n)
        prev = cout
    return None


class _ConvBN(nn.Module):
    """mmcv's ConvModule as a parameter holder: ``conv`` (no bias) and ``bn``; the activation is a pass of its own (ops.leaky)."""

    def __init__(self, cin, cout, k, stride, norm):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride, k // 2, bias=False)
        self.bn = norm(cout)

    def raw(self, cache, x):
        """z = BN(conv(x)), the folded eval-mode form, no activation."""
        s, b = folded_bn(cache, self.bn)
        return ops.conv2d(x, packed_conv(cache, self.conv), scale=s, bias=b)


class ResBlock(nn.Module):
    """darknet.py:13-55: conv1 1x1 C -> C/2, conv2 3x3 C/2 -> C, ``out + residual``."""

    def __init__(self, channels, norm):
        super().__init__()
        assert channels % 2 == 0
        self.conv1 = _ConvBN(channels, channels // 2, 1, 1, norm)
        self.conv2 = _ConvBN(channels // 2, channels, 3, 1, norm)

    def run(self, cache, x, slope, save=None):
        a1 = ops.leaky(self.conv1.raw(cache, x), slope)
        z2 = self.conv2.raw(cache, a1)
        if save is None:
            return ops.leaky(z2, slope, res=x)
        out = ops.leaky(z2, slope, res=x, out=torch.empty_like(z2))
        save.update(x=x, a1=a1, z2=z2)
        return out


@BACKBONES.register_module()
class Darknet(nn.Module):
    """Darknet (darknet.py:58-212).  State-dict keys and shapes are the reference's: conv1.conv / conv1.bn, conv_res_block{i}.conv.conv /
    .conv.bn, conv_res_block{i}.res{j}.conv1.conv / .conv1.bn / .conv2.conv / .conv2.bn."""
    # Dict(depth: (layers, channels)), read at construction (darknet.py:94-98): add an entry to build another depth
    arch_settings = {53: ((1, 2, 8, 8, 4), ((32, 64), (64, 128), (128, 256), (256, 512), (512, 1024)))}
    darknet = True      # training.BackwardEngine walks this backbone's one record (_backward_darknet), autograd_bridge one Function

    def __init__(self, depth=53, out_indices=(3, 4, 5), frozen_stages=-1, conv_cfg=None, norm_cfg=dict(type='BN', requires_grad=True),
                 act_cfg=dict(type='LeakyReLU', negative_slope=0.1), norm_eval=True, pretrained=None, init_cfg=None):
        super().__init__()
        if depth not in self.arch_settings:
            raise KeyError('invalid depth %s for darknet' % (depth,))
        assert not (init_cfg and pretrained), 'init_cfg and pretrained cannot be setting at the same time'
        if not (pretrained is None or isinstance(pretrained, str)):
            raise TypeError('pretrained must be a str or None')
        reason = unsupported_reason(conv_cfg, norm_cfg, act_cfg)
        if reason is not None:
            raise NotImplementedError('Darknet ' + reason)
        self.layers, self.channels = self.arch_settings[depth]
        reason = arch_reason(self.layers, self.channels)
        if reason is not None:
            raise NotImplementedError('Darknet depth=%r: %s' % (depth, reason))
        n_stages = len(self.layers) + 1
        if not set(out_indices).issubset(range(n_stages)) or not len(out_indices):
            raise ValueError('out_indices must be a non-empty subset of range(0, %d). But received %s' % (n_stages, out_indices))
        bn_kw = {'momentum': norm_cfg['momentum']} if 'momentum' in norm_cfg else {}
        norm_cls = nn.SyncBatchNorm if norm_cfg['type'] == 'SyncBN' else nn.BatchNorm2d
        rg = norm_cfg.get('requires_grad', True)

        def norm(c):
            m = norm_cls(c, **bn_kw)
            for p in m.parameters():
                p.requires_grad = rg
            return m
        self.depth, self.out_indices, self.frozen_stages = depth, tuple(out_indices), frozen_stages
        self.conv_cfg, self.norm_cfg, self.act_cfg = conv_cfg, norm_cfg, act_cfg
        self.norm_eval, self.pretrained, self.init_cfg = norm_eval, pretrained, init_cfg
        self.negative_slope = float(act_cfg.get('negative_slope', 0.01))
        self.fp32_only = 'a Darknet backbone runs in the fp32 compute mode only: the bf16 compute mode has no LeakyReLU pass'
        self.conv1 = _ConvBN(3, 32, 3, 1, norm)
        self.cr_blocks = ['conv1']
        for i, n_layers in enumerate(self.layers):
            name = 'conv_res_block%d' % (i + 1)
            in_c, out_c = self.channels[i]
            self.add_module(name, self.make_conv_res_block(in_c, out_c, n_layers, norm))
            self.cr_blocks.append(name)
        self.stage_widths = [32] + [c[1] for c in self.channels]
        self.feat_dim = self.stage_widths[max(self.out_indices)]
        self.compute_dtype = torch.float32
        self._cache = _PackCache()
        self.init_weights()

    @staticmethod
    def make_conv_res_block(in_channels, out_channels, res_repeat, norm):      # darknet.py:178-212
        model = nn.Sequential()
        model.add_module('conv', _ConvBN(in_channels, out_channels, 3, 2, norm))
        for idx in range(res_repeat):
            model.add_module('res%d' % idx, ResBlock(out_channels, norm))
        return model

    def init_weights(self):
        """The reference's default init_cfg (darknet.py:141-148): Kaiming on every conv (mmcv's KaimingInit defaults: normal, fan_out,
        relu), constant 1 on every norm (bias 0)."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, _BatchNorm):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        bump_weight_epoch()

    def _freeze_stages(self):      # darknet.py:162-168
        if self.frozen_stages >= 0:
            for i in range(self.frozen_stages):
                m = getattr(self, self.cr_blocks[i])
                m.eval()
                for p in m.parameters():
                    p.requires_grad = False

    def train(self, mode=True):      # darknet.py:170-176
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, _BatchNorm):
                    m.eval()
        return self

    # ---------------------------------------------------------------------------------------------- structure
    def stage_parts(self, i):
        """Stage ``i`` >= 1 -> (its stride-2 ConvModule, [its ResBlocks])."""
        seq = getattr(self, self.cr_blocks[i])
        return seq.conv, [m for m in seq if isinstance(m, ResBlock)]

    def last_stage(self):
        """The last stage an output is taken from: nothing behind it is computed, and nothing behind it receives a gradient."""
        return max(self.out_indices)

    def stem_parameters(self):
        return list(self.conv1.parameters())

    def stem_train_reason(self):
        """None: conv1 has a backward rule (the weight gradient of csrc/darknet.hip)."""
        return None

    def freeze_reason(self):
        """None when the frozen parameters form sets the folded conv -> BN backward rule serves (HRNet.freeze_reason): a conv and the
        BatchNorm behind it train or are frozen together, or the conv trains under a wholly frozen norm."""
        for name, m in self.named_modules():
            if isinstance(m, _ConvBN):
                cw, g, b = m.conv.weight.requires_grad, m.bn.weight.requires_grad, m.bn.bias.requires_grad
                if g != b or (g and not cw):
                    return 'Darknet: %s.conv.weight, %s.bn.weight and %s.bn.bias have requires_grad = %s, %s, %s: a conv and the ' \
                        'BatchNorm behind it train or are frozen together (or the conv trains under a frozen norm) -- their gradients ' \
                        'come from one pass' % (name, name, name, cw, g, b)
        return None

    def batch_stats_active(self):
        return self.training and any(m.training for m in self.modules() if isinstance(m, _BatchNorm))

    def _check_mode(self):
        if self.compute_dtype != torch.float32:
            raise NotImplementedError(self.fp32_only)
        if self.batch_stats_active():
            raise NotImplementedError(_BATCH_STATS)

    # ---------------------------------------------------------------------------------------------- forward
    def run(self, img, tape=None):
        """(N,3,H,W) image -> the NHWC outputs of the ``out_indices`` stages, in stage order.  tape (list): one record
        (``darknet=True``) is appended -- ``x4`` the NHWC4 image conv1 read, ``a0`` conv1's activated map, ``stages``: per stage 1 ..
        last_stage ``x`` (the stride-2 conv's input), ``a`` (its activated output), ``blocks`` (ResBlock.run's records).  Stages behind the last output are not run."""
        self._check_mode()
        c, slope = self._cache, self.negative_slope
        x4 = ops.from_nchw(img) if (img.shape[1] == 4 and img.stride(1) == 1) else ops.nchw_to_nhwc(img)
        x = ops.leaky(self.conv1.raw(c, x4), slope)
        rec = None
        if tape is not None:
            rec = dict(darknet=True, x4=x4, a0=x, stages=[])
            tape.append(rec)
        outs = {0: x}
        for i in range(1, self.last_stage() + 1):
            conv, blocks = self.stage_parts(i)
            a = ops.leaky(conv.raw(c, x), slope)
            srec = dict(x=x, a=a, blocks=[]) if rec is not None else None
            x = a
            for blk in blocks:
                r = {} if rec is not None else None
                x = blk.run(c, x, slope, r)
                if rec is not None:
                    srec['blocks'].append(r)
            if rec is not None:
                rec['stages'].append(srec)
            outs[i] = x
        return [outs[i] for i in sorted(set(self.out_indices))]

    def forward(self, x, tape=None):
        """x: (N,3,H,W) -> tuple of the ``out_indices`` stage outputs in stage order, NCHW views (N, width, H, W) of the NHWC buffers."""
        return tuple(ops.as_nchw(y) for y in self.run(x, tape))
