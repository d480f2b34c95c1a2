"""CTResNetNeck, the CenterNet neck (T/mmdet/models/necks/ct_resnet_neck.py:10-93): the LAST backbone map goes through one stage per entry
of ``num_deconv_filters`` -- 3x3 conv + BN + ReLU, then ConvTranspose2d(4, stride 2, padding 1) + BN + ReLU -- and comes out as ONE map at
2**stages times its resolution (a ResNet-18 C5, stride 32 / 512 channels, through (256, 128, 64): stride 4 / 64 channels).  The only neck
here that raises resolution with learned weights.

The 3x3 convs are the dense kernels every neck uses (Winograd where eligible); the transposed convs run in ops.deconv4x4s2
(csrc/deconv.hip): one launch for the four output-parity classes, the doubled map written directly.

Eval mode: both convs of a stage carry the folded BatchNorm + ReLU in their epilogues.  Train mode (``self.training``; the reference has
no ``norm_eval`` here): the raw conv output, ops.bn_batch_stats with the running-statistics update, ops.bn_apply(relu=True); the
statistics of a transposed conv's output run over its N * 2H * 2W rows.  The batch-statistics kernels take C % 64 == 0: a stage whose width is
an odd multiple of 32 runs its train-mode maps at width + 32 with exact-zero pad channels (bn_pitch).

Training (training.py ``_backward_ctneck``): per stage, last first, bn_train_bwd with the ReLU mask, the transposed conv's weight and data
gradient (dense-conv kernels with the roles swapped: ops.deconv4x4s2_wgrad / deconv4x4s2_dgrad_pack), bn_train_bwd, the 3x3 conv's.

Not built (NotImplementedError naming the key): ``use_dcn=True`` (the reference's default; mmcv's DCNv2 is not vendored), a
``num_deconv_kernels`` entry other than 4, widths that are no multiple of 32, SyncBatchNorm inside the neck, the bf16 compute mode,
and a recorded (training) forward through the neck in eval() mode."""
import math

import torch
import torch.nn as nn

from .. import ops
from ..layers import ConvModule, _PackCache, _zero_embedded, _zero_extended, folded_bn, packed_conv, packed_conv_padded
from ..registry import NECKS

BF16 = 'a CTResNetNeck runs in the fp32 compute mode only: the bf16 compute mode has no transposed convolution'
EVAL_TAPE = 'training through a CTResNetNeck in eval() mode is not built (the folded-BatchNorm rule for the (Cin, Cout, 4, 4) ' \
            'transposed-conv weight): call neck.train()'


class DeconvModule(nn.Module):
    """mmcv's ConvModule(conv_cfg=dict(type='deconv'), norm_cfg=dict(type='BN')): ``conv`` an nn.ConvTranspose2d without bias, ``bn``."""

    def __init__(self, channels):
        super().__init__()
        self.conv = nn.ConvTranspose2d(channels, channels, 4, stride=2, padding=1, bias=False)
        self.bn = nn.BatchNorm2d(channels)


@NECKS.register_module()
class CTResNetNeck(nn.Module):
    materialised = True         # forward_lazy returns the map, not a (raw, (a, b)) pair: BatchNorm + ReLU are applied here
    fp32_only = BF16

    def __init__(self, in_channel, num_deconv_filters, num_deconv_kernels, use_dcn=True, init_cfg=None):
        super().__init__()
        assert len(num_deconv_filters) == len(num_deconv_kernels) >= 1
        if use_dcn:
            raise NotImplementedError('CTResNetNeck use_dcn=True is not built: mmcv\'s DCNv2 is third-party and not vendored '
                                      '(pass use_dcn=False, the form of centernet_resnet18_140e_coco.py)')
        if any(k != 4 for k in num_deconv_kernels):
            raise NotImplementedError('CTResNetNeck num_deconv_kernels=%r is not built: the transposed-conv kernel is 4x4 / stride 2 / '
                                      'padding 1' % (tuple(num_deconv_kernels),))
        if in_channel % 32 != 0:
            raise NotImplementedError('CTResNetNeck in_channel=%r is not built: the convs take a multiple of 32 channels' % (in_channel,))
        if any(f % 32 != 0 or f <= 0 for f in num_deconv_filters):
            raise NotImplementedError('CTResNetNeck num_deconv_filters=%r is not built: the convs take multiples of 32 channels'
                                      % (tuple(num_deconv_filters),))
        self.in_channel, self.use_dcn, self.init_cfg = in_channel, use_dcn, init_cfg
        self.num_deconv_filters, self.num_deconv_kernels = tuple(num_deconv_filters), tuple(num_deconv_kernels)
        layers, c = [], in_channel
        for f in num_deconv_filters:
            layers.append(ConvModule(c, f, 3, padding=1, norm_cfg=dict(type='BN')))
            layers.append(DeconvModule(f))
            c = f
        self.deconv_layers = nn.Sequential(*layers)
        self.out_channels = c
        self._cache = _PackCache()
        self.init_weights()

    def init_weights(self):
        """ct_resnet_neck.py:63-87: the convs keep torch's reset_parameters, then every transposed conv's ``w[:, 0]`` is the bilinear
        upsampling kernel (1 - |i / f - c|)(1 - |j / f - c|) with f = ceil(k / 2), c = (2f - 1 - f % 2) / (2f); BatchNorm at 1 / 0."""
        for m in self.modules():
            if isinstance(m, nn.ConvTranspose2d):
                m.reset_parameters()
                w = m.weight.data
                f = math.ceil(w.size(2) / 2)
                c = (2 * f - 1 - f % 2) / (2. * f)
                for i in range(w.size(2)):
                    for j in range(w.size(3)):
                        w[0, 0, i, j] = (1 - math.fabs(i / f - c)) * (1 - math.fabs(j / f - c))
                for k in range(1, w.size(0)):
                    w[k, 0, :, :] = w[0, 0, :, :]
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Conv2d):
                m.reset_parameters()

    def stages(self):
        """[(the 3x3 ConvModule, the DeconvModule)] per stage."""
        mods = list(self.deconv_layers)
        return list(zip(mods[0::2], mods[1::2]))

    @staticmethod
    def bn_pitch(c):
        """Channels of a train-mode map of width c: the batch-statistics kernels take C % 64 == 0, so a width that is an odd multiple of
        32 runs at c + 32 with exact-zero pad channels (zero pack rows / columns, zero gamma / beta in the pad)."""
        return c if c % 64 == 0 else c + 32

    def deconv_pack(self, m, pitch=None):
        """The forward pack of a transposed conv; pitch: both channel counts padded to it (train mode at an odd multiple of 32)."""
        w = m.conv.weight
        p = w.shape[0] if pitch is None else pitch
        return self._cache.get(('deconv', id(m.conv), p), [w], lambda: ops.DeconvPack(w if p == w.shape[0] else _zero_embedded(w, p, p)))

    def deconv_dgrad_pack(self, m, pitch=None):
        """The data-gradient pack of a transposed conv (training): its weight read as a (Cin, Cout, 4, 4) stride-2 dense conv."""
        w = m.conv.weight
        p = w.shape[0] if pitch is None else pitch
        return self._cache.get(('deconv_dgrad', id(m.conv), p), [w],
                               lambda: ops.deconv4x4s2_dgrad_pack(w if p == w.shape[0] else _zero_embedded(w, p, p)))

    def _check(self, x):
        if x.dtype != torch.float32:
            raise NotImplementedError(BF16)
        assert x.shape[-1] == self.in_channel, 'CTResNetNeck(in_channel=%d) got a map of %d channels' % (self.in_channel, x.shape[-1])
        if any(isinstance(m.bn, nn.SyncBatchNorm) for m in self.deconv_layers):
            raise NotImplementedError('CTResNetNeck: nn.SyncBatchNorm inside the neck is not built (its BatchNorms take per-rank '
                                      'batch statistics)')

    @staticmethod
    def _bn_train(y, bn):
        """Batch statistics + running update + normalise + ReLU of the raw map y -> (BnStats, gamma as the kernels read it, output).  y wider
        than the BatchNorm (bn_pitch): gamma, beta and the running buffers are zero-extended copies -- the pad channels of the output are
        exact zeros -- and the real part of the updated buffers is copied back."""
        C, f = y.shape[-1], bn.num_features
        if C == f:
            gamma = bn.weight
            st = ops.bn_batch_stats(y, gamma, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps)
        else:
            gamma, beta = _zero_extended(bn.weight.detach(), C), _zero_extended(bn.bias.detach(), C)
            rm, rv = _zero_extended(bn.running_mean, C), _zero_extended(bn.running_var, C)
            st = ops.bn_batch_stats(y, gamma, beta, rm, rv, bn.num_batches_tracked, bn.momentum, bn.eps)
            bn.running_mean.copy_(rm[:f])
            bn.running_var.copy_(rv[:f])
        return st, gamma, ops.bn_apply(y, st.scale, st.cshift, center=st.center, relu=True)

    def run(self, x, tape=None):
        """x: the NHWC last backbone map -> the NHWC output map.  tape: one record per stage, kind 'ct_stage' -- the stage's input, the two
        raw conv outputs with their BnStats and gammas, and the two activated maps (the backward's ReLU masks and weight-gradient operands);
        in train mode the maps of a stage of width f sit at bn_pitch(f)."""
        self._check(x)
        if tape is not None and not self.training:
            raise NotImplementedError(EVAL_TAPE)
        for k, (cm, dm) in enumerate(self.stages()):
            if self.training:
                f = cm.conv.out_channels
                fp = self.bn_pitch(f)
                y1 = ops.conv2d(x, packed_conv_padded(self._cache, cm.conv, fp, x.shape[-1]))
                s1, g1, o1 = self._bn_train(y1, cm.bn)
                y2 = ops.deconv4x4s2(o1, self.deconv_pack(dm, fp))
                s2, g2, o2 = self._bn_train(y2, dm.bn)
                if tape is not None:
                    tape.append(dict(kind='ct_stage', stage=k, x=x, y1=y1, s1=s1, g1=g1, o1=o1, y2=y2, s2=s2, g2=g2, o2=o2))
            else:
                sc1, sh1 = folded_bn(self._cache, cm.bn)
                sc2, sh2 = folded_bn(self._cache, dm.bn)
                o1 = ops.conv2d(x, packed_conv(self._cache, cm.conv), scale=sc1, bias=sh1, relu=True)
                o2 = ops.deconv4x4s2(o1, self.deconv_pack(dm), scale=sc2, bias=sh2, relu=True)
            x = o2
        if x.shape[-1] != self.out_channels:      # the last stage ran at its padded pitch: the real channels
            x = x[..., :self.out_channels].contiguous()
        return x

    def run_outputs(self, lat, src=None, lazy=True, tape=None, out_b8=False):
        """The necks' common signature behind the boundary the autograd bridge cuts at: here the neck's output itself, nothing follows."""
        assert src is None and len(lat) == 1
        return list(lat)

    def forward(self, inputs):
        return (ops.as_nchw(self.forward_lazy(inputs)[0]),)

    def forward_lazy(self, inputs, tape=None, out_b8=False):
        """-> [the MATERIALISED NHWC map].  tape: the records of ``run``, the first one also holding ``n_in`` = len(inputs) (the gradient
        goes to the last input).  out_b8: accepted for the necks' common signature."""
        assert isinstance(inputs, (list, tuple))
        out = self.run(ops.neck_input(inputs[-1]), tape)
        if tape:
            tape[0]['n_in'] = len(inputs)
        return [out]
