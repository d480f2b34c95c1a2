"""HRFPN neck, the High-Resolution Feature Pyramid (T/mmdet/models/necks/hrfpn.py:32-99): every input level is brought to the finest
resolution by bilinear interpolation, the levels are concatenated and reduced by ONE 1x1 conv with bias, average pools of the reduced
map make the pyramid, and one 3x3 conv with bias per level writes the outputs.  No norm layer, no activation.

Written as the reference writes it the concatenated map behind a ResNet-50 at 640^2 has 3840 channels at 160 x 160.  Interpolation and
the 1x1 conv are both linear and bilinear weights sum to one, so
    reduction_conv(cat_i(up_i(x_i))) = bias + y_0 + sum_{i>=1} up_i(y_i),   y_i = W_i * x_i at level i's OWN resolution
with W_i the column slice of the reduction weight that belongs to level i.  The 1x1 convs run on the dense / streamed conv kernels at
native resolution; ops.hrfpn_fuse adds the bias and the upsampled y_i in one pass, ops.hrfpn_pool makes every pooled level from that map
in one launch (csrc/hrfpn.hip), and the 3x3 convs are the kernels every other neck uses.  The concatenated map never exists.

``norm_cfg`` is stored and otherwise ignored: the reference never passes it to its ConvModules (hrfpn.py:52-69), so a config that sets it
gets biased convs without a norm layer there and here.

Training (training.py ``_backward_hrfpn_outputs`` / ``_backward_hrfpn_inputs``): the output convs' gradients, ops.hrfpn_pool_bwd (d_out and
the column sums that are the reduction bias gradient), ops.hrfpn_fuse_bwd (dy_i), then per level the 1x1 weight gradient into its column
slice of the reduction weight's gradient and the 1x1 data gradient into the backbone stage.

Not built: ``pooling_type='MAX'``, ``with_cp=True``, a ``conv_cfg`` other than Conv2d."""
import torch
import torch.nn as nn

from .. import ops
from ..layers import ConvModule, _PackCache, _zero_embedded, packed_conv
from ..registry import NECKS


@NECKS.register_module()
class HRFPN(nn.Module):
    materialised = True         # forward_lazy returns maps, not (raw, (a, b)) pairs: no norm follows the output convs

    def __init__(self, in_channels, out_channels, num_outs=5, pooling_type='AVG', conv_cfg=None, norm_cfg=None, with_cp=False, stride=1,
                 init_cfg=dict(type='Caffe2Xavier', layer='Conv2d')):
        super().__init__()
        assert isinstance(in_channels, (list, tuple))
        if pooling_type != 'AVG':
            raise NotImplementedError("HRFPN pooling_type=%r is not built: the pyramid is made by average pooling (pooling_type='AVG')"
                                      % (pooling_type,))
        if with_cp:
            raise NotImplementedError('HRFPN with_cp=True is not built: there is no activation checkpointing on this path')
        if conv_cfg is not None and conv_cfg.get('type') not in (None, 'Conv2d'):
            raise NotImplementedError('HRFPN conv_cfg=%r is not built: its layers are plain Conv2d' % (conv_cfg,))
        if stride not in (1, 2):
            raise NotImplementedError('HRFPN stride=%r is not built: the 3x3 output convs run at stride 1 or 2' % (stride,))
        if not 1 <= len(in_channels) <= ops.HRFPN_MAX_LEVELS:
            raise NotImplementedError('HRFPN in_channels=%r is not built: the fuse kernel takes 1 .. %d inputs'
                                      % (list(in_channels), ops.HRFPN_MAX_LEVELS))
        if not 1 <= num_outs <= ops.HRFPN_MAX_OUTS:
            raise NotImplementedError('HRFPN num_outs=%r is not built: 1 .. %d output levels' % (num_outs, ops.HRFPN_MAX_OUTS))
        if out_channels % 32 != 0:
            raise NotImplementedError('HRFPN out_channels=%r is not built: the 3x3 output convs take a multiple of 32 input channels'
                                      % (out_channels,))
        self.in_channels, self.out_channels = list(in_channels), out_channels
        self.num_ins, self.num_outs = len(in_channels), num_outs
        self.pooling_type, self.with_cp, self.stride = pooling_type, with_cp, stride
        self.conv_cfg, self.norm_cfg, self.init_cfg = conv_cfg, norm_cfg, init_cfg
        self.reduction_conv = ConvModule(sum(in_channels), out_channels, 1, conv_cfg=conv_cfg, act_cfg=None)
        self.fpn_convs = nn.ModuleList(ConvModule(out_channels, out_channels, 3, padding=1, stride=stride, conv_cfg=conv_cfg, act_cfg=None)
                                       for _ in range(num_outs))
        self._cache = _PackCache()
        self.init_weights()

    def init_weights(self):
        """init_cfg=dict(type='Caffe2Xavier', layer='Conv2d') (hrfpn.py:41): mmcv's caffe2_xavier_init restated -- Kaiming uniform with
        a=1, fan_in, leaky_relu -- and zero biases."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1, mode='fan_in', nonlinearity='leaky_relu')
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def _level_pack(self, i, x):
        """The 1x1 pack of level i: the column slice of the reduction weight that belongs to it, at the pitch and dtype of the map x
        (zero columns behind the real channels of a backbone map kept at a padded pitch).  Cached on the reduction weight."""
        c, pitch = self.in_channels[i], x.shape[-1]
        assert pitch == c or (x.dtype == torch.float32 and pitch == ops.pad32(c)), \
            'HRFPN input %d has %d channels, in_channels[%d] = %d' % (i, pitch, i, c)
        return self._cache.get(('hr1x1', i, x.dtype, pitch), [self.reduction_conv.conv.weight],
                               lambda: ops.PackedConv(self.level_weight(i, pitch), 1, 0, x.dtype))

    def level_slice(self, i):
        """(first column, columns) of level i in the reduction weight (out_channels, sum(in_channels), 1, 1)."""
        return sum(self.in_channels[:i]), self.in_channels[i]

    def level_weight(self, i, pitch):
        """Level i's column slice of the reduction weight as a dense (out_channels, pitch, 1, 1) tensor, zero columns in the pad."""
        w = self.reduction_conv.conv.weight
        lo, c = self.level_slice(i)
        ws = w.detach()[:, lo:lo + c].contiguous()
        return ws if pitch == c else _zero_embedded(ws, w.shape[0], pitch)

    def level_dgrad_pack(self, i, pitch):
        """The data-gradient pack of level i's 1x1 conv (training), cached on the reduction weight like the forward pack."""
        return self._cache.get(('hr1x1_dgrad', i, pitch), [self.reduction_conv.conv.weight],
                               lambda: ops.dgrad_pack(self.level_weight(i, pitch), 1, 0))

    def _sizes(self, xs):
        H0, W0 = xs[0].shape[1:3]
        sizes = [tuple(x.shape[1:3]) for x in xs]
        if any((h << i, w << i) != (H0, W0) for i, (h, w) in enumerate(sizes)):
            raise ValueError('HRFPN: level i must be level 0 divided by 2**i exactly (the reference concatenates the levels upsampled '
                             'by 2**i), got sizes %s' % (sizes,))
        if min(H0, W0) >> (self.num_outs - 1) == 0:
            raise ValueError('HRFPN: a %d x %d level 0 leaves output level %d empty (avg_pool2d by %d)'
                             % (H0, W0, self.num_outs - 1, 1 << (self.num_outs - 1)))
        return sizes

    def run_fuse(self, xs, tape=None):
        """xs: the NHWC inputs (ops.neck_input) -> the reduced map ``out`` (N, H0, W0, out_channels): the per-level 1x1 convs and the
        fuse.  tape: one record, kind 'hrfpn_in' -- the inputs and their sizes (the backward's reduction-weight gradient reads them)."""
        assert len(xs) == self.num_ins, 'HRFPN(in_channels=%s) got %d inputs' % (self.in_channels, len(xs))
        sizes = self._sizes(xs)
        ys = [ops.conv2d(x, self._level_pack(i, x)) for i, x in enumerate(xs)]
        if tape is not None:
            tape.append(dict(kind='hrfpn_in', xs=xs, sizes=sizes))
        return ops.hrfpn_fuse(ys, self.reduction_conv.conv.bias)

    def run_outputs(self, lat, src=None, lazy=True, tape=None, out_b8=False):
        """lat: [the reduced map] -> the materialised NHWC outputs: the pooled levels and one biased 3x3 conv each.  tape: one record,
        kind 'hrfpn_out' -- the reduced map and the pooled levels (the output convs' weight gradients read them).  src / lazy / out_b8:
        the necks' common signature; there is no extra source, and no norm whose affine could stay pending."""
        out, = lat
        assert src is None
        levels = [out] + ops.hrfpn_pool(out, self.num_outs)
        if tape is not None:
            tape.append(dict(kind='hrfpn_out', out=out, levels=levels))
        return [ops.conv2d(lv, packed_conv(self._cache, m.conv, lv.dtype), bias=m.conv.bias) for lv, m in zip(levels, self.fpn_convs)]

    def run(self, xs, tape=None):
        """xs: the NHWC inputs -> the materialised NHWC outputs; tape: the two records above."""
        return self.run_outputs([self.run_fuse(xs, tape)], tape=tape)

    def forward(self, inputs):
        return tuple(ops.as_nchw(t) for t in self.forward_lazy(inputs))

    def forward_lazy(self, inputs, tape=None, out_b8=False):
        """-> the MATERIALISED NHWC levels (biased convs without a norm: a consumer has no pending affine to apply).  out_b8: accepted
        for the necks' common signature; the levels are plain NHWC."""
        assert len(inputs) == self.num_ins
        return self.run([ops.neck_input(x) for x in inputs], tape)
