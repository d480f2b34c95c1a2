"""FPN neck with the fork's ``num_outs`` < #levels behaviour (T/mmdet/models/necks/fpn.py:67-218; fork edits
at :96,134,193): every lateral 1x1 conv + GN and the whole top-down nearest-upsample chain run, but only the
first ``num_outs`` 3x3 output convs exist.  GroupNorm-apply and the top-down add are ONE fused pass per level.

``num_outs`` > #levels (fpn.py:146-164, 195-217): the extra pyramid levels are stride-2 3x3 conv + GN modules appended to
``fpn_convs`` (``add_extra_convs`` 'on_input' / 'on_lateral' / 'on_output'), or ``F.max_pool2d(outs[-1], 1, stride=2)`` without
them (ops.subsample2)."""
import warnings

import torch.nn as nn

from .. import ops
from ..layers import ConvModule, _PackCache, conv_gn
from ..registry import NECKS


@NECKS.register_module()
class FPN(nn.Module):
    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False,
                 extra_convs_on_inputs=True, relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None,
                 norm_cfg=None, act_cfg=None, upsample_cfg=dict(mode='nearest'), init_cfg=None):
        super().__init__()
        assert isinstance(in_channels, (list, tuple))
        assert norm_cfg is not None and norm_cfg['type'] == 'GN' and not no_norm_on_lateral and act_cfg is None, \
            'the CPR/P2P configs use GN laterals without activation (SURVEY.md §8 a2)'
        assert upsample_cfg.get('mode', 'nearest') == 'nearest' and 'scale_factor' not in upsample_cfg
        self.in_channels, self.out_channels, self.num_outs = list(in_channels), out_channels, num_outs
        self.num_ins = len(in_channels)
        self.backbone_end_level = self.num_ins if end_level == -1 else end_level
        self.start_level, self.end_level = start_level, end_level
        self.relu_before_extra_convs = relu_before_extra_convs
        if end_level != -1:     # if end_level < inputs, no extra level is allowed (fpn.py:98-101)
            assert end_level <= len(in_channels)
            assert num_outs <= end_level - start_level, 'extra pyramid levels need end_level == -1'
        assert isinstance(add_extra_convs, (str, bool))
        if isinstance(add_extra_convs, str):
            assert add_extra_convs in ('on_input', 'on_lateral', 'on_output')
        elif add_extra_convs:   # True (fpn.py:109-118)
            if extra_convs_on_inputs:
                warnings.warn("add_extra_convs=True with extra_convs_on_inputs is deprecated: pass add_extra_convs='on_input'",
                              DeprecationWarning)
                add_extra_convs = 'on_input'
            else:
                add_extra_convs = 'on_output'
        self.add_extra_convs = add_extra_convs
        self.lateral_convs = nn.ModuleList()
        self.fpn_convs = nn.ModuleList()
        for i in range(start_level, self.backbone_end_level):
            self.lateral_convs.append(ConvModule(in_channels[i], out_channels, 1, norm_cfg=norm_cfg, act_cfg=None))
            if i < start_level + num_outs:  # fork change (fpn.py:134)
                self.fpn_convs.append(ConvModule(out_channels, out_channels, 3, padding=1, norm_cfg=norm_cfg,
                                                 act_cfg=None))
        # extra pyramid levels (fpn.py:146-164): conv modules under the next fpn_convs indices, or max-pool levels without parameters
        self.extra_levels = max(0, num_outs - self.backbone_end_level + start_level)
        if self.add_extra_convs:
            for k in range(self.extra_levels):
                cin = in_channels[self.backbone_end_level - 1] if k == 0 and self.add_extra_convs == 'on_input' else out_channels
                self.fpn_convs.append(ConvModule(cin, out_channels, 3, stride=2, padding=1, norm_cfg=norm_cfg, act_cfg=None))
        self._cache = _PackCache()
        self.init_weights()

    def init_weights(self):
        """init_cfg=dict(type='Xavier', layer='Conv2d', distribution='uniform') (fpn.py:81-82): Xavier-uniform conv
        weights, zero biases; GroupNorm keeps weight 1 / bias 0."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def run_laterals(self, xs, tape=None):
        """xs: the NHWC stage outputs from ``start_level`` on -> the top-down lateral sums, finest first (fpn.py:166-188)."""
        c = self._cache
        # top-down: coarsest level first; GN-apply of level i and "+= upsample(level i+1)" in one kernel
        lat = [None] * len(xs)
        for i in range(len(xs) - 1, -1, -1):
            up = lat[i + 1] if i + 1 < len(xs) else None
            rec = None
            if tape is not None:
                rec = dict(kind='lateral', level=i)
                tape.append(rec)
            lat[i] = conv_gn(c, self.lateral_convs[i], xs[i], up=up, save=rec)
        return lat

    def run_outputs(self, lat, src, lazy, tape=None, out_b8=False):
        """The lateral sums ``lat`` (finest first; at least the ones the output convs read) and, for 'on_input' extra levels, the last
        backbone map ``src`` -> every output level: lazy (raw, (a, b)) pairs, else materialised maps.  tape: training records -- kind
        'out' (fpn_convs[level]), then the extra levels' own (run_extras)."""
        c, outs = self._cache, []
        for i in range(min(len(lat), self.num_outs)):
            rec = None
            if tape is not None:
                rec = dict(kind='out', level=i)
                tape.append(rec)
            outs.append(conv_gn(c, self.fpn_convs[i], lat[i], materialize=not lazy, save=rec,
                                out_b8=out_b8 and lazy and not self.extra_levels))
        if self.extra_levels:
            assert len(lat) == len(self.lateral_convs) and (src is not None) == (self.add_extra_convs == 'on_input')
            outs += self.run_extras(outs[-1], lat[-1], src, lazy, tape)
        return outs

    def _run(self, inputs, lazy, tape=None, out_b8=False):
        assert len(inputs) == len(self.in_channels)
        # (ops.neck_input: a backbone map kept at a padded channel pitch -- RegNet -- is read in place by a pack with zero columns)
        xs = [ops.neck_input(inputs[i + self.start_level]) for i in range(len(self.lateral_convs))]
        lat = self.run_laterals(xs, tape)
        src = None
        if self.extra_levels and self.add_extra_convs == 'on_input':
            src = ops.neck_input(inputs[self.backbone_end_level - 1])
        return self.run_outputs(lat, src, lazy, tape, out_b8)

    def run_extras(self, last, lat_last, src, lazy, tape=None):
        """The extra pyramid levels (fpn.py:195-217) behind the last regular output ``last`` (lazy: (raw, (a, b)), else the
        materialised map), the coarsest lateral sum ``lat_last`` and, for 'on_input', the last backbone map ``src`` -> their
        outputs in ``last``'s form.  Max-pool levels are pure selections, which commute with the per-(image, channel) affine:
        a lazy level is the subsampled raw map with its producer's affine.  An extra conv has stride 2, where no conv kernel
        applies a pending affine on load: it reads the materialised map (with the ReLU of ``relu_before_extra_convs`` from the
        second extra conv on)."""
        c, outs, used = self._cache, [], len(self.lateral_convs)
        if not self.add_extra_convs:
            for k in range(self.extra_levels):
                if tape is not None:
                    tape.append(dict(kind='pool', level=used + k))
                if lazy:
                    last = (ops.subsample2(last[0]), last[1])
                else:
                    last = ops.subsample2(last)
                outs.append(last)
            return outs
        cur = None      # the previous extra conv's (raw, (a, b))
        for k in range(self.extra_levels):
            relu = k > 0 and self.relu_before_extra_convs
            reads = self.add_extra_convs if k == 0 else 'on_output'
            if reads == 'on_input':
                x = src
            elif reads == 'on_lateral':
                x = lat_last
            elif k == 0 and not lazy:
                x = last
            else:
                raw, (a, b) = last if k == 0 else cur
                x = ops.gn_apply(raw, a, b, relu=relu)
            rec = None
            if tape is not None:
                rec = dict(kind='extra', level=used + k, reads=reads, relu_in=relu)
                tape.append(rec)
            cur = conv_gn(c, self.fpn_convs[used + k], x, materialize=False, save=rec)
            outs.append(cur if lazy else ops.gn_apply(cur[0], cur[1][0], cur[1][1]))
        return outs

    def forward(self, inputs):
        return tuple(ops.as_nchw(t) for t in self._run(inputs, lazy=False))

    def forward_lazy(self, inputs, tape=None, out_b8=False):
        """Internal fast path: per level (raw conv output NHWC, (a, b)) -- the consumer conv applies the GroupNorm
        affine while loading (no activation after the FPN convs: act_cfg=None).  tape: training records.
        out_b8: the consumer is a Winograd 3x3 layer (CPRHead tower) -- raw outputs channel-blocked where the layer can."""
        return self._run(inputs, lazy=True, tape=tape, out_b8=out_b8 and tape is None)
