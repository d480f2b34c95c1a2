"""PAFPN neck: FPN plus a bottom-up path (T/mmdet/models/necks/pafpn.py:40-154, Path Aggregation Network).

With L used backbone levels: the laterals and the top-down chain are FPN's; ``inter[i] = fpn_convs[i](lat[i])``; bottom-up
``inter[i+1] += downsample_convs[i](inter[i])`` (3x3 stride 2 + GN); ``out[0] = inter[0]``, ``out[i] = pafpn_convs[i-1](inter[i])`` (3x3 + GN);
the extra levels behind them follow FPN's rules (``FPN.run_extras``).  Both summands of a bottom-up step exist only as a raw conv output
with the pending per-(image, channel) GroupNorm affine of their layer: ONE pass materialises the sum (``ops.gn_apply2``, csrc/pafpn.hip).
``inter[0]`` has two consumers -- it is the finest output, and the stride-2 ``downsample_convs[0]`` reads it (no conv kernel applies a
pending affine at stride 2, layers.conv_gn) -- so it is materialised by ``ops.gn_apply`` while the lazy output keeps its (raw, (a, b))."""
import torch.nn as nn

from .. import ops
from ..layers import ConvModule, conv_gn
from ..registry import NECKS
from .fpn import FPN


@NECKS.register_module()
class PAFPN(FPN):
    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False,
                 extra_convs_on_inputs=True, relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None,
                 norm_cfg=None, act_cfg=None, init_cfg=dict(type='Xavier', layer='Conv2d', distribution='uniform')):
        levels = (len(in_channels) if end_level == -1 else end_level) - start_level
        assert num_outs >= levels, 'PAFPN needs num_outs >= the %d used backbone levels (num_outs=%d): every level has an output conv ' \
            '(the reference indexes fpn_convs[i] for each of them, pafpn.py:115-117)' % (levels, num_outs)
        super().__init__(in_channels, out_channels, num_outs, start_level, end_level, add_extra_convs, extra_convs_on_inputs,
                         relu_before_extra_convs, no_norm_on_lateral, conv_cfg, norm_cfg, act_cfg, init_cfg=init_cfg)
        # the bottom-up pathway (pafpn.py:69-93)
        self.downsample_convs = nn.ModuleList()
        self.pafpn_convs = nn.ModuleList()
        for _ in range(self.start_level + 1, self.backbone_end_level):
            self.downsample_convs.append(ConvModule(out_channels, out_channels, 3, stride=2, padding=1, norm_cfg=norm_cfg, act_cfg=None))
            self.pafpn_convs.append(ConvModule(out_channels, out_channels, 3, padding=1, norm_cfg=norm_cfg, act_cfg=None))
        self.init_weights()

    def run_outputs(self, lat, src, lazy, tape=None, out_b8=False):
        """The lateral sums ``lat`` (finest first; FPN.run_laterals) and, for 'on_input' extra levels, the last backbone map ``src`` ->
        every output level: lazy (raw, (a, b)) pairs, else materialised maps.  tape: training records -- kind 'out' (fpn_convs[level]),
        'down' (downsample_convs[level]: inter[level] -> its share of inter[level + 1]), 'pa_out' (pafpn_convs[level - 1]), then the
        extra levels' own."""
        if not len(self.downsample_convs):      # one used level: no bottom-up module, FPN itself
            return super().run_outputs(lat, src, lazy, tape, out_b8)
        c, L = self._cache, len(lat)
        assert L == len(self.lateral_convs) and L > 1

        def rec(kind, level):
            if tape is None:
                return None
            tape.append(dict(kind=kind, level=level))
            return tape[-1]
        inter = [conv_gn(c, self.fpn_convs[i], lat[i], materialize=False, save=rec('out', i)) for i in range(L)]
        raw, (a, b) = inter[0]
        keep = lazy or tape is not None        # somebody still reads the raw map: the lazy output, the backward
        cur = ops.gn_apply(raw, a, b, out=None if keep else raw)
        outs = [inter[0] if lazy else cur]
        for i in range(L - 1):
            draw, (da, db) = conv_gn(c, self.downsample_convs[i], cur, materialize=False, save=rec('down', i))
            raw, (a, b) = inter[i + 1]
            cur = ops.gn_apply2(raw, a, b, draw, da, db, out=None if tape is not None else raw)
            outs.append(conv_gn(c, self.pafpn_convs[i], cur, materialize=not lazy, save=rec('pa_out', i + 1)))
        if self.extra_levels:
            outs += self.run_extras(outs[-1], lat[-1], src, lazy, tape)
        return outs
