"""BFP neck, the Balanced Feature Pyramid of Libra R-CNN (T/mmdet/models/necks/bfp.py:32-101), and the list-valued neck it comes in:
``neck=[dict(type='FPN' | 'PAFPN', ...), dict(type='BFP', ...)]`` (``NeckSequence``, the reference's ``Sequential``).

With r = ``refine_level`` and (h, w) the size of level r:
  gather    bsf = mean_i feat_i; feat_i = adaptive_max_pool2d(level_i, (h, w)) for i < r, nearest(level_i, (h, w)) for i >= r
  refine    None | 'conv': ConvModule(C, C, 3, padding=1, norm_cfg) = conv -> GN -> ReLU (ConvModule's default activation)
  scatter   out_i = residual_i + level_i; residual_i = nearest(bsf, size_i) for i < r, adaptive_max_pool2d(bsf, size_i) for i >= r
Gather and scatter are ONE launch each over all levels (ops.bfp_gather / ops.bfp_scatter, csrc/bfp.hip).  The levels arrive as the inner
neck's lazy outputs -- raw conv outputs with their pending GroupNorm affines -- and are never materialised on their own: both passes apply
the affine on load.  The refine layer's GroupNorm + ReLU is applied by the scatter on load as well, so it has no apply pass either."""
import torch
import torch.nn as nn

from .. import ops
from ..layers import ConvModule, _PackCache, conv_gn
from ..registry import NECKS
from .fpn import FPN


@NECKS.register_module()
class BFP(nn.Module):
    def __init__(self, in_channels, num_levels, refine_level=2, refine_type=None, conv_cfg=None, norm_cfg=None,
                 init_cfg=dict(type='Xavier', layer='Conv2d', distribution='uniform')):
        super().__init__()
        assert refine_type in [None, 'conv', 'non_local']
        if refine_type == 'non_local':
            raise NotImplementedError("BFP refine_type='non_local' is not built: mmcv's NonLocal2d is not part of this project, so its "
                                      "arithmetic cannot be pinned (refine_type None and 'conv' are)")
        if conv_cfg is not None and conv_cfg.get('type') not in (None, 'Conv2d'):
            raise NotImplementedError('BFP conv_cfg=%r is not built: the refine layer is a plain Conv2d' % (conv_cfg,))
        if refine_type == 'conv' and (norm_cfg is None or norm_cfg.get('type') != 'GN'):
            raise NotImplementedError("BFP refine_type='conv' with norm_cfg=%r is not built: the necks here are GroupNorm-only "
                                      "(norm_cfg=dict(type='GN', num_groups=...))" % (norm_cfg,))
        assert 1 <= num_levels <= ops.BFP_MAX_LEVELS, 'BFP takes 1 .. %d levels (num_levels=%d)' % (ops.BFP_MAX_LEVELS, num_levels)
        assert 0 <= refine_level < num_levels
        self.in_channels, self.num_levels = in_channels, num_levels
        self.conv_cfg, self.norm_cfg = conv_cfg, norm_cfg
        self.refine_level, self.refine_type = refine_level, refine_type
        if refine_type == 'conv':
            self.refine = ConvModule(in_channels, in_channels, 3, padding=1, conv_cfg=conv_cfg, norm_cfg=norm_cfg)
        self._cache = _PackCache()
        self.init_weights()

    init_weights = FPN.init_weights

    def run(self, levels, tape=None):
        """levels: per level a materialised NHWC map or the (raw, (a, b)) of a lazy neck output -> the materialised NHWC outputs.
        tape: training records -- kind 'bfp_gather' (the levels, the argmax record), 'bfp_refine' (the refine layer's, layers.conv_gn),
        'bfp_scatter' (the argmax record)."""
        assert len(levels) == self.num_levels, 'BFP(num_levels=%d) got %d levels' % (self.num_levels, len(levels))
        r, rec = self.refine_level, tape is not None
        got = ops.bfp_gather(levels, r, record=rec)
        bsf, gather_args = got if rec else (got, None)
        if rec:
            tape.append(dict(kind='bfp_gather', args=gather_args, shapes=[tuple((l if torch.is_tensor(l) else l[0]).shape) for l in levels]))
        ref_ab = None
        if self.refine_type == 'conv':
            save = None
            if rec:
                save = dict(kind='bfp_refine')
                tape.append(save)
            bsf, ref_ab = conv_gn(self._cache, self.refine, bsf, materialize=False, save=save)
        got = ops.bfp_scatter(levels, r, bsf, ref_ab, record=rec)
        if rec:
            tape.append(dict(kind='bfp_scatter', args=got[1]))
            return got[0]
        return got

    def forward(self, inputs):
        assert len(inputs) == self.num_levels
        return tuple(ops.as_nchw(t) for t in self.run([ops.from_nchw(x) for x in inputs]))


class NeckSequence(nn.Sequential):
    """A list-valued ``neck``: the reference builds ``nn.Sequential`` of the entries (state-dict keys ``neck.0.*``, ``neck.1.*``).
    Built here: [FPN | PAFPN, BFP].  ``inner`` / ``bfp`` name the two; the backward rules (training.py) walk them in reverse."""

    materialised = True         # forward_lazy returns maps, not (raw, (a, b)) pairs

    def __init__(self, *modules):
        kinds = [type(m).__name__ for m in modules]
        if len(modules) != 2 or kinds[0] not in ('FPN', 'PAFPN') or kinds[1] != 'BFP':
            raise NotImplementedError('a list-valued neck is built as [FPN | PAFPN, BFP]; got %s' % kinds)
        inner, bfp = modules
        n_outs = min(len(inner.lateral_convs), inner.num_outs) + inner.extra_levels
        if bfp.in_channels != inner.out_channels or bfp.num_levels != n_outs:
            raise ValueError('BFP(in_channels=%d, num_levels=%d) does not fit the %s in front of it (out_channels=%d, %d output levels)'
                             % (bfp.in_channels, bfp.num_levels, kinds[0], inner.out_channels, n_outs))
        super().__init__(*modules)

    @property
    def inner(self):
        return self[0]

    @property
    def bfp(self):
        return self[1]

    # the backbone levels it reads and the number of its outputs are the inner neck's
    start_level = property(lambda self: self.inner.start_level)
    backbone_end_level = property(lambda self: self.inner.backbone_end_level)
    num_outs = property(lambda self: self.inner.num_outs)

    def forward(self, inputs):
        return tuple(ops.as_nchw(t) for t in self.forward_lazy(inputs))

    def forward_lazy(self, inputs, tape=None, out_b8=False):
        """-> the MATERIALISED NHWC levels (the scatter writes them): a consumer has no pending affine to apply.  tape: the inner
        neck's records followed by BFP's.  out_b8: accepted for the necks' common signature; the levels are plain NHWC."""
        return self.bfp.run(self.inner.forward_lazy(inputs, tape=tape), tape)

    def run_laterals(self, xs, tape=None):
        return self.inner.run_laterals(xs, tape)

    def run_outputs(self, lat, src, lazy, tape=None, out_b8=False):
        """The inner neck's lazy outputs behind its lateral sums (never materialised: BFP applies their affines on load), then BFP, on
        one tape -> the materialised NHWC levels, as forward_lazy.  out_b8: accepted for the common signature, as there."""
        assert lazy, 'BFP reads the inner neck\'s lazy outputs (forward and forward_lazy both do)'
        return self.bfp.run(self.inner.run_outputs(lat, src, lazy, tape), tape)
