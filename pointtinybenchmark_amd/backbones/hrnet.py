"""HRNet backbone (T/mmdet/models/backbones/hrnet.py): a stem of two 3x3 / 2 convs, ``layer1``, then three stages of HRModules --
parallel branches of residual blocks at resolutions 1/4, 1/8, 1/16, 1/32 that exchange their maps after every module:
    x_fuse[i] = ReLU(sum_j f_ij(x_j)),  f_ii = identity, f_ij (j > i) = nearest-upsample(BN(conv1x1(x_j))),
                                         f_ij (j < i) = a chain of i - j convs 3x3 / 2 + BN (ReLU between them).
``transition{1,2,3}`` open a stage: a 3x3 conv where an existing branch changes its width, a chain of 3x3 / 2 convs for a new branch
(read from the previous stage's LAST branch), nothing otherwise.  State-dict keys, order and shapes are the reference's.

The blocks are resnet._Block with folded eval-mode BatchNorm; the stem's conv2, the transitions, the down chains and the fuse 1x1
convs run on ops.conv2d with the folded BN (and the ReLU where the reference has one) in the epilogue, a fuse 1x1 conv at its own,
coarse, resolution.  The exchange itself -- upsample, sum in the reference's order (source branch ascending), ReLU -- is one launch per
output branch (ops.hrnet_fuse, csrc/hrnet.hip).  conv1 (3 -> 64) runs on the dense kernel's 4-channel mode over the NHWC4 image.
Maps are NHWC fp32; ``forward`` returns NCHW views (ops.as_nchw) that the necks read in place.

Built: widths ``num_channels[b] * expansion`` that are multiples of 32 (HRNetV2p-W32), at most four branches, plain Conv2d, BN / SyncBN
modules in eval mode (norm_eval=True or model.eval()), the fp32 compute mode.  Everything else raises NotImplementedError naming its
key.  A stage may change the width of the LAST branch of the stage before it (a same-resolution 3x3 transition on that branch); changing
any other existing branch is refused: the reference's forward feeds every transition the last branch (hrnet.py:541, :549) and fails there.  The recorded forward (``tape=``) feeds
training.BackwardEngine._backward_hrnet."""
import torch
import torch.nn as nn

from .. import ops
from ..layers import _PackCache, bump_weight_epoch, folded_bn, packed_conv
from ..registry import BACKBONES
from .resnet import _Block

_BatchNorm = nn.modules.batchnorm._BatchNorm

_BATCH_STATS = 'BatchNorm batch statistics in an HRNet backbone (norm_eval=False in training mode): its blocks, transitions and fuse ' \
    'layers run with eval-mode BatchNorm only -- keep norm_eval=True'
_KINDS = {'BASIC': ('basic', 1), 'BOTTLENECK': ('bottleneck', 4)}
MAX_BRANCHES = 4


def unsupported_reason(extra, conv_cfg=None, norm_cfg=dict(type='BN'), with_cp=False):
    """None when the kernels take this setting, else why not, naming the key."""
    if with_cp:
        return 'with_cp=True is not built (SURVEY.md §2a row 5)'
    if conv_cfg is not None and conv_cfg.get('type') not in (None, 'Conv2d'):
        return 'conv_cfg=%r is not built: plain Conv2d layers (conv_cfg=None)' % (conv_cfg,)
    if norm_cfg is None or norm_cfg.get('type') not in ('BN', 'SyncBN'):
        return "norm_cfg type %r is not built: the norms are 'BN' (nn.BatchNorm2d) or 'SyncBN' (nn.SyncBatchNorm)" \
            % (None if norm_cfg is None else norm_cfg.get('type'),)
    pre = None
    for s in (1, 2, 3, 4):
        cfg = extra['stage%d' % s]
        if cfg['block'] not in _KINDS:
            return "extra['stage%d']['block']=%r is not built: 'BASIC' or 'BOTTLENECK'" % (s, cfg['block'])
        if cfg['num_branches'] > MAX_BRANCHES:
            return "extra['stage%d']['num_branches']=%d is not built: at most %d branches (the exchange kernel sums up to %d terms)" \
                % (s, cfg['num_branches'], MAX_BRANCHES, MAX_BRANCHES)
        exp = _KINDS[cfg['block']][1]
        widths = [c * exp for c in cfg['num_channels']]
        if any(w % 32 for w in widths):
            return "extra['stage%d']['num_channels']=%r (x expansion %d) is not built: every branch width must be a multiple of 32 -- " \
                "W32-style widths (32, 64, 128, 256) are what is built; W18 / W40 / W48 need padded-pitch blocks" \
                % (s, tuple(cfg['num_channels']), exp)
        if pre is not None and any(a != b for a, b in zip(pre[:-1], widths)):
            return "extra['stage%d']['num_channels']=%r changes the width of a branch other than the last of the stage before it (which " \
                "ends at %r): the reference's forward feeds every transition that stage's LAST branch (hrnet.py:541, :549) and fails on " \
                "the channel count -- only the last existing branch may change its width" % (s, tuple(cfg['num_channels']), tuple(pre))
        pre = widths
    return None


def _conv_bn(cin, cout, k, stride, norm, tail=None):
    """Sequential(conv ``0``, norm ``1``[, tail ``2``]): the reference's indices; ``tail`` (ReLU / Upsample) holds no parameter."""
    mods = [nn.Conv2d(cin, cout, k, stride, k // 2, bias=False), norm(cout)]
    return nn.Sequential(*(mods + ([tail] if tail is not None else [])))


def run_conv_bn(cache, seq, x, relu):
    """conv ``seq[0]`` + folded BN ``seq[1]`` (+ ReLU) on an NHWC map."""
    s, b = folded_bn(cache, seq[1])
    return ops.conv2d(x, packed_conv(cache, seq[0]), scale=s, bias=b, relu=relu)


def run_chain(cache, chain, x, last_relu, rec=None):
    """A Sequential of conv-BN Sequentials (a down chain of a fuse layer: ReLU between the convs, ``last_relu`` False; a new branch's
    transition: ReLU after every conv).  rec (list): the input of every conv, then the output."""
    maps = [x]
    for k, seq in enumerate(chain):
        x = run_conv_bn(cache, seq, x, relu=last_relu or k + 1 < len(chain))
        maps.append(x)
    if rec is not None:
        rec.extend(maps)
    return x


class HRModule(nn.Module):
    """hrnet.py:12-199 with multiscale_output=True (what HRNet builds): ``branches`` and ``fuse_layers``."""

    def __init__(self, num_branches, block, num_blocks, in_channels, num_channels, norm):
        super().__init__()
        if num_branches != len(num_blocks):
            raise ValueError('NUM_BRANCHES(%d) != NUM_BLOCKS(%d)' % (num_branches, len(num_blocks)))
        if num_branches != len(num_channels):
            raise ValueError('NUM_BRANCHES(%d) != NUM_CHANNELS(%d)' % (num_branches, len(num_channels)))
        if num_branches != len(in_channels):
            raise ValueError('NUM_BRANCHES(%d) != NUM_INCHANNELS(%d)' % (num_branches, len(in_channels)))
        kind, exp = _KINDS[block]
        self.num_branches, self.in_channels = num_branches, in_channels
        branches = []
        for b in range(num_branches):
            blocks = []
            for k in range(num_blocks[b]):
                ds = None
                if k == 0 and in_channels[b] != num_channels[b] * exp:
                    ds = nn.Sequential(nn.Conv2d(in_channels[b], num_channels[b] * exp, 1, 1, bias=False), norm(num_channels[b] * exp))
                blocks.append(_Block(kind, in_channels[b], num_channels[b], 1, ds, norm))
                in_channels[b] = num_channels[b] * exp
            branches.append(nn.Sequential(*blocks))
        self.branches = nn.ModuleList(branches)
        self.fuse_layers = None
        if num_branches > 1:
            fuse = []
            for i in range(num_branches):
                row = []
                for j in range(num_branches):
                    if j > i:
                        row.append(_conv_bn(in_channels[j], in_channels[i], 1, 1, norm, nn.Upsample(scale_factor=2 ** (j - i), mode='nearest')))
                    elif j == i:
                        row.append(None)
                    else:
                        row.append(nn.Sequential(*[
                            _conv_bn(in_channels[j], in_channels[i], 3, 2, norm) if k == i - j - 1 else
                            _conv_bn(in_channels[j], in_channels[j], 3, 2, norm, nn.ReLU(inplace=False)) for k in range(i - j)]))
                fuse.append(nn.ModuleList(row))
            self.fuse_layers = nn.ModuleList(fuse)
        self.relu = nn.ReLU(inplace=False)

    def fuse_terms(self, cache, i, xs, rec=None):
        """The terms of output branch i in the reference's order, source branch ascending -> [(map, k)] for ops.hrnet_fuse.
        rec (dict): j -> the maps a down chain read and wrote (run_chain)."""
        terms = []
        for j in range(self.num_branches):
            fl = self.fuse_layers[i][j]
            if j == i:
                terms.append((xs[j], 0))
            elif j > i:
                terms.append((run_conv_bn(cache, fl, xs[j], relu=False), j - i))
            else:
                maps = [] if rec is not None else None
                terms.append((run_chain(cache, fl, xs[j], False, maps), 0))
                if rec is not None:
                    rec[j] = maps
        return terms

    def run(self, cache, xs, rec=None):
        """xs: one NHWC map per branch -> the exchanged maps.  rec (dict): ``blocks`` (per branch the block records), ``x`` (the branch
        chains' outputs, the fuse inputs), ``chains`` (per output branch: j -> a down chain's maps), ``out`` (the fuse outputs)."""
        assert len(xs) == self.num_branches
        outs, brecs = [], []
        for b, branch in enumerate(self.branches):
            x, recs = xs[b], []
            for blk in branch:
                r = {} if rec is not None else None
                x = blk.run(cache, x, r)
                recs.append(r)
            outs.append(x)
            brecs.append(recs)
        if self.fuse_layers is None:
            fused, chains = outs, []
        else:
            fused, chains = [], []
            for i in range(self.num_branches):
                ch = {} if rec is not None else None
                fused.append(ops.hrnet_fuse(self.fuse_terms(cache, i, outs, ch), outs[i].shape[1:3]))
                chains.append(ch)
        if rec is not None:
            rec.update(module=self, blocks=brecs, x=outs, chains=chains, out=fused)
        return fused


def branch_sizes(H, W, n):
    """The (H, W) of branches 0 .. n-1 for an image of (H, W), by conv arithmetic: conv1 and conv2 (3x3 / 2, padding 1), then one
    3x3 / 2 per branch step."""
    def half(v):
        return (v - 1) // 2 + 1
    h, w = half(half(H)), half(half(W))
    sizes = []
    for _ in range(n):
        sizes.append((h, w))
        h, w = half(h), half(w)
    return sizes


@BACKBONES.register_module()
class HRNet(nn.Module):
    """HRNet (hrnet.py:202-564).  ``extra``: stage1 .. stage4, each num_modules, num_branches, block, num_blocks, num_channels."""
    hrnet = True      # training.BackwardEngine walks a DAG of branches for this backbone (_backward_hrnet), autograd_bridge one Function

    def __init__(self, extra, in_channels=3, conv_cfg=None, norm_cfg=dict(type='BN'), norm_eval=True, with_cp=False,
                 zero_init_residual=False, pretrained=None, init_cfg=None):
        super().__init__()
        assert not (init_cfg and pretrained), 'init_cfg and pretrained cannot be setting at the same time'
        if not (pretrained is None or isinstance(pretrained, str)):
            raise TypeError('pretrained must be a str or None')
        reason = unsupported_reason(extra, conv_cfg, norm_cfg, with_cp)
        if reason is not None:
            raise NotImplementedError('HRNet ' + reason)
        if in_channels != 3:
            raise NotImplementedError('HRNet in_channels=%r is not built: conv1 reads the three-channel image (in_channels=3)' % (in_channels,))
        bn_kw = {'momentum': norm_cfg['momentum']} if 'momentum' in norm_cfg else {}
        norm_cls = nn.SyncBatchNorm if norm_cfg['type'] == 'SyncBN' else nn.BatchNorm2d
        rg = norm_cfg.get('requires_grad', True)

        def norm(c):
            m = norm_cls(c, **bn_kw)
            for p in m.parameters():
                p.requires_grad = rg
            return m
        self.extra, self.conv_cfg, self.norm_cfg, self.norm_eval = extra, conv_cfg, norm_cfg, norm_eval
        self.with_cp, self.zero_init_residual, self.pretrained, self.init_cfg = with_cp, zero_init_residual, pretrained, init_cfg
        self.fp32_only = "an HRNet backbone (extra=...) runs in the fp32 compute mode only: its 32-channel branch cannot feed the bf16 " \
            "kernels (64-channel chunks)"
        self.conv1 = nn.Conv2d(in_channels, 64, 3, 2, 1, bias=False)
        self.bn1 = norm(64)
        self.conv2 = nn.Conv2d(64, 64, 3, 2, 1, bias=False)
        self.bn2 = norm(64)
        self.relu = nn.ReLU(inplace=True)
        # stage 1
        self.stage1_cfg = extra['stage1']
        kind, exp = _KINDS[self.stage1_cfg['block']]
        planes, blocks = self.stage1_cfg['num_channels'][0], self.stage1_cfg['num_blocks'][0]
        layer, inplanes = [], 64
        for k in range(blocks):
            ds = None
            if k == 0 and inplanes != planes * exp:
                ds = nn.Sequential(nn.Conv2d(inplanes, planes * exp, 1, 1, bias=False), norm(planes * exp))
            layer.append(_Block(kind, inplanes, planes, 1, ds, norm))
            inplanes = planes * exp
        self.layer1 = nn.Sequential(*layer)
        pre = [inplanes]
        for s in (2, 3, 4):
            cfg = extra['stage%d' % s]
            setattr(self, 'stage%d_cfg' % s, cfg)
            exp = _KINDS[cfg['block']][1]
            cur = [c * exp for c in cfg['num_channels']]
            if len(cur) < len(pre):
                raise ValueError("extra['stage%d'] has %d branches, fewer than the %d of the stage before it" % (s, len(cur), len(pre)))
            setattr(self, 'transition%d' % (s - 1), self._make_transition_layer(pre, cur, norm))
            mods, inch = [], list(cur)
            for _ in range(cfg['num_modules']):
                mods.append(HRModule(cfg['num_branches'], cfg['block'], cfg['num_blocks'], inch, cfg['num_channels'], norm))
            setattr(self, 'stage%d' % s, nn.Sequential(*mods))
            pre = inch
        self.out_channels = list(pre)
        self.feat_dim = pre[-1]
        self.compute_dtype = torch.float32
        self._cache = _PackCache()
        self.init_weights()

    @staticmethod
    def _make_transition_layer(pre, cur, norm):      # hrnet.py:387-431
        layers = []
        for i in range(len(cur)):
            if i < len(pre):
                layers.append(_conv_bn(pre[i], cur[i], 3, 1, norm, nn.ReLU(inplace=True)) if cur[i] != pre[i] else None)
            else:
                layers.append(nn.Sequential(*[
                    _conv_bn(pre[-1], cur[i] if j == i - len(pre) else pre[-1], 3, 2, norm, nn.ReLU(inplace=True))
                    for j in range(i + 1 - len(pre))]))
        return nn.ModuleList(layers)

    @property
    def norm1(self):
        return self.bn1

    @property
    def norm2(self):
        return self.bn2

    def init_weights(self):
        """The reference's default init_cfg (hrnet.py:287-294): Kaiming normal (fan_out, relu) on every conv, constant 1 on every norm
        (bias 0); zero_init_residual: weight 0 on the last norm of every block."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, _BatchNorm):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if self.zero_init_residual:
            for m in self.modules():
                if isinstance(m, _Block):
                    nn.init.constant_((m.bn2 if m.kind == 'basic' else m.bn3).weight, 0)
        bump_weight_epoch()

    def train(self, mode=True):      # hrnet.py:556-564
        super().train(mode)
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, _BatchNorm):
                    m.eval()
        return self

    # ---------------------------------------------------------------------------------------------- structure
    def stages(self):
        """[(transition ModuleList, stage Sequential of HRModules)] for stages 2, 3, 4."""
        return [(getattr(self, 'transition%d' % (s - 1)), getattr(self, 'stage%d' % s)) for s in (2, 3, 4)]

    def stem_parameters(self):
        return list(self.conv1.parameters()) + list(self.bn1.parameters()) + list(self.conv2.parameters()) + list(self.bn2.parameters())

    def stem_train_reason(self):
        """None: conv1 / bn1 / conv2 / bn2 have backward rules (BackwardEngine._backward_hrnet)."""
        return None

    def freeze_reason(self):
        """None when the frozen parameters form sets the folded conv -> BN backward rule serves, else why not, naming the pair.  That
        rule (training.BackwardEngine._folded_param_grads) writes the gradients of a conv and of the BatchNorm behind it from one pass,
        skips the pass for a frozen conv and writes the norm's two gradients together: a pair trains or is frozen as a whole, or the
        conv trains under a wholly frozen norm (norm_cfg requires_grad=False).  A trainable norm behind a frozen conv, or a norm with
        one of weight / bias frozen, would be left without its gradient."""
        conv = None
        for name, m in self.named_modules():
            if isinstance(m, nn.Conv2d):
                conv = (name, m)
            elif isinstance(m, _BatchNorm):
                cw, g, b = conv[1].weight.requires_grad, m.weight.requires_grad, m.bias.requires_grad
                if g != b or (g and not cw):
                    return 'HRNet: %s.weight, %s.weight and %s.bias have requires_grad = %s, %s, %s: a conv and the BatchNorm behind it ' \
                        'train or are frozen together (or the conv trains under a frozen norm) -- their gradients come from one pass' \
                        % (conv[0], name, name, cw, g, b)
        return None

    def batch_stats_active(self):
        return self.training and any(m.training for m in self.modules() if isinstance(m, _BatchNorm))

    def _check_mode(self):
        if self.compute_dtype != torch.float32:
            raise NotImplementedError(self.fp32_only)
        if self.batch_stats_active():
            raise NotImplementedError(_BATCH_STATS)

    def check_size(self, H, W):
        """The reference's ``y += upsample(..)`` raises unless branch j times 2^(j-i) is branch i exactly: checked up front."""
        sizes = branch_sizes(H, W, len(self.out_channels))
        for i, (hi, wi) in enumerate(sizes):
            for j in range(i + 1, len(sizes)):
                hj, wj = sizes[j]
                if (hj << (j - i), wj << (j - i)) != (hi, wi):
                    raise ValueError('HRNet: an image of %d x %d gives branch %d a %d x %d map and branch %d a %d x %d map, which is not '
                                     'branch %d divided by %d exactly (the exchange upsamples by %d); sizes divisible by 32 always pass'
                                     % (H, W, i, hi, wi, j, hj, wj, i, 1 << (j - i), 1 << (j - i)))
        return sizes

    # ---------------------------------------------------------------------------------------------- forward
    def run_stem(self, x, tape=None):
        """(N,3,H,W) image -> the NHWC map (N, H/4, W/4, 64) after conv1 + bn1 + ReLU and conv2 + bn2 + ReLU.  tape (dict): the NHWC4
        image conv1 read, conv1's output and conv2's."""
        self._check_mode()
        c = self._cache
        x4 = ops.from_nchw(x) if (x.shape[1] == 4 and x.stride(1) == 1) else ops.nchw_to_nhwc(x)
        s1, b1 = folded_bn(c, self.bn1)
        o1 = ops.conv2d(x4, packed_conv(c, self.conv1), scale=s1, bias=b1, relu=True)
        s2, b2 = folded_bn(c, self.bn2)
        o2 = ops.conv2d(o1, packed_conv(c, self.conv2), scale=s2, bias=b2, relu=True)
        if tape is not None:
            tape.update(x4=x4, o1=o1, o2=o2)
        return o2

    def run(self, img, tape=None):
        """(N,3,H,W) image -> the NHWC branch outputs of stage4's last module.  tape (list): one record (``hrnet=True``) is appended --
        ``stem``, ``layer1`` (block records), ``stages``: per stage ``trans`` (per branch None or the maps of its transition chain,
        run_chain) and ``modules`` (HRModule.run's records)."""
        self._check_mode()
        self.check_size(img.shape[-2], img.shape[-1])
        c = self._cache
        rec = None
        if tape is not None:
            rec = dict(hrnet=True, stem={}, layer1=[], stages=[])
            tape.append(rec)
        x = self.run_stem(img, rec['stem'] if rec is not None else None)
        for blk in self.layer1:
            r = {} if rec is not None else None
            x = blk.run(c, x, r)
            if rec is not None:
                rec['layer1'].append(r)
        ys = [x]
        for trans, stage in self.stages():
            xs, trecs = [], []
            for i, t in enumerate(trans):
                maps = None
                if t is None:
                    xs.append(ys[i])
                else:
                    # (every transition reads the previous stage's last branch, hrnet.py:533, :541, :549: a new branch's chain, or the
                    # same-resolution conv of that very branch when it changes its width -- unsupported_reason admits no other)
                    maps = [] if rec is not None else None
                    xs.append(run_chain(c, [t] if isinstance(t[0], nn.Conv2d) else t, ys[-1], True, maps))
                trecs.append(maps)
            mrecs = []
            for mod in stage:
                r = {} if rec is not None else None
                xs = mod.run(c, xs, r)
                mrecs.append(r)
            if rec is not None:
                rec['stages'].append(dict(trans=trecs, modules=mrecs))
            ys = xs
        return ys

    def forward(self, x, tape=None):
        """x: (N,3,H,W) -> the tuple of branch outputs of the last module of stage4, NCHW views of the NHWC buffers."""
        return tuple(ops.as_nchw(y) for y in self.run(x, tape))
