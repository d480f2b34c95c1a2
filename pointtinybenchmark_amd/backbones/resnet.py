"""ResNet backbone on the fp32-MFMA implicit-GEMM conv kernel.

Interface of T/mmdet/models/backbones/resnet.py:305-657 (ctor kwargs, ``forward(x) -> tuple`` of the
``out_indices`` stage outputs, ``frozen_stages`` / ``norm_eval`` train() semantics, state-dict keys).
BatchNorm in eval mode (norm_eval=True, every CPR/P2P config; or model.eval()) uses running statistics and is folded into the
conv epilogue; the bottleneck shortcut add + ReLU are fused into conv3's epilogue.  With norm_eval=False the BatchNorm modules of the
non-frozen stages are in training mode (the reference's ``train()``) and normalise with batch statistics: raw conv, statistics pass,
normalise / residual / ReLU pass (csrc/bn_train.hip), running statistics updated on the device.  norm_cfg type 'SyncBN' (or
torch.nn.SyncBatchNorm.convert_sync_batchnorm) builds nn.SyncBatchNorm modules -- same names and state-dict keys -- whose batch statistics
run over the rows of every rank of their process group (``sync_group``); on one rank they are BatchNorm bit for bit.
``dilations[i] > 1`` in a stage with ``strides[i] == 1`` (DC5: strides (1, 2, 2, 1), dilations (1, 1, 1, 2)) puts every block's 3x3 of that stage
at padding = dilation (resnet.py:36-47, 175-200), on the dilated instances of the direct conv kernels (fp32 compute mode; ops.PackedConv
``dilation``); a stage that is dilated and strided is refused.
The backward of the trainable stages -- and of a trainable stem (frozen_stages=-1) -- is driven by training.CprTrainer from the records
of ``forward(tape=)``."""
import math

import torch
import torch.nn as nn

from .. import ops
from ..layers import _PackCache, folded_bn, folded_bn_padded, packed_conv, packed_conv_padded
from ..registry import BACKBONES


_BatchNorm = nn.modules.batchnorm._BatchNorm      # BatchNorm2d and SyncBatchNorm (T/mmdet/models/backbones/resnet.py:7, :655)


def sync_group(bn):
    """The process group a BatchNorm module synchronises its batch statistics over in the next forward, or None: an nn.SyncBatchNorm in
    training mode, torch.distributed initialised, and more than one rank in ``bn.process_group`` (None: the world group) -- torch's
    ``need_sync`` rule."""
    if not (isinstance(bn, nn.SyncBatchNorm) and bn.training):
        return None
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return None
    group = bn.process_group if bn.process_group is not None else dist.group.WORLD
    return group if dist.get_world_size(group) > 1 else None


def _grouped_not_mixed(groups):
    return NotImplementedError('a grouped backbone (ResNeXt groups=%d) runs in the fp32 compute mode only: the bf16 compute mode (mixed '
                               'precision) has no grouped convolution' % groups)


def _dilated_not_mixed(dilations):
    return NotImplementedError('a dilated backbone (dilations=%r) runs in the fp32 compute mode only: the bf16 compute mode (mixed '
                               'precision) has no dilated convolution' % (tuple(dilations),))


def block_width(planes, groups=1, base_width=4, base_channels=64):
    """Channels of a bottleneck's conv1 output / conv2 (T/mmdet/models/backbones/resnext.py:28-32): ``planes`` for a ResNet,
    floor(planes * base_width / base_channels) * groups for a ResNeXt."""
    if groups == 1:
        return planes
    return math.floor(planes * (base_width / base_channels)) * groups


def _bn_not_mixed():
    return NotImplementedError('BatchNorm batch statistics (ResNet norm_eval=False) run in the fp32 compute mode only: the bf16 compute '
                               'mode (mixed precision) keeps norm_eval=True')


class _Block(nn.Module):
    def __init__(self, kind, inplanes, planes, stride, downsample, norm=nn.BatchNorm2d, style='pytorch', groups=1, base_width=4,
                 base_channels=64, dilation=1):
        super().__init__()
        self.kind = kind
        # every block of a dilated stage: the 3x3 that carries the stride slot -- bottleneck conv2, BasicBlock conv1 -- runs at
        # padding = dilation (resnet.py:36-47, 175-200; resnext.py:55-75); BasicBlock conv2 stays padding 1 / dilation 1
        d = dilation
        assert groups == 1 or kind == 'bottleneck', 'grouped blocks are bottlenecks (resnext.py:11)'
        if kind == 'bottleneck':  # style='pytorch': the stride sits on the 3x3, 'caffe': on the first 1x1 (resnet.py:153-158)
            s1, s2 = (1, stride) if style == 'pytorch' else (stride, 1)
            # ResNeXt (resnext.py:28-84): conv1 inplanes -> width, conv2 width -> width in ``groups`` groups (csrc/conv_group.hip),
            # conv3 width -> 4 * planes; groups == 1: width = planes, the ResNet block
            width = block_width(planes, groups, base_width, base_channels)
            self.conv1 = nn.Conv2d(inplanes, width, 1, s1, bias=False)
            self.bn1 = norm(width)
            self.conv2 = nn.Conv2d(width, width, 3, s2, d, dilation=d, groups=groups, bias=False)
            self.bn2 = norm(width)
            self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
            self.bn3 = norm(planes * 4)
        else:
            self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, d, dilation=d, bias=False)
            self.bn1 = norm(planes)
            self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
            self.bn2 = norm(planes)
        self.downsample = downsample

    # the projection shortcut: Sequential(conv 1x1 / stride, BN), or with avg_down Sequential(AvgPool2d(stride, ceil_mode,
    # count_include_pad=False), conv 1x1 / 1, BN) (res_layer.py:39-60) -- the pool module is there at stride 1 too (the identity)
    @property
    def ds_conv(self):
        return self.downsample[-2]

    @property
    def ds_bn(self):
        return self.downsample[-1]

    @property
    def ds_pool(self):
        """The window (= stride) of the shortcut's average pool when it does anything: avg_down and stride > 1; else 0."""
        if self.downsample is None or len(self.downsample) != 3:
            return 0
        k = self.downsample[0].kernel_size
        k = k if isinstance(k, int) else k[0]
        return k if k > 1 else 0

    def shortcut_input(self, x):
        """What the projection shortcut's conv reads: the block input, or with avg_down its average-pooled map (ops.avgpool)."""
        k = self.ds_pool
        return ops.avgpool(x, k) if k else x

    def conv3_shortcut(self, cache, x, o, Pp, record):
        """conv3 -> folded bn3 (+ the shortcut) -> ReLU of a family block (Bottle2neck, ResNeSt, padded RegNet) whose conv3 reads ``o``,
        output pitch Pp -> (out, xp: what the shortcut conv read, or None).  The maps may sit at a padded pitch: the packs and folds
        come through the padded helpers, which fall through where nothing is padded.  Forward only (record False) the shortcut GEMM
        rides in conv3's launch (ops.conv2d_dual, as the ResNet bottleneck's; the same bits); the recorded forward keeps the two
        launches (its backward walks the recorded maps)."""
        pc3 = packed_conv_padded(cache, self.conv3, Pp, o.shape[-1])
        s3, b3 = folded_bn_padded(cache, self.bn3, Pp)
        if self.downsample is None:
            return ops.conv2d(o, pc3, scale=s3, bias=b3, residual=x, relu=True), None
        xp = self.shortcut_input(x)      # avg_down: the pooled map (pad channels average to 0)
        pcd = packed_conv_padded(cache, self.ds_conv, Pp, x.shape[-1])
        sd, bd = folded_bn_padded(cache, self.ds_bn, Pp)
        if not record:
            return ops.conv2d_dual(o, pc3, xp, pcd, scale=s3, bias=b3, scale2=sd, bias2=bd, relu=True), xp
        identity = ops.conv2d(xp, pcd, scale=sd, bias=bd)
        return ops.conv2d(o, pc3, scale=s3, bias=b3, residual=identity, relu=True), xp

    def _norms(self):
        return [self.bn1, self.bn2] + ([self.bn3] if self.kind == 'bottleneck' else []) + \
            ([self.ds_bn] if self.downsample is not None else [])

    def batch_stats(self):
        """True when this block's BatchNorms normalise with batch statistics (training mode, norm_eval=False, stage not frozen)."""
        modes = {self.training and bn.training for bn in self._norms()}
        if len(modes) > 1:
            raise NotImplementedError('a block whose BatchNorm modules are partly in training mode (set the modes through '
                                      'ResNet.train / norm_eval)')
        return modes.pop()

    def run(self, cache, x, save=None):
        """save (dict): training mode -- keeps the block's activations for the backward pass."""
        if self.batch_stats():
            return self._run_batch_stats(cache, x, save)
        identity = x
        dt = x.dtype
        # forward-only fp32 bottleneck with a projection shortcut: the shortcut GEMM rides in conv3's launch (bit-identical,
        # ops.conv2d_dual); the training step keeps the two launches (its backward walks the recorded maps)
        fuse_shortcut = self.downsample is not None and save is None and self.kind == 'bottleneck' and dt == torch.float32
        xp = self.shortcut_input(x) if self.downsample is not None else None      # avg_down: the pooled map (the record keeps it)
        if self.downsample is not None and not fuse_shortcut:
            s, b = folded_bn(cache, self.ds_bn)
            identity = ops.conv2d(xp, packed_conv(cache, self.ds_conv, x.dtype), scale=s, bias=b)
        s1, b1 = folded_bn(cache, self.bn1)
        o1 = ops.conv2d(x, packed_conv(cache, self.conv1, dt), scale=s1, bias=b1, relu=True)
        s2, b2 = folded_bn(cache, self.bn2)
        if self.kind == 'bottleneck':
            o2 = ops.conv2d(o1, packed_conv(cache, self.conv2, dt), scale=s2, bias=b2, relu=True)
            s3, b3 = folded_bn(cache, self.bn3)
            if fuse_shortcut:
                sd, bd = folded_bn(cache, self.ds_bn)
                out = ops.conv2d_dual(o2, packed_conv(cache, self.conv3, dt), xp, packed_conv(cache, self.ds_conv, dt),
                                      scale=s3, bias=b3, scale2=sd, bias2=bd, relu=True)
            else:
                out = ops.conv2d(o2, packed_conv(cache, self.conv3, dt), scale=s3, bias=b3, residual=identity, relu=True)
        else:
            o2 = None
            out = ops.conv2d(o1, packed_conv(cache, self.conv2, dt), scale=s2, bias=b2, residual=identity, relu=True)
        if save is not None:
            save.update(block=self, x=x, xp=xp, o1=o1, o2=o2, identity=identity, out=out)
        return out

    def _run_batch_stats(self, cache, x, save):
        """Training-mode BatchNorm: raw conv (unscaled pack, no epilogue affine) -> batch statistics (running buffers updated) ->
        normalise (+ shortcut) (+ ReLU).  The projection shortcut of a bottleneck joins in conv3's apply pass (two-input form);
        nothing here takes the fused-shortcut conv2d_dual path.  save: the pre-BN maps y* and each BN's statistics (ops.BnStats) as well, and
        beside them the process group each one was synchronised over (``groups``; None: per rank)."""
        if x.dtype != torch.float32:
            raise _bn_not_mixed()
        stats, groups = {}, {}

        def conv_stats(name, conv, bn, inp):
            y = ops.conv2d(inp, packed_conv(cache, conv, torch.float32))
            groups[name] = sync_group(bn)
            stats[name] = ops.bn_batch_stats(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                             bn.momentum, bn.eps, group=groups[name])
            return y, stats[name]

        y1, t1 = conv_stats('bn1', self.conv1, self.bn1, x)
        o1 = ops.bn_apply(y1, t1.scale, t1.cshift, center=t1.center, relu=True)
        y2, t2 = conv_stats('bn2', self.conv2, self.bn2, o1)
        yd = o2 = y3 = xp = None
        if self.downsample is not None:
            xp = self.shortcut_input(x)
            yd, td = conv_stats('bnd', self.ds_conv, self.ds_bn, xp)
        if self.kind == 'bottleneck':
            o2 = ops.bn_apply(y2, t2.scale, t2.cshift, center=t2.center, relu=True)
            y3, tl = conv_stats('bn3', self.conv3, self.bn3, o2)
            yl = y3
        else:
            yl, tl = y2, t2
        if self.downsample is not None:
            out = ops.bn_apply(yl, tl.scale, tl.cshift, center=tl.center, y2=yd, scale2=td.scale, shift2=td.cshift, center2=td.center,
                               relu=True)
        else:
            out = ops.bn_apply(yl, tl.scale, tl.cshift, center=tl.center, residual=x, relu=True)
        if save is not None:
            save.update(block=self, x=x, xp=xp, o1=o1, o2=o2, out=out, y1=y1, y2=y2, y3=y3, yd=yd, stats=stats, groups=groups,
                        batch_stats=True)
        return out


class _StemAttr:
    """``ResNet.stem``: with deep_stem the stem's Sequential, the reference's attribute and state-dict prefix (resnet.py:566); on the
    standard net, which has no such module, the name stays what it was here -- the method that runs the stem (``run_stem``)."""

    def __get__(self, obj, cls):
        if obj is None:
            return self
        m = obj._modules.get('stem')
        return m if m is not None else obj.run_stem


F32_STEM = [True]         # False: stem conv on the implicit-GEMM kernel + separate max-pool (tests)
BF16_STEM_POOL = [True]   # False: stem conv and max-pool as two kernels
BF16_STEM = [True]        # False: the bf16 mode keeps its stem on the fp32 kernel (tests)


@BACKBONES.register_module()
class ResNet(nn.Module):
    arch_settings = {18: ('basic', (2, 2, 2, 2)), 34: ('basic', (3, 4, 6, 3)), 50: ('bottleneck', (3, 4, 6, 3)),
                     101: ('bottleneck', (3, 4, 23, 3)), 152: ('bottleneck', (3, 8, 36, 3))}

    stem = _StemAttr()
    groups, base_width = 1, 4      # ResNeXt sets them before this constructor runs (resnext.py:142-145)

    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4,
                 strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style='pytorch',
                 deep_stem=False, avg_down=False, frozen_stages=-1, conv_cfg=None,
                 norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None, stage_with_dcn=None,
                 plugins=None, with_cp=False, zero_init_residual=True, pretrained=None, init_cfg=None):
        super().__init__()
        if depth not in self.arch_settings:
            raise KeyError('invalid depth %s for resnet' % depth)
        assert style in ('pytorch', 'caffe'), style
        assert dcn is None and plugins is None and not with_cp, 'dcn, plugins and with_cp are not built (SURVEY.md §2a row 5)'
        assert len(strides) >= num_stages and len(dilations) >= num_stages
        self.strides, self.dilations = tuple(strides[:num_stages]), tuple(int(d) for d in dilations[:num_stages])
        for i, (s, d) in enumerate(zip(self.strides, self.dilations)):
            # a dilated stage keeps its resolution: the data gradient of a strided dilated 3x3 (zero insertion at a dilated extent) is
            # not built, and no shipped config asks for it (DC5: strides (1, 2, 2, 1), dilations (1, 1, 1, 2))
            assert d >= 1 and (d == 1 or s == 1), \
                'stage %d: dilations[%d]=%d needs strides[%d]=1, got strides=%r dilations=%r' % (i + 1, i, d, i, self.strides, self.dilations)
        if norm_cfg.get('type') not in ('BN', 'SyncBN'):
            raise NotImplementedError("norm_cfg type %r is not built: the backbone norms are 'BN' (nn.BatchNorm2d) or 'SyncBN' "
                                      "(nn.SyncBatchNorm)" % (norm_cfg.get('type'),))
        if deep_stem and (stem_channels or base_channels) != 64:
            raise NotImplementedError('deep_stem is built for stem_channels=64 (convs 3 -> 32 -> 32 -> 64, csrc/stem_deep.hip), not '
                                      'stem_channels=%s' % (stem_channels or base_channels))
        if self.groups > 1:
            for i in range(num_stages):
                cg = block_width(base_channels * 2 ** i, self.groups, self.base_width, base_channels) // self.groups
                if cg not in ops.GROUP_WIDTHS:
                    raise NotImplementedError('groups=%d with base_width=%d gives a group width of %d channels at stage %d: the grouped 3x3 '
                                              'kernels (csrc/conv_group.hip) are built for widths %s'
                                              % (self.groups, self.base_width, cg, i + 1, list(ops.GROUP_WIDTHS)))
        bn_kw = {'momentum': norm_cfg['momentum']} if 'momentum' in norm_cfg else {}     # (mmcv build_norm_layer)

        norm_cls = nn.SyncBatchNorm if norm_cfg['type'] == 'SyncBN' else nn.BatchNorm2d

        def norm(c):
            return norm_cls(c, **bn_kw)
        self.depth, self.num_stages, self.out_indices = depth, num_stages, tuple(out_indices)
        self.frozen_stages, self.norm_eval = frozen_stages, norm_eval
        self.style, self.deep_stem, self.avg_down = style, bool(deep_stem), bool(avg_down)
        kind, blocks = self.arch_settings[depth]
        exp = 4 if kind == 'bottleneck' else 1
        stem = stem_channels or base_channels
        if self.deep_stem:    # resnet.py:564-596: three 3x3 convs, BN + ReLU after each (the ReLU modules hold the indices 2, 5, 8)
            self.stem = nn.Sequential(
                nn.Conv2d(in_channels, stem // 2, 3, 2, 1, bias=False), norm(stem // 2), nn.ReLU(inplace=True),
                nn.Conv2d(stem // 2, stem // 2, 3, 1, 1, bias=False), norm(stem // 2), nn.ReLU(inplace=True),
                nn.Conv2d(stem // 2, stem, 3, 1, 1, bias=False), norm(stem), nn.ReLU(inplace=True))
        else:
            self.conv1 = nn.Conv2d(in_channels, stem, 7, 2, 3, bias=False)
            self.bn1 = norm(stem)
        inplanes = stem
        self.res_layers = []
        for i in range(num_stages):
            planes = base_channels * 2 ** i
            layer = []
            for bi in range(blocks[i]):
                stride = strides[i] if bi == 0 else 1
                ds = None
                if bi == 0 and (stride != 1 or inplanes != planes * exp):
                    if self.avg_down:     # res_layer.py:39-60 (the pool module is there at stride 1 as well: it shifts the keys)
                        ds = nn.Sequential(nn.AvgPool2d(kernel_size=stride, stride=stride, ceil_mode=True, count_include_pad=False),
                                           nn.Conv2d(inplanes, planes * exp, 1, 1, bias=False), norm(planes * exp))
                    else:
                        ds = nn.Sequential(nn.Conv2d(inplanes, planes * exp, 1, stride, bias=False), norm(planes * exp))
                layer.append(self._make_block(kind, inplanes, planes, stride, ds, norm, style, base_channels, first=bi == 0,
                                              dilation=self.dilations[i]))
                inplanes = planes * exp
            name = 'layer%d' % (i + 1)
            self.add_module(name, nn.Sequential(*layer))
            self.res_layers.append(name)
        self.feat_dim = inplanes
        self.compute_dtype = torch.float32   # torch.bfloat16 = bf16 activations/weights from the stem output on
        self._cache = _PackCache()
        self.zero_init_residual = zero_init_residual
        self.init_weights()
        self._freeze_stages()

    def _make_block(self, kind, inplanes, planes, stride, downsample, norm, style, base_channels, first, dilation=1):
        """One residual block of a stage (``first``: its first block); Res2Net builds its own kind."""
        return _Block(kind, inplanes, planes, stride, downsample, norm, style, self.groups, self.base_width, base_channels, dilation)

    def _freeze_stages(self):  # resnet.py:612-628
        if self.frozen_stages >= 0:
            if self.deep_stem:
                self.stem.eval()
                for p in self.stem.parameters():
                    p.requires_grad = False
            else:
                self.bn1.eval()
                for m in (self.conv1, self.bn1):
                    for p in m.parameters():
                        p.requires_grad = False
        for i in range(1, self.frozen_stages + 1):
            m = getattr(self, 'layer%d' % i)
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def train(self, mode=True):  # resnet.py:647-657
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, _BatchNorm):
                    m.eval()
        return self

    def batch_stats_active(self):
        """True when some BatchNorm of this backbone normalises with batch statistics in the next forward."""
        return (self.training and any(bn.training for bn in self.stem_norms())) or \
            any(blk.batch_stats() for name in self.res_layers for blk in getattr(self, name))

    def stem_norms(self):
        return [self.stem[i] for i in (1, 4, 7)] if self.deep_stem else [self.bn1]

    def stem_parameters(self):
        return list(self.stem.parameters()) if self.deep_stem else list(self.conv1.parameters()) + list(self.bn1.parameters())

    def dilated(self):
        return any(d != 1 for d in self.dilations)

    def _check_mode(self):
        if self.compute_dtype != torch.float32 and self.groups > 1:
            raise _grouped_not_mixed(self.groups)
        if self.compute_dtype != torch.float32 and self.dilated():
            raise _dilated_not_mixed(self.dilations)
        if self.compute_dtype != torch.float32 and self.batch_stats_active():
            raise _bn_not_mixed()

    def init_weights(self):
        """The reference's default init_cfg when no checkpoint is given (resnet.py:404-424; the configs name
        torchvision://resnet50, which is not available offline, so weights normally arrive through load_state_dict):
        Kaiming normal (fan_out, relu) on every conv, BatchNorm weight 1 / bias 0, and -- zero_init_residual -- weight 0 on
        the last norm of every block."""
        from ..layers import bump_weight_epoch
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, _BatchNorm):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if self.zero_init_residual:
            for name in self.res_layers:
                for blk in getattr(self, name):
                    nn.init.constant_((blk.bn2 if blk.kind == 'basic' else blk.bn3).weight, 0)
        bump_weight_epoch()

    def stem_train_reason(self):
        """None when the stem has a backward rule (the standard stem: conv1 7x7 / stride 2 / pad 3, 3 -> 64, no bias, + bn1 + ReLU +
        the 3x3 / 2 max-pool, csrc/stem_bwd.hip), else why not, naming the shape."""
        if self.deep_stem:
            return 'a trainable deep stem (deep_stem=True with frozen_stages=-1) has no backward rule: freeze it (frozen_stages >= 0)'
        c1 = self.conv1
        if not all(p.requires_grad for p in getattr(self, self.res_layers[0]).parameters()):
            return 'a trainable stem needs a trainable %s (its backward starts from that stage\'s input gradient)' % self.res_layers[0]
        if tuple(c1.weight.shape) == (64, 3, 7, 7) and c1.stride == (2, 2) and c1.padding == (3, 3) and c1.bias is None and \
                c1.dilation == (1, 1) and c1.groups == 1:
            return None
        return 'a trainable stem has a backward rule for conv1 7x7 / stride 2 / pad 3, 3 -> 64 only, not for weight %s stride %s ' \
            'padding %s' % (tuple(c1.weight.shape), c1.stride, c1.padding)

    def run_stem(self, x, tape=None):
        """(N,3,H,W) image -> the NHWC map after conv1 + bn1 + ReLU + max-pool (resnet.py:630-637).
        tape (list): when conv1 or bn1 trains, the recording pool instances run and one record (``stem=True``) is appended: the input as the
        kernels read it, the argmax byte map of the pool (csrc/stem_bwd.hip reads both), and with batch statistics the raw conv map and
        its BnStats."""
        c = self._cache
        if self.deep_stem:
            return self._deep_stem(x, tape)
        c1 = self.conv1
        rec = None
        if tape is not None and any(p.requires_grad for p in (c1.weight, self.bn1.weight, self.bn1.bias)):
            reason = self.stem_train_reason()
            if reason is not None:
                raise NotImplementedError(reason)
            rec = dict(stem=True, stage=-1)
            tape.append(rec)

        def pool(m, inp, planar):
            if rec is None:
                return ops.maxpool3x3s2(m)
            out, arg = ops.maxpool3x3s2(m, record=True)
            rec.update(x=inp, planar=planar, arg=arg, conv_hw=(m.shape[1], m.shape[2]))
            return out
        if self.training and self.bn1.training:
            # a stem BatchNorm in training mode (frozen_stages < 0, norm_eval=False): the implicit-GEMM stem conv, batch statistics,
            # normalise + ReLU, then the max-pool
            self._check_mode()
            x = ops.from_nchw(x) if (x.shape[1] > 4 or (x.shape[1] == 4 and x.stride(1) == 1)) else ops.nchw_to_nhwc(x)
            y = ops.conv2d(x, packed_conv(c, c1))
            bn = self.bn1
            group = sync_group(bn)
            t = ops.bn_batch_stats(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps,
                                   group=group)
            if rec is not None:
                rec.update(y=y, stats=t, group=group, batch_stats=True)
            return pool(ops.bn_apply(y, t.scale, t.cshift, center=t.center, relu=True), x, False)
        s, b = folded_bn(c, self.bn1)
        std7 = tuple(c1.weight.shape) == (64, 3, 7, 7) and c1.stride == (2, 2) and c1.padding == (3, 3)
        # the fused stem kernels read the three planes of a contiguous (N,3,H,W) fp32 image themselves (no nchw_to_nhwc4 pass)
        planar = std7 and x.dim() == 4 and x.dtype == torch.float32 and x.shape[1] == 3 and x.is_contiguous() and \
            (F32_STEM[0] if self.compute_dtype == torch.float32 else BF16_STEM[0])
        if not planar:
            # (N,3,H,W) float image -> NHWC4; a 4-channel channels-last view (datasets.GpuImagePipeline output) is taken as is
            x = ops.from_nchw(x) if (x.shape[1] > 4 or (x.shape[1] == 4 and x.stride(1) == 1)) else ops.nchw_to_nhwc(x)
        fused_in = std7 and x.dtype == torch.float32 and (planar or x.shape[-1] == 4)
        record = rec is not None
        if self.compute_dtype == torch.bfloat16 and BF16_STEM[0] and fused_in and ops.stem_bf16_fits(x, planar):
            # bf16 compute mode: the stem on the bf16 matrix cores (csrc/stem_bf16.hip; round 4)
            wp = c.get(('stem_bf16', id(c1)), [c1.weight], lambda: ops.stem_weight_bf16(c1.weight))
            if BF16_STEM_POOL[0]:
                # conv + BN + ReLU + max-pool, one kernel
                r = ops.stem7x7s2_pool_bf16(x, wp, scale=s, bias=b, planar=planar, record=record)
                if not record:
                    return r
                OH, OW = (x.shape[-2] if planar else x.shape[1]) - 1, (x.shape[-1] if planar else x.shape[2]) - 1
                rec.update(x=x, planar=planar, arg=r[1], conv_hw=(OH // 2 + 1, OW // 2 + 1))
                return r[0]
            return pool(ops.stem7x7s2_bf16(x, wp, scale=s, bias=b, relu=True, planar=planar), x, planar)
        elif self.compute_dtype == torch.float32 and F32_STEM[0] and fused_in:
            # conv + BN + ReLU + max-pool in one exact-fp32 kernel (csrc/stem_f32.hip; round 4)
            wp = c.get(('stem_f32', id(c1)), [c1.weight], lambda: ops.stem_weight_f32(c1.weight))
            r = ops.stem7x7s2_pool_f32(x, wp, scale=s, bias=b, planar=planar, record=record)
            if not record:
                return r
            OH, OW = (x.shape[-2] if planar else x.shape[1]) - 1, (x.shape[-1] if planar else x.shape[2]) - 1
            rec.update(x=x, planar=planar, arg=r[1], conv_hw=(OH // 2 + 1, OW // 2 + 1))
            return r[0]
        else:
            # (other stems: the implicit-GEMM kernel in its stem mode; in the bf16 mode it emits the bf16 map)
            if planar:          # (a bf16-mode map too large for the bf16 stem kernel's 32-bit offsets)
                x = ops.nchw_to_nhwc(x)
            x4 = x
            x = ops.conv2d(x, packed_conv(c, c1), scale=s, bias=b, relu=True, out_dtype=self.compute_dtype)
        return pool(x, x4, False)

    def _deep_stem(self, x, tape=None):
        """The deep stem (resnet.py:564-596): three conv3x3 + eval-BN + ReLU and the max-pool as csrc/stem_deep.hip runs them -- exact
        fp32 in both compute modes, the bf16 mode rounds the pooled map once.  The fused 7x7 stems (F32_STEM / BF16_STEM) do not apply.
        Forward only: a tape with trainable stem parameters raises stem_train_reason()."""
        st = self.stem
        if tape is not None and any(p.requires_grad for p in st.parameters()):
            raise NotImplementedError(self.stem_train_reason())
        if self.training and any(bn.training for bn in self.stem_norms()):
            raise NotImplementedError('deep_stem with BatchNorm batch statistics in the stem (norm_eval=False and frozen_stages=-1): '
                                      'the deep stem runs with eval-mode BatchNorm only')
        c = self._cache
        planar = x.dim() == 4 and x.dtype == torch.float32 and x.shape[1] == 3 and x.is_contiguous()
        if not planar:
            # (N,3,H,W) float image -> NHWC4; a 4-channel channels-last view (datasets.GpuImagePipeline output) is taken as is
            x = ops.from_nchw(x) if (x.shape[1] == 4 and x.stride(1) == 1) else ops.nchw_to_nhwc(x)
        packs = [packed_conv(c, st[i]) for i in (0, 3, 6)]
        folds = [folded_bn(c, st[i]) for i in (1, 4, 7)]
        return ops.stem_deep(x, packs, folds, planar=planar, out_dtype=self.compute_dtype)

    def run_stage(self, i, x, tape=None):
        """Stage ``i`` (``layer{i+1}``) on an NHWC map.  tape (list): one record per block with trainable parameters."""
        self._check_mode()
        for blk in getattr(self, self.res_layers[i]):
            rec = None
            if tape is not None and blk.conv1.weight.requires_grad:
                rec = dict(stage=i)
                tape.append(rec)
            x = blk.run(self._cache, x, rec)
        return x

    def forward(self, x, tape=None):
        """x: (N,3,H,W) -> tuple of NCHW-shaped (channels_last) stage outputs.
        tape (list): training mode -- one record per block with trainable parameters, in forward order."""
        self._check_mode()
        x = self.run_stem(x, tape)
        outs = []
        for i in range(len(self.res_layers)):
            x = self.run_stage(i, x, tape)
            if i in self.out_indices:
                outs.append(ops.as_nchw(x))
        return tuple(outs)


@BACKBONES.register_module()
class ResNetV1d(ResNet):
    """ResNetV1d (resnet.py:659-671): the 7x7 stem conv replaced by three 3x3 convs, and a 2x2 average pool before the (then
    stride-1) 1x1 conv of every downsampling shortcut."""

    def __init__(self, **kwargs):
        super().__init__(deep_stem=True, avg_down=True, **kwargs)


@BACKBONES.register_module()
class ResNeXt(ResNet):
    """ResNeXt (T/mmdet/models/backbones/resnext.py:108-153): the bottleneck ResNet whose 3x3 conv runs in ``groups`` groups of
    floor(planes * base_width / base_channels) channels (32x4d: 128 / 256 / 512 / 1024 wide, 64x4d: 256 .. 2048; the stage outputs keep
    ResNet's 256 .. 2048).  Same module names and state-dict keys as ResNet, other shapes.  The grouped layer is csrc/conv_group.hip
    (fp32 compute mode only; group widths 4 / 8 / 16 / 32); ``groups=1`` is the ResNet of that depth on the dense kernels."""
    arch_settings = {50: ('bottleneck', (3, 4, 6, 3)), 101: ('bottleneck', (3, 4, 23, 3)), 152: ('bottleneck', (3, 8, 36, 3))}

    def __init__(self, groups=1, base_width=4, **kwargs):
        self.groups = groups
        self.base_width = base_width
        super().__init__(**kwargs)
