"""Deterministic synthetic weights and inputs for the CPR / P2P hot path.

There is no network in the build or GPU environment, so neither datasets nor the
``torchvision://resnet50`` checkpoint the reference configs name are available.
This module produces (a) a state dict with the reference's key layout
(``backbone.layer{1-4}.{i}.conv{1-3}.weight`` ... ``bbox_head.cls_out.weight``)
and (b) synthetic 640x640 "tiny person" tiles + point annotations with the shapes the
reference pipeline produces (``T/configs2/TinyPersonV2/coarsepointv2/
coarse_point_refine_base_TinyPersonV2_640.py:17-27``: normalised image, Pad(32), 16x16 pseudo
boxes around coarse points).  Pure torch-CPU; no HIP, no oracle import.
"""
import math

import torch

ARCH = {  # T/mmdet/models/backbones/resnet.py:360-366
    18: ('basic', (2, 2, 2, 2)),
    34: ('basic', (3, 4, 6, 3)),
    50: ('bottleneck', (3, 4, 6, 3)),
    101: ('bottleneck', (3, 4, 23, 3)),
    152: ('bottleneck', (3, 8, 36, 3)),
}


def backbone_out_channels(depth):
    kind, _ = ARCH[depth]
    e = 4 if kind == 'bottleneck' else 1
    return [64 * e, 128 * e, 256 * e, 512 * e]


def _bn(sd, prefix, c, g):
    sd[prefix + '.weight'] = torch.rand(c, generator=g) * 0.5 + 0.5
    sd[prefix + '.bias'] = torch.randn(c, generator=g) * 0.1
    sd[prefix + '.running_mean'] = torch.randn(c, generator=g) * 0.1
    sd[prefix + '.running_var'] = torch.rand(c, generator=g) + 0.5
    sd[prefix + '.num_batches_tracked'] = torch.tensor(0, dtype=torch.long)


def _kaiming(shape, g):
    fan_out = shape[0] * shape[2] * shape[3]
    return torch.randn(shape, generator=g) * math.sqrt(2.0 / fan_out)


def _xavier_uniform(shape, g):
    rf = shape[2] * shape[3]
    a = math.sqrt(6.0 / (shape[1] * rf + shape[0] * rf))
    return (torch.rand(shape, generator=g) * 2 - 1) * a


def _gn(sd, prefix, c, g):
    sd[prefix + '.weight'] = torch.rand(c, generator=g) * 0.5 + 0.75
    sd[prefix + '.bias'] = torch.randn(c, generator=g) * 0.1


def resnet_state_dict(depth=50, seed=0, prefix='backbone.', deep_stem=False, avg_down=False, groups=1, base_width=4):
    """deep_stem: the keys of the three-conv stem (``stem.0 / .3 / .6`` convs, ``stem.1 / .4 / .7`` norms) in place of conv1 / bn1;
    avg_down: the projection shortcuts as ``downsample.1`` (conv) / ``downsample.2`` (norm) behind the parameter-free pool at index
    0.  (style='caffe' moves a stride, no key.)  groups / base_width: the ResNeXt shapes (bottleneck depths) -- conv1 / conv2 / conv3
    around width = floor(planes * base_width / 64) * groups channels, conv2 (width, width / groups, 3, 3).  The defaults draw the tensors
    they always drew."""
    g = torch.Generator().manual_seed(seed)
    kind, blocks = ARCH[depth]
    sd = {}
    if deep_stem:
        for i, (co, ci) in zip((0, 3, 6), ((32, 3), (32, 32), (64, 32))):
            sd['%sstem.%d.weight' % (prefix, i)] = _kaiming((co, ci, 3, 3), g)
            _bn(sd, '%sstem.%d' % (prefix, i + 1), co, g)
    else:
        sd[prefix + 'conv1.weight'] = _kaiming((64, 3, 7, 7), g)
        _bn(sd, prefix + 'bn1', 64, g)
    ds = (1, 2) if avg_down else (0, 1)
    inplanes = 64
    for li, nb in enumerate(blocks):
        planes = 64 * 2 ** li
        stride = 1 if li == 0 else 2
        exp = 4 if kind == 'bottleneck' else 1
        for bi in range(nb):
            p = '%slayer%d.%d.' % (prefix, li + 1, bi)
            if kind == 'bottleneck':
                width = planes if groups == 1 else int(planes * base_width // 64) * groups
                sd[p + 'conv1.weight'] = _kaiming((width, inplanes, 1, 1), g)
                _bn(sd, p + 'bn1', width, g)
                sd[p + 'conv2.weight'] = _kaiming((width, width // groups, 3, 3), g)
                _bn(sd, p + 'bn2', width, g)
                sd[p + 'conv3.weight'] = _kaiming((planes * 4, width, 1, 1), g)
                _bn(sd, p + 'bn3', planes * 4, g)
            else:
                sd[p + 'conv1.weight'] = _kaiming((planes, inplanes, 3, 3), g)
                _bn(sd, p + 'bn1', planes, g)
                sd[p + 'conv2.weight'] = _kaiming((planes, planes, 3, 3), g)
                _bn(sd, p + 'bn2', planes, g)
            if bi == 0 and (stride != 1 or inplanes != planes * exp):
                sd[p + 'downsample.%d.weight' % ds[0]] = _kaiming((planes * exp, inplanes, 1, 1), g)
                _bn(sd, p + 'downsample.%d' % ds[1], planes * exp, g)
            inplanes = planes * exp
    return sd


def res2net_state_dict(depth=50, scales=4, base_width=26, seed=0, prefix='backbone.'):
    """The keys and shapes of mmdet's Res2Net (res2net.py), in its state-dict order: the deep stem, then per block conv1, bn1, conv3,
    bn3, downsample.1 / .2 (behind the parameter-free pool at index 0), convs.i, bns.i with slices of floor(planes * base_width / 64)
    channels.  Its own generator: no other call's random stream moves."""
    g = torch.Generator().manual_seed(seed)
    _, blocks = ARCH[depth]
    assert depth in (50, 101, 152), depth
    sd = {}
    for i, (co, ci) in zip((0, 3, 6), ((32, 3), (32, 32), (64, 32))):
        sd['%sstem.%d.weight' % (prefix, i)] = _kaiming((co, ci, 3, 3), g)
        _bn(sd, '%sstem.%d' % (prefix, i + 1), co, g)
    inplanes = 64
    for li, nb in enumerate(blocks):
        planes = 64 * 2 ** li
        width = int(math.floor(planes * (base_width / 64)))
        for bi in range(nb):
            p = '%slayer%d.%d.' % (prefix, li + 1, bi)
            sd[p + 'conv1.weight'] = _kaiming((width * scales, inplanes, 1, 1), g)
            _bn(sd, p + 'bn1', width * scales, g)
            sd[p + 'conv3.weight'] = _kaiming((planes * 4, width * scales, 1, 1), g)
            _bn(sd, p + 'bn3', planes * 4, g)
            if bi == 0:
                sd[p + 'downsample.1.weight'] = _kaiming((planes * 4, inplanes, 1, 1), g)
                _bn(sd, p + 'downsample.2', planes * 4, g)
            for i in range(scales - 1):
                sd['%sconvs.%d.weight' % (p, i)] = _kaiming((width, width, 3, 3), g)
            for i in range(scales - 1):
                _bn(sd, '%sbns.%d' % (p, i), width, g)
            inplanes = planes * 4
    return sd


def regnet_state_dict(arch='regnetx_3.2gf', seed=0, prefix='backbone.', avg_down=False, strides=(2, 2, 2, 2)):
    """The keys and shapes of mmdet's RegNet (regnet.py), in its state-dict order: conv1 (32, 3, 3, 3) / bn1, then per block of stage
    width W in groups of group_w channels conv1 (W, inplanes, 1, 1), conv2 (W, group_w, 3, 3), conv3 (W, W, 1, 1) with their norms and
    the first block's downsample.0 / .1 (avg_down: .1 / .2).  ``arch``: a name of RegNet.arch_settings or the parameter dict.  Its own
    generator: no other call's random stream moves."""
    from .backbones.regnet import RegNet, stage_layout
    g = torch.Generator().manual_seed(seed)
    widths, group_widths, blocks = stage_layout(RegNet.arch_settings[arch] if isinstance(arch, str) else arch)
    sd = {prefix + 'conv1.weight': _kaiming((32, 3, 3, 3), g)}
    _bn(sd, prefix + 'bn1', 32, g)
    ds = (1, 2) if avg_down else (0, 1)
    inplanes = 32
    for li, nb in enumerate(blocks):
        W, gw = widths[li], group_widths[li]
        for bi in range(nb):
            p = '%slayer%d.%d.' % (prefix, li + 1, bi)
            sd[p + 'conv1.weight'] = _kaiming((W, inplanes, 1, 1), g)
            _bn(sd, p + 'bn1', W, g)
            sd[p + 'conv2.weight'] = _kaiming((W, gw, 3, 3), g)
            _bn(sd, p + 'bn2', W, g)
            sd[p + 'conv3.weight'] = _kaiming((W, W, 1, 1), g)
            _bn(sd, p + 'bn3', W, g)
            if bi == 0 and (strides[li] != 1 or inplanes != W):
                sd[p + 'downsample.%d.weight' % ds[0]] = _kaiming((W, inplanes, 1, 1), g)
                _bn(sd, p + 'downsample.%d' % ds[1], W, g)
            inplanes = W
    return sd


def resnest_state_dict(depth=50, seed=0, radix=2, reduction_factor=4, prefix='backbone.'):
    """The keys and shapes of mmdet's ResNeSt (resnest.py; groups=1), in its state-dict order: the deep stem, then per block conv1, bn1,
    conv2.conv (planes * radix, planes / radix, 3, 3), conv2.bn0, conv2.fc1 (weight, bias), conv2.bn1, conv2.fc2 (weight, bias), conv3,
    bn3, downsample.1 / .2 (behind the parameter-free pool at index 0).  Its own generator: no other call's random stream moves."""
    g = torch.Generator().manual_seed(seed)
    blocks = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3), 200: (3, 24, 36, 3)}[depth]
    sd = {}
    for i, (co, ci) in zip((0, 3, 6), ((32, 3), (32, 32), (64, 32))):
        sd['%sstem.%d.weight' % (prefix, i)] = _kaiming((co, ci, 3, 3), g)
        _bn(sd, '%sstem.%d' % (prefix, i + 1), co, g)
    inplanes = 64
    for li, nb in enumerate(blocks):
        planes = 64 * 2 ** li
        inter = max(planes * radix // reduction_factor, 32)
        for bi in range(nb):
            p = '%slayer%d.%d.' % (prefix, li + 1, bi)
            sd[p + 'conv1.weight'] = _kaiming((planes, inplanes, 1, 1), g)
            _bn(sd, p + 'bn1', planes, g)
            sd[p + 'conv2.conv.weight'] = _kaiming((planes * radix, planes // radix, 3, 3), g)
            _bn(sd, p + 'conv2.bn0', planes * radix, g)
            sd[p + 'conv2.fc1.weight'] = _kaiming((inter, planes, 1, 1), g)
            sd[p + 'conv2.fc1.bias'] = torch.randn(inter, generator=g) * 0.1
            _bn(sd, p + 'conv2.bn1', inter, g)
            sd[p + 'conv2.fc2.weight'] = _kaiming((planes * radix, inter, 1, 1), g)
            sd[p + 'conv2.fc2.bias'] = torch.randn(planes * radix, generator=g) * 0.1
            sd[p + 'conv3.weight'] = _kaiming((planes * 4, planes, 1, 1), g)
            _bn(sd, p + 'bn3', planes * 4, g)
            if bi == 0:
                sd[p + 'downsample.1.weight'] = _kaiming((planes * 4, inplanes, 1, 1), g)
                _bn(sd, p + 'downsample.2', planes * 4, g)
            inplanes = planes * 4
    return sd


def mobilenet_v2_state_dict(seed=0, prefix='backbone.'):
    """The keys and shapes of mmdet's MobileNetV2 (mobilenet_v2.py, widen_factor 1.0), in its state-dict order: conv1.conv (32, 3, 3, 3) /
    conv1.bn, per inverted-residual block expand_conv (absent in layer1.0), depthwise_conv (mid, 1, 3, 3) and linear_conv, each .conv /
    .bn, then conv2.conv (1280, 320, 1, 1) / conv2.bn.  Scales are chosen so that ReLU6 clamps on both sides: a conv's weights have
    variance 1 / (fan_in * E[x^2]) for its input's nominal second moment (1 for the image and the linear maps, 5 for a ReLU6 map), so
    its output is about unit variance, and the BatchNorm in front of a ReLU6 has gamma in [2.5, 4.5) and beta ~ N(1, 1) -- a
    pre-activation of standard deviation ~3.5 that is below 0 on ~40 % and above 6 on ~8 % of the elements; a linear conv's BatchNorm
    has gamma in [0.5, 1).  Its own generator: no other call's random stream moves."""
    from .backbones.mobilenet_v2 import MobileNetV2
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv_bn(p, shape, in_moment, act):
        fan_in = shape[1] * shape[2] * shape[3]
        sd[p + '.conv.weight'] = torch.randn(shape, generator=g) * math.sqrt(1.0 / (fan_in * in_moment))
        c = shape[0]
        if act:
            sd[p + '.bn.weight'] = torch.rand(c, generator=g) * 2.0 + 2.5
            sd[p + '.bn.bias'] = torch.randn(c, generator=g) + 1.0
        else:
            sd[p + '.bn.weight'] = torch.rand(c, generator=g) * 0.5 + 0.5
            sd[p + '.bn.bias'] = torch.randn(c, generator=g) * 0.1
        sd[p + '.bn.running_mean'] = torch.randn(c, generator=g) * 0.1
        sd[p + '.bn.running_var'] = torch.rand(c, generator=g) + 0.5
        sd[p + '.bn.num_batches_tracked'] = torch.tensor(0, dtype=torch.long)
    conv_bn(prefix + 'conv1', (32, 3, 3, 3), 1.0, True)
    cin = 32
    for li, (t, c, n, s) in enumerate(MobileNetV2.arch_settings):
        for bi in range(n):
            p = '%slayer%d.%d.' % (prefix, li + 1, bi)
            mid = int(round(cin * t))
            if t != 1:
                conv_bn(p + 'expand_conv', (mid, cin, 1, 1), 1.0, True)
            conv_bn(p + 'depthwise_conv', (mid, 1, 3, 3), 5.0, True)
            conv_bn(p + 'linear_conv', (c, mid, 1, 1), 5.0, False)
            cin = c
    conv_bn(prefix + 'conv2', (1280, cin, 1, 1), 1.0, True)
    return sd


def fpn_state_dict(in_channels, out_channels=256, start_level=0, num_outs=1, seed=1, prefix='neck.', add_extra_convs=False,
                   extra_convs_on_inputs=True):
    """add_extra_convs (False / True / 'on_input' / 'on_lateral' / 'on_output', as FPN takes it): the stride-2 convs of the
    num_outs - (len(in_channels) - start_level) extra pyramid levels, under the next fpn_convs indices, drawn after the regular
    levels (so the regular weights of a seed do not depend on them)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for j, i in enumerate(range(start_level, len(in_channels))):
        sd['%slateral_convs.%d.conv.weight' % (prefix, j)] = _xavier_uniform((out_channels, in_channels[i], 1, 1), g)
        _gn(sd, '%slateral_convs.%d.gn' % (prefix, j), out_channels, g)
        if i < start_level + num_outs:
            sd['%sfpn_convs.%d.conv.weight' % (prefix, j)] = _xavier_uniform((out_channels, out_channels, 3, 3), g)
            _gn(sd, '%sfpn_convs.%d.gn' % (prefix, j), out_channels, g)
    if add_extra_convs is True:
        add_extra_convs = 'on_input' if extra_convs_on_inputs else 'on_output'
    levels = len(in_channels) - start_level
    for k in range(num_outs - levels if add_extra_convs else 0):
        cin = in_channels[-1] if k == 0 and add_extra_convs == 'on_input' else out_channels
        sd['%sfpn_convs.%d.conv.weight' % (prefix, levels + k)] = _xavier_uniform((out_channels, cin, 3, 3), g)
        _gn(sd, '%sfpn_convs.%d.gn' % (prefix, levels + k), out_channels, g)
    return sd


def pafpn_state_dict(in_channels, out_channels=256, start_level=0, num_outs=None, seed=1, prefix='neck.', add_extra_convs=False,
                     extra_convs_on_inputs=True):
    """``fpn_state_dict`` of the same arguments plus PAFPN's bottom-up modules (pafpn.py:69-93): ``downsample_convs.<i>`` (3x3 stride 2)
    and ``pafpn_convs.<i>`` (3x3) for the len(in_channels) - start_level - 1 steps, drawn from a generator of their own (so the FPN part
    of a seed is fpn_state_dict's).  num_outs: None = one output per used level."""
    levels = len(in_channels) - start_level
    num_outs = levels if num_outs is None else num_outs
    assert num_outs >= levels
    sd = fpn_state_dict(in_channels, out_channels, start_level, num_outs, seed, prefix, add_extra_convs, extra_convs_on_inputs)
    g = torch.Generator().manual_seed(seed + 7919)
    for i in range(levels - 1):
        for name in ('downsample_convs', 'pafpn_convs'):
            sd['%s%s.%d.conv.weight' % (prefix, name, i)] = _xavier_uniform((out_channels, out_channels, 3, 3), g)
            _gn(sd, '%s%s.%d.gn' % (prefix, name, i), out_channels, g)
    return sd


def bfp_state_dict(in_channels=256, refine_type='conv', seed=1, prefix='neck.1.'):
    """BFP's parameters (bfp.py:53-60): the refine ConvModule -- ``refine.conv.weight`` (3x3, no bias under a norm layer), ``refine.gn.*`` --
    for refine_type 'conv'; none for refine_type None.  prefix: 'neck.1.' is BFP's place in ``neck=[FPN | PAFPN, BFP]``."""
    sd = {}
    if refine_type == 'conv':
        g = torch.Generator().manual_seed(seed + 104729)
        sd[prefix + 'refine.conv.weight'] = _xavier_uniform((in_channels, in_channels, 3, 3), g)
        _gn(sd, prefix + 'refine.gn', in_channels, g)
    else:
        assert refine_type is None, refine_type
    return sd


def hrfpn_state_dict(in_channels, out_channels=256, num_outs=5, seed=1, prefix='neck.'):
    """HRFPN's parameters in the reference's order (hrfpn.py:52-69): ``reduction_conv.conv.weight`` (out, sum(in_channels), 1, 1) and
    ``.bias``, then ``fpn_convs.<k>.conv.weight`` (3x3) and ``.bias`` per output level.  Weights uniform at the fan-in bound of mmcv's
    caffe2_xavier_init; the biases -- zero after that init -- are drawn non-zero so that a test sees them."""
    g = torch.Generator().manual_seed(seed + 15485863)

    def conv(name, shape):
        bound = math.sqrt(3.0 / (shape[1] * shape[2] * shape[3]))
        sd['%s%s.conv.weight' % (prefix, name)] = (torch.rand(shape, generator=g) * 2 - 1) * bound
        sd['%s%s.conv.bias' % (prefix, name)] = torch.randn(shape[0], generator=g) * 0.1
    sd = {}
    conv('reduction_conv', (out_channels, sum(in_channels), 1, 1))
    for k in range(num_outs):
        conv('fpn_convs.%d' % k, (out_channels, out_channels, 3, 3))
    return sd


def ctneck_layout(in_channel, num_deconv_filters):
    """[(ConvModule key, conv shape)] of the reference's CTResNetNeck (ct_resnet_neck.py:37-61) in its state-dict order: per stage
    ``deconv_layers.<2s>`` -- the 3x3 conv (F, Cin, 3, 3) -- and ``deconv_layers.<2s+1>`` -- the transposed conv (F, F, 4, 4), nn.ConvTranspose2d's
    (in, out, kh, kw) layout.  No conv biases; every module has a ``bn``."""
    out, c = [], in_channel
    for s, f in enumerate(num_deconv_filters):
        out.append(('deconv_layers.%d' % (2 * s), (f, c, 3, 3)))
        out.append(('deconv_layers.%d' % (2 * s + 1), (f, f, 4, 4)))
        c = f
    return out


def ctneck_state_dict(in_channel, num_deconv_filters, seed=1, prefix='neck.'):
    """A state dict of the reference's CTResNetNeck layout (ctneck_layout): Kaiming-scaled conv weights -- the transposed convs at the
    fan of their 2 x 2 live taps per output pixel -- and BatchNorms with non-trivial gammas, betas and running statistics (_bn)."""
    g = torch.Generator().manual_seed(seed + 32452843)
    sd = {}
    for k, (key, shape) in enumerate(ctneck_layout(in_channel, num_deconv_filters)):
        w = _kaiming(shape, g)
        sd[prefix + key + '.conv.weight'] = w * 2.0 if k % 2 else w
        _bn(sd, prefix + key + '.bn', shape[0], g)
    return sd


def hrnet_layout(extra, in_channels=3):
    """[(conv key, conv shape, norm key)] of the reference's HRNet (hrnet.py:267-518) in its state-dict order: conv1 / bn1, conv2 / bn2,
    layer1, then per stage its transition and its modules -- per module the branches' blocks, then ``fuse_layers.<i>.<j>``: for j > i
    a Sequential (conv 1x1 ``0``, norm ``1``, upsample), for j < i a Sequential of i - j Sequentials (conv 3x3 / 2 ``<k>.0``, norm
    ``<k>.1``), nothing at j == i.  A transition entry: a Sequential (conv 3x3 ``0``, norm ``1``) on an existing branch whose width
    changes, a Sequential of Sequentials (``<k>.0``, ``<k>.1``) for a new branch, nothing otherwise."""
    out = []

    def pair(prefix, co, ci, k):
        out.append((prefix + '.0.weight', (co, ci, k, k), prefix + '.1'))

    def block(p, kind, inplanes, planes):
        exp = 4 if kind == 'BOTTLENECK' else 1
        if kind == 'BOTTLENECK':
            out.append((p + '.conv1.weight', (planes, inplanes, 1, 1), p + '.bn1'))
            out.append((p + '.conv2.weight', (planes, planes, 3, 3), p + '.bn2'))
            out.append((p + '.conv3.weight', (planes * 4, planes, 1, 1), p + '.bn3'))
        else:
            out.append((p + '.conv1.weight', (planes, inplanes, 3, 3), p + '.bn1'))
            out.append((p + '.conv2.weight', (planes, planes, 3, 3), p + '.bn2'))
        if inplanes != planes * exp:
            pair(p + '.downsample', planes * exp, inplanes, 1)
        return planes * exp

    out.append(('conv1.weight', (64, in_channels, 3, 3), 'bn1'))
    out.append(('conv2.weight', (64, 64, 3, 3), 'bn2'))
    s1 = extra['stage1']
    c = 64
    for b in range(s1['num_blocks'][0]):
        c = block('layer1.%d' % b, s1['block'], c, s1['num_channels'][0])
    pre = [c]
    for s in (2, 3, 4):
        cfg = extra['stage%d' % s]
        exp = 4 if cfg['block'] == 'BOTTLENECK' else 1
        cur = [ch * exp for ch in cfg['num_channels']]
        for i, ch in enumerate(cur):
            t = 'transition%d.%d' % (s - 1, i)
            if i < len(pre):
                if ch != pre[i]:
                    pair(t, ch, pre[i], 3)
            else:
                for j in range(i + 1 - len(pre)):
                    pair('%s.%d' % (t, j), ch if j == i - len(pre) else pre[-1], pre[-1], 3)
        nb = cfg['num_branches']
        inch = list(cur)
        for m in range(cfg['num_modules']):
            p = 'stage%d.%d' % (s, m)
            for b in range(nb):
                for k in range(cfg['num_blocks'][b]):
                    inch[b] = block('%s.branches.%d.%d' % (p, b, k), cfg['block'], inch[b], cfg['num_channels'][b])
            for i in range(nb):
                for j in range(nb):
                    f = '%s.fuse_layers.%d.%d' % (p, i, j)
                    if j > i:
                        pair(f, inch[i], inch[j], 1)
                    elif j < i:
                        for k in range(i - j):
                            pair('%s.%d' % (f, k), inch[i] if k == i - j - 1 else inch[j], inch[j], 3)
        pre = inch
    return out


def hrnet_state_dict(extra, seed=0, prefix='', in_channels=3):
    """A state dict of the reference's HRNet layout for ``extra`` (hrnet_layout): Kaiming-scaled conv weights and BatchNorms with
    non-trivial gammas, betas and running statistics (_bn)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape, norm in hrnet_layout(extra, in_channels):
        sd[prefix + key] = _kaiming(shape, g)
        _bn(sd, prefix + norm, shape[0], g)
    return sd


def darknet_layout(depth=53):
    """[(ConvModule key, conv shape)] of the reference's Darknet (darknet.py:121-130, :204-212) in its state-dict order: conv1, then per
    conv_res_block{i} its stride-2 ``conv`` and res{j}.conv1 / res{j}.conv2; each holds ``.conv.weight`` and ``.bn.*``.  ``depth`` is
    looked up in the drop-in class's ``arch_settings``."""
    from .backbones.darknet import Darknet
    layers, channels = Darknet.arch_settings[depth]
    out = [('conv1', (32, 3, 3, 3))]
    for i, (n, (cin, cout)) in enumerate(zip(layers, channels)):
        name = 'conv_res_block%d' % (i + 1)
        out.append((name + '.conv', (cout, cin, 3, 3)))
        for j in range(n):
            out.append(('%s.res%d.conv1' % (name, j), (cout // 2, cout, 1, 1)))
            out.append(('%s.res%d.conv2' % (name, j), (cout, cout // 2, 3, 3)))
    return out


def darknet_state_dict(depth=53, seed=0, prefix=''):
    """A state dict of the reference's Darknet layout for ``depth`` (darknet_layout): Kaiming-scaled conv weights and BatchNorms with
    non-trivial gammas, betas and running statistics (_bn)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in darknet_layout(depth):
        sd[prefix + key + '.conv.weight'] = _kaiming(shape, g)
        _bn(sd, prefix + key + '.bn', shape[0], g)
    return sd


def cpr_head_state_dict(num_classes=1, in_channels=256, feat_channels=256, stacked_convs=4, seed=2,
                        prefix='bbox_head.', std=0.01, num_cls_fcs=0, fc_out_channels=1024, binary_ins=False,
                        ins_tower=False, out_bg_cls=False):
    """Normal(0, std) on Conv2d/Linear, cls_out bias = bias_init_with_prob(0.01)
    (T/mmdet/models/point/dense_heads/cpr_head.py:939-948).  ``std`` larger than the reference's
    0.01 makes the synthetic logits spread out (used by tests to exercise the refine filters).
    ins_tower: ins_share_head_feat=False -- a second tower ``ins_convs`` / ``ins_fcs`` (cpr_head.py:992-1008);
    out_bg_cls: one more classifier output (cpr_head.py:953)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    chn = in_channels
    for i in range(stacked_convs):
        sd['%scls_convs.%d.conv.weight' % (prefix, i)] = torch.randn((feat_channels, chn, 3, 3), generator=g) * 0.01
        _gn(sd, '%scls_convs.%d.gn' % (prefix, i), feat_channels, g)
        chn = feat_channels
    for i in range(num_cls_fcs):          # cpr_head.py:999-1005 (ins_share_head_feat: no separate ins_fcs)
        sd['%scls_fcs.%d.weight' % (prefix, i)] = torch.randn((fc_out_channels, chn), generator=g) * (2.0 / chn) ** 0.5
        sd['%scls_fcs.%d.bias' % (prefix, i)] = torch.randn((fc_out_channels,), generator=g) * 0.1
        chn = fc_out_channels
    if ins_tower:
        c2 = in_channels
        for i in range(stacked_convs):
            sd['%sins_convs.%d.conv.weight' % (prefix, i)] = torch.randn((feat_channels, c2, 3, 3), generator=g) * 0.01
            _gn(sd, '%sins_convs.%d.gn' % (prefix, i), feat_channels, g)
            c2 = feat_channels
        for i in range(num_cls_fcs):
            sd['%sins_fcs.%d.weight' % (prefix, i)] = torch.randn((fc_out_channels, c2), generator=g) * (2.0 / c2) ** 0.5
            sd['%sins_fcs.%d.bias' % (prefix, i)] = torch.randn((fc_out_channels,), generator=g) * 0.1
            c2 = fc_out_channels
    n_cls = num_classes + 1 if out_bg_cls else num_classes
    sd[prefix + 'cls_out.weight'] = torch.randn((n_cls, chn), generator=g) * std
    sd[prefix + 'cls_out.bias'] = torch.full((n_cls,), -math.log((1 - 0.01) / 0.01))
    n_ins = n_cls * 2 if binary_ins else n_cls          # cpr_head.py:1009-1011
    sd[prefix + 'ins_out.weight'] = torch.randn((n_ins, chn), generator=g) * std
    sd[prefix + 'ins_out.bias'] = torch.zeros(n_ins)
    return sd


def p2p_head_state_dict(num_classes=1, num_points=1, in_channels=256, feat_channels=256, stacked_convs=4,
                        seed=3, prefix='bbox_head.', std=0.01):
    """T/mmdet/models/point/dense_heads/p2p_head.py:84-105 layer layout."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for tower in ('cls_convs', 'reg_convs'):
        chn = in_channels
        for i in range(stacked_convs):
            sd['%s%s.%d.conv.weight' % (prefix, tower, i)] = torch.randn((feat_channels, chn, 3, 3), generator=g) * 0.01
            _gn(sd, '%s%s.%d.gn' % (prefix, tower, i), feat_channels, g)
            chn = feat_channels
    sd[prefix + 'cls_out.weight'] = torch.randn((num_classes * num_points, feat_channels, 3, 3), generator=g) * std
    sd[prefix + 'cls_out.bias'] = torch.full((num_classes * num_points,), -math.log((1 - 0.01) / 0.01))
    sd[prefix + 'reg_out.weight'] = torch.randn((num_points * 2, feat_channels, 3, 3), generator=g) * std
    sd[prefix + 'reg_out.bias'] = torch.zeros(num_points * 2)
    return sd


def locator_state_dict(depth=50, num_classes=1, start_level=0, head='cpr', seed=0, head_std=0.01, num_points=1,
                       num_cls_fcs=0, fc_out_channels=1024, binary_ins=False, ins_tower=False, out_bg_cls=False, deep_stem=False,
                       avg_down=False, groups=1, base_width=4, arch=None):
    """arch: a RegNet backbone (regnet_state_dict) in place of the ResNet of ``depth``; the FPN then reads its stage widths.
    arch='mobilenet_v2': MobileNetV2 with its default out_indices (1, 2, 4, 7)."""
    if arch == 'mobilenet_v2':
        sd = mobilenet_v2_state_dict(seed)
        chans = [24, 32, 96, 1280]
    elif arch is not None:
        from .backbones.regnet import RegNet, stage_layout
        sd = regnet_state_dict(arch, seed, avg_down=avg_down)
        chans = stage_layout(RegNet.arch_settings[arch] if isinstance(arch, str) else arch)[0]
    else:
        sd = resnet_state_dict(depth, seed, deep_stem=deep_stem, avg_down=avg_down, groups=groups, base_width=base_width)
        chans = backbone_out_channels(depth)
    sd.update(fpn_state_dict(chans, 256, start_level, 1, seed + 1))
    if head == 'cpr':
        sd.update(cpr_head_state_dict(num_classes, seed=seed + 2, std=head_std, num_cls_fcs=num_cls_fcs,
                                      fc_out_channels=fc_out_channels, binary_ins=binary_ins, ins_tower=ins_tower,
                                      out_bg_cls=out_bg_cls))
    else:
        sd.update(p2p_head_state_dict(num_classes, num_points, seed=seed + 3, std=head_std))
    return sd


def synthetic_batch(batch=2, height=640, width=640, num_gts=32, num_classes=1, seed=0, ragged=False):
    """SURVEY.md §8(d) inputs: seed-fixed normalised images, ``num_gts`` coarse points per tile uniform in
    [8, W-8) x [8, H-8), 16x16 pseudo boxes (the dataset's ``pseuw16h16`` annotations), labels, ann ids.
    ``ragged`` gives each image a different number of gts (num_gts, num_gts//2+1, ...)."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randn((batch, 3, height, width), generator=g)
    g2 = torch.Generator().manual_seed(seed + 1)
    gt_bboxes, gt_labels, gt_anns_id, img_metas = [], [], [], []
    next_id = 0
    for b in range(batch):
        n = num_gts if not ragged else max(1, num_gts // (b + 1) + (b % 2))
        xy = torch.rand((n, 2), generator=g2)
        xy[:, 0] = xy[:, 0] * (width - 16) + 8
        xy[:, 1] = xy[:, 1] * (height - 16) + 8
        gt_bboxes.append(torch.cat([xy - 8, xy + 8], dim=1))
        if num_classes == 1:
            gt_labels.append(torch.zeros(n, dtype=torch.long))
        else:
            gt_labels.append(torch.randint(0, num_classes, (n,), generator=g2))
        gt_anns_id.append(torch.arange(next_id, next_id + n, dtype=torch.long))
        next_id += n
        img_metas.append(dict(img_shape=(height, width, 3), pad_shape=(height, width, 3),
                              ori_shape=(height, width, 3), scale_factor=[1.0, 1.0, 1.0, 1.0],
                              filename='synthetic_%d' % b, flip=False))
    return dict(img=img, img_metas=img_metas, gt_bboxes=gt_bboxes, gt_labels=gt_labels, gt_anns_id=gt_anns_id)


def with_refine_points(batch, num_refine, seed=0, jitter=6.0):
    """num_refine > 1 inputs (cpr_head.py:1240-1246): every gt brings R pseudo boxes, gt-major ((num_gts*R, 4) per image):
    refine 0 is the annotated point, the others are seeded perturbations of it (as a previous refinement round would
    supply), kept inside the image.  Returns a copy of ``batch`` with the wider ``gt_bboxes``."""
    if num_refine == 1:
        return batch
    g = torch.Generator().manual_seed(seed + 77)
    out = dict(batch)
    boxes = []
    for b, bb in enumerate(batch['gt_bboxes']):
        h, w = batch['img_metas'][b]['img_shape'][:2]
        ctr = (bb[:, :2] + bb[:, 2:]) / 2
        pts = [ctr]
        for _ in range(num_refine - 1):
            p = ctr + torch.randn(ctr.shape, generator=g) * jitter
            p[:, 0] = p[:, 0].clamp(1, w - 2)
            p[:, 1] = p[:, 1].clamp(1, h - 2)
            pts.append(p)
        pts = torch.stack(pts, dim=1).reshape(-1, 2)                       # (G, R, 2) -> (G*R, 2)
        boxes.append(torch.cat([pts - 8, pts + 8], dim=1))
    out['gt_bboxes'] = boxes
    return out
