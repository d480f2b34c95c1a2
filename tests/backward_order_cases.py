"""The model configurations whose flat parameter order (CprTrainer._backward_order) is pinned by tests/golden/backward_order.json
(written by tools/gen_backward_order.py, checked by tests/test_backward_order_host.py).  One axis at a time from ResNet-50 +
FPN(num_outs=1) + CPRHead (bench.model_cfg); the multi-level necks sit under P2PHead on ResNet-18 with six strides, as in the necks' own
host tests.  Everything builds on the CPU: no device, no weights loaded (the order depends on the modules and requires_grad alone)."""
from tests import dilated_ref as DR
from tests import hrnet_ref as HR

GN = dict(type='GN', num_groups=32, requires_grad=True)
STRIDES6 = [4, 8, 16, 32, 64, 128]
HR_WIDTHS = [32, 64, 128, 256]
MBV2_NECK_IN = [24, 32, 96, 1280]


def _base(head='cpr', depth=50, num_classes=1):
    from bench import model_cfg, p2p_model_cfg
    return model_cfg(depth, num_classes) if head == 'cpr' else p2p_model_cfg(depth, num_classes)


def _head(**kw):
    cfg = _base()
    cfg['bbox_head'] = dict(cfg['bbox_head'], **kw)
    return cfg


def _backbone(head='cpr', depth=50, replace=None, neck_in=None, **kw):
    """replace: the keys of the base backbone config that another backbone type keeps (None: all of them)."""
    cfg = _base(head, depth)
    if replace is not None:
        cfg['backbone'] = dict({k: v for k, v in cfg['backbone'].items() if k in replace}, **kw)
    else:
        cfg['backbone'] = dict(cfg['backbone'], **kw)
    if neck_in is not None:
        cfg['neck'] = dict(cfg['neck'], in_channels=neck_in)
    return cfg


def _neck(kind, extra, bfp=False, refine=None):
    cfg = _base('p2p', 18, 2)
    neck = dict(cfg['neck'], type=kind, num_outs=6, add_extra_convs=extra)
    cfg['neck'] = neck
    if bfp:
        cfg['neck'] = [neck, dict(type='BFP', in_channels=neck['out_channels'], num_levels=6, refine_level=2, refine_type=refine, norm_cfg=GN)]
    cfg['bbox_head'] = dict(cfg['bbox_head'], strides=STRIDES6)
    return cfg


def _regnet(arch, fs):
    from pointtinybenchmark_amd.backbones.regnet import RegNet, stage_layout
    return _backbone(replace=('frozen_stages', 'norm_cfg', 'norm_eval', 'style', 'out_indices'), type='RegNet', arch=arch, frozen_stages=fs,
                     neck_in=stage_layout(RegNet.arch_settings[arch])[0])


def _hrnet(head, neck, n):
    cfg = _base(head)
    cfg['backbone'] = dict(type='HRNet', extra=HR.CASES['w32_tiny']['extra'])
    if neck == 'HRFPN':
        cfg['neck'] = dict(type='HRFPN', in_channels=HR_WIDTHS, out_channels=256, num_outs=n)
    else:
        cfg['neck'] = dict(cfg['neck'], in_channels=HR_WIDTHS, num_outs=n, add_extra_convs=False)
    if head == 'p2p':
        cfg['bbox_head'] = dict(cfg['bbox_head'], strides=[4 << k for k in range(n)])
    return cfg


def _freeze_hrnet_fuse_pair(m):
    fl = m.backbone.stage3[0].fuse_layers[0][1]
    for mod in (fl[0], fl[1]):
        for p in mod.parameters():
            p.requires_grad = False


# name -> (config factory, a function applied to the built model | None)
CASES = {
    # ---- heads
    'cpr_shared_tower': (_head, None),
    'cpr_two_towers': (lambda: _head(ins_share_head_feat=False), None),
    'cpr_fc': (lambda: _head(num_cls_fcs=2, fc_out_channels=64), None),
    'cpr_two_towers_fc': (lambda: _head(ins_share_head_feat=False, num_cls_fcs=1, fc_out_channels=64), None),
    'cpr_shared_classifier': (lambda: _head(ins_share_head_classifier=True), None),
    'p2p': (lambda: _base('p2p'), None),
    # ---- necks
    'fpn_extra_on_input': (lambda: _neck('FPN', 'on_input'), None),
    'fpn_extra_on_lateral': (lambda: _neck('FPN', 'on_lateral'), None),
    'fpn_extra_on_output': (lambda: _neck('FPN', 'on_output'), None),
    'fpn_extra_pool': (lambda: _neck('FPN', False), None),
    'pafpn': (lambda: _neck('PAFPN', False), None),
    'pafpn_extra_on_input': (lambda: _neck('PAFPN', 'on_input'), None),
    'pafpn_extra_on_output': (lambda: _neck('PAFPN', 'on_output'), None),
    'fpn_bfp_refine_none': (lambda: _neck('FPN', 'on_output', True, None), None),
    'fpn_bfp_refine_conv': (lambda: _neck('FPN', 'on_output', True, 'conv'), None),
    'pafpn_bfp_refine_none': (lambda: _neck('PAFPN', 'on_output', True, None), None),
    'pafpn_bfp_refine_conv': (lambda: _neck('PAFPN', 'on_output', True, 'conv'), None),
    'hrnet_hrfpn_1': (lambda: _hrnet('cpr', 'HRFPN', 1), None),
    'hrnet_hrfpn_5': (lambda: _hrnet('p2p', 'HRFPN', 5), None),
    # ---- backbones
    'r50_norm_eval_false': (lambda: _backbone(norm_eval=False), None),
    'r18_norm_eval_false_fs-1': (lambda: _backbone(depth=18, norm_eval=False, frozen_stages=-1), None),
    'r50_v1d': (lambda: _backbone(deep_stem=True, avg_down=True), None),
    'r50_caffe': (lambda: _backbone(style='caffe'), None),
    'r50_dc5': (lambda: _backbone(**DR.DC5), None),
    'r18_os8_fs0': (lambda: _backbone(depth=18, frozen_stages=0, **DR.OS8), None),
    'resnext50': (lambda: _backbone(type='ResNeXt', groups=32, base_width=4), None),
    'res2net50': (lambda: _backbone(type='Res2Net', scales=4, base_width=26), None),
    'res2net50_fs0': (lambda: _backbone(type='Res2Net', scales=4, base_width=26, frozen_stages=0), None),
    'resnest50': (lambda: _backbone(type='ResNeSt'), None),
    'resnest50_fs0': (lambda: _backbone(type='ResNeSt', frozen_stages=0), None),
    'regnetx_800mf_fs1': (lambda: _regnet('regnetx_800mf', 1), None),
    'regnetx_1.6gf_fs-1': (lambda: _regnet('regnetx_1.6gf', -1), None),
    'regnetx_3.2gf_fs0': (lambda: _regnet('regnetx_3.2gf', 0), None),
    'mobilenet_v2_fs-1': (lambda: _backbone(replace=(), type='MobileNetV2', norm_eval=True, frozen_stages=-1, neck_in=MBV2_NECK_IN), None),
    'mobilenet_v2_fs3': (lambda: _backbone(replace=(), type='MobileNetV2', norm_eval=True, frozen_stages=3, neck_in=MBV2_NECK_IN), None),
    'hrnet_fpn_p2p_3': (lambda: _hrnet('p2p', 'FPN', 3), None),
    'hrnet_fpn_cpr_1': (lambda: _hrnet('cpr', 'FPN', 1), None),
    'hrnet_hrfpn_3_fuse_pair_frozen': (lambda: _hrnet('p2p', 'HRFPN', 3), _freeze_hrnet_fuse_pair),
}
for _depth in (18, 50):
    for _fs in (-1, 0, 1, 4):
        CASES['r%d_fs%d' % (_depth, _fs)] = (lambda d=_depth, f=_fs: _backbone(depth=d, frozen_stages=f), None)


def build(name):
    """-> (the model in train mode, its trainer class)."""
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    factory, after = CASES[name]
    cfg = factory()
    m = P.build_detector(cfg)
    m.train()
    if after is not None:
        after(m)
    return m, (P2PTrainer if cfg['bbox_head']['type'] == 'P2PHead' else CprTrainer)


def order_names(name):
    """-> (the parameter names in _backward_order(), the names of the trainable parameters in module order)."""
    m, cls = build(name)
    names = {id(p): k for k, p in m.named_parameters()}
    shell = object.__new__(cls)
    shell.model = m
    return [names[id(p)] for p in shell._backward_order()], [k for k, p in m.named_parameters() if p.requires_grad]
