"""Host-side tests of the CTResNetNeck neck (no GPU):

  restatement  tests/ctneck_ref.net in fp64 against the reference's own class (tests/golden/ctneck.npz): output, every gradient and
               the BatchNorm buffers after the forward <= 1e-12 relative
  identity     the four-parity-class form csrc/deconv.hip computes -- 2 x 2 taps per output pixel, rows i + a - t, columns j + b - u,
               weight tap (1 - a + 2t, 1 - b + 2u) -- and the two gradient identities training.py uses, against F.conv_transpose2d and
               autograd in fp64
  layout       state-dict keys, order and shapes are the fixture's recorded list; reference-layout state dicts load strictly
  refusals     every constructor refusal names its key; the bf16 compute mode and an eval-mode neck are refused by name
  init         the bilinear formula in w[:, 0] of every transposed conv, BatchNorm at 1 / 0
  registry     CPR and P2P configs with neck=dict(type='CTResNetNeck', ..., use_dcn=False) build, the bridge admits them, and the
               trainer's flat order lists every parameter once, the neck's in the order its rule states"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import ctneck_ref as CR

R18_NECK = dict(type='CTResNetNeck', in_channel=512, num_deconv_filters=(256, 128, 64), num_deconv_kernels=(4, 4, 4), use_dcn=False)


def _build(cfg):
    import pointtinybenchmark_amd as P
    return P.build_neck(dict(type='CTResNetNeck', **CR.constructor_kwargs(cfg)))


def test_case_names_are_the_fixtures_and_cover_the_issue():
    import json
    cases = json.loads(str(CR.archive()['cases']))
    assert sorted(cases) == sorted(CR.CASE_NAMES)
    assert all(cases[n] == json.loads(json.dumps(CR.CASES[n])) for n in cases)
    got = {(c['in_channel'], tuple(c['filters']), tuple(c['input']), c['train']) for c in CR.CASES.values()}
    assert {(64, (64, 32, 32), (2, 64, 3, 5), True), (32, (32,), (3, 32, 1, 4), True), (64, (64, 32), (1, 64, 2, 2), True),
            (64, (64, 32, 32), (2, 64, 3, 5), False)} <= got
    assert CR.DEVICE_TRAIN == [n for n in CR.CASE_NAMES if CR.CASES[n]['train']], 'every train-mode case runs in train mode on the device'


@pytest.mark.parametrize('name', CR.CASE_NAMES)
def test_fp64_restatement_matches_the_reference_class(name):
    cfg = CR.CASES[name]
    out, grads, stats = CR.restated_case(cfg)
    assert CR.output_error(name, out) <= 1e-12, name
    assert set(CR.grad_names(name)) == set(grads), sorted(set(CR.grad_names(name)) ^ set(grads))
    for key, g in grads.items():
        en, es = CR.grad_errors(name, key, g)
        assert en <= 1e-12 and es <= 1e-12, (name, key, en, es)
    assert set(CR.stat_names(name)) == set(stats)
    for key, v in stats.items():
        ref = torch.from_numpy(CR.stat(name, key))
        if key.endswith('num_batches_tracked'):
            assert int(v) == int(ref) == (1 if cfg['train'] else 0), (name, key)
        else:
            assert float((v - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (name, key)


@pytest.mark.parametrize('shape', [(2, 5, 7, 32, 64), (3, 1, 9, 64, 32), (1, 2, 2, 32, 32)])
def test_parity_class_identity_and_gradient_identities_fp64(shape):
    """y[n, 2i+a, 2j+b] = sum_{t,u} x[n, i+a-t, j+b-u] . w[:, :, 1-a+2t, 1-b+2u], as one GEMM per class over
    ops.deconv_pack_image; dx = conv2d(dy, w, stride 2, padding 1) with w read as (out = Cin, in = Cout); dw = the dense weight gradient with the maps' roles swapped.  Small integers: every sum is exact."""
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-4, 5, (N, Cin, H, W), generator=g).double().requires_grad_(True)
    w = torch.randint(-4, 5, (Cin, Cout, 4, 4), generator=g).double().requires_grad_(True)
    y = F.conv_transpose2d(x, w, None, 2, 1)
    from pointtinybenchmark_amd import ops
    pack = ops.deconv_pack_image(w.detach())          # [class][Cout][(tap row, tap column, cin)]: what the kernel's GEMM reads
    assert tuple(pack.shape) == (4, Cout, 4 * Cin)
    z = torch.zeros_like(y)
    xp = F.pad(x.detach(), (1, 1, 1, 1))
    for a in range(2):
        for b in range(2):
            rows = torch.cat([xp[:, :, 1 + a - t:1 + a - t + H, 1 + b - u:1 + b - u + W] for t in range(2) for u in range(2)], 1)
            z[:, :, a::2, b::2] = torch.einsum('nkhw,dk->ndhw', rows, pack[2 * a + b])
    assert torch.equal(z, y.detach())
    dy = torch.randint(-4, 5, tuple(y.shape), generator=g).double()
    y.backward(dy)
    assert torch.equal(F.conv2d(dy, w.detach(), None, 2, 1), x.grad)
    wv = w.detach().clone().requires_grad_(True)
    (F.conv2d(dy, wv, None, 2, 1) * x.detach()).sum().backward()      # the 'conv' reads dy and writes x's shape: its dw with dy := x
    assert torch.equal(wv.grad, w.grad)


@pytest.mark.parametrize('name', CR.CASE_NAMES)
def test_state_dict_layout_is_the_references(name):
    cfg = CR.CASES[name]
    neck = _build(cfg)
    want = CR.archive_keys(name)
    got = [(k, tuple(v.shape)) for k, v in neck.state_dict().items()]
    assert got == want, (got, want)          # keys, ORDER and shapes
    f0 = cfg['filters'][0]
    assert got[0] == ('deconv_layers.0.conv.weight', (f0, cfg['in_channel'], 3, 3))
    assert got[6] == ('deconv_layers.1.conv.weight', (f0, f0, 4, 4)) and all('conv.bias' not in k for k, _ in got)
    sd = CR.case_state_dict(cfg, torch.float32)
    assert list(sd) == [k for k, _ in want]
    neck.load_state_dict(sd, strict=True)
    assert all(torch.equal(neck.state_dict()[k], v) for k, v in sd.items())
    assert isinstance(neck.deconv_layers[1].conv, torch.nn.ConvTranspose2d) and neck.out_channels == cfg['filters'][-1]


def test_registry_exports_and_init_weights():
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd.necks import CTResNetNeck
    assert P.CTResNetNeck is CTResNetNeck and P.NECKS.get('CTResNetNeck') is CTResNetNeck and CTResNetNeck.materialised
    n = P.build_neck(dict(type='CTResNetNeck', in_channel=64, num_deconv_filters=(64, 32), num_deconv_kernels=(4, 4), use_dcn=False))
    f, c = 2, (2 * 2 - 1 - 0) / 4.0          # f = ceil(4 / 2), c = (2f - 1 - f % 2) / (2f)
    want = torch.tensor([[(1 - math.fabs(i / f - c)) * (1 - math.fabs(j / f - c)) for j in range(4)] for i in range(4)])
    for _, dm in n.stages():
        w = dm.conv.weight.detach()
        assert all(torch.equal(w[k, 0], want) for k in range(w.shape[0]))
        assert not torch.equal(w[0, 1], want), 'only the first output channel holds the bilinear kernel'
    for m in n.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            assert bool((m.weight == 1).all()) and bool((m.bias == 0).all())
    n.deconv_layers[1].conv.weight.data.zero_()
    n.init_weights()
    assert torch.equal(n.deconv_layers[1].conv.weight.detach()[3, 0], want)


def test_constructor_refusals_name_their_key():
    import pointtinybenchmark_amd as P
    kw = dict(type='CTResNetNeck', in_channel=64, num_deconv_filters=(64, 32), num_deconv_kernels=(4, 4), use_dcn=False)
    for bad, key in ((dict(use_dcn=True), 'use_dcn'), (dict(num_deconv_kernels=(4, 3)), 'num_deconv_kernels'),
                     (dict(num_deconv_kernels=(2, 4)), 'num_deconv_kernels'), (dict(num_deconv_filters=(64, 48)), 'num_deconv_filters'),
                     (dict(in_channel=48), 'in_channel')):
        with pytest.raises(NotImplementedError, match=key):
            P.build_neck(dict(kw, **bad))
    with pytest.raises(NotImplementedError, match='use_dcn'):      # the reference's default
        P.build_neck({k: v for k, v in kw.items() if k != 'use_dcn'})


def test_cpu_maps_and_bf16_maps_are_refused():
    import pointtinybenchmark_amd as P
    from pointtinybenchmark_amd._lib import CprHipError
    n = P.build_neck(dict(type='CTResNetNeck', in_channel=32, num_deconv_filters=(32,), num_deconv_kernels=(4,), use_dcn=False)).eval()
    with pytest.raises(NotImplementedError, match='CTResNetNeck.*fp32 compute mode only'):
        n.run(torch.zeros((1, 2, 2, 32), dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match='CTResNetNeck in eval'):
        n.run(torch.zeros((1, 2, 2, 32)), tape=[])
    with pytest.raises((CprHipError, AssertionError)):      # no CPU fallback: a missing device is an error, not an eager route
        n.run(torch.zeros((1, 2, 2, 32)))


def test_syncbn_inside_the_neck_is_refused_before_any_device_call():
    import pointtinybenchmark_amd as P
    n = P.build_neck(dict(type='CTResNetNeck', in_channel=32, num_deconv_filters=(32,), num_deconv_kernels=(4,), use_dcn=False))
    n = torch.nn.SyncBatchNorm.convert_sync_batchnorm(n)
    assert isinstance(n.deconv_layers[1].bn, torch.nn.SyncBatchNorm)
    for mode in (True, False):
        with pytest.raises(NotImplementedError, match='SyncBatchNorm inside the neck'):
            n.train(mode).run(torch.zeros((2, 2, 2, 32)))      # a CPU map: the refusal comes before the first kernel


def test_train_mode_pitch_is_a_multiple_of_64():
    from pointtinybenchmark_amd.necks import CTResNetNeck
    assert [CTResNetNeck.bn_pitch(c) for c in (32, 64, 96, 128, 160, 256)] == [64, 64, 128, 128, 192, 256]


def _models():
    import pointtinybenchmark_amd as P
    from bench import model_cfg, p2p_model_cfg
    cpr = model_cfg(18, 1)
    cpr['neck'] = dict(R18_NECK)
    cpr['bbox_head'] = dict(cpr['bbox_head'], in_channels=64, strides=[4])
    p2p = p2p_model_cfg(18, 1)
    p2p['neck'] = dict(R18_NECK)
    p2p['bbox_head'] = dict(p2p['bbox_head'], in_channels=64, strides=[4])
    return P.build_detector(cpr), P.build_detector(p2p)


def test_cpr_and_p2p_configs_build_and_the_flat_order_is_the_rules():
    from pointtinybenchmark_amd import autograd_bridge, synthetic
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    for m, T in zip(_models(), (CprTrainer, P2PTrainer)):
        assert type(m.neck).__name__ == 'CTResNetNeck'
        sd = synthetic.ctneck_state_dict(512, (256, 128, 64))
        assert tuple(sd['neck.deconv_layers.5.conv.weight'].shape) == (64, 64, 4, 4)
        res = m.load_state_dict(sd, strict=False)
        assert res.unexpected_keys == [] and not [k for k in res.missing_keys if k.startswith('neck.')]
        assert autograd_bridge.unsupported_reason(m) is None
        shell = T.__new__(T)
        shell.model = m
        order = shell._backward_order()
        ids = [id(p) for p in order]
        assert len(set(ids)) == len(ids) and set(ids) == {id(p) for p in m.parameters() if p.requires_grad}
        names = {id(p): k for k, p in m.named_parameters()}
        got = [names[i] for i in ids if names[i].startswith('neck.')]
        want = ['neck.deconv_layers.%d.%s' % (k, s) for k in (5, 4, 3, 2, 1, 0) for s in ('conv.weight', 'bn.weight', 'bn.bias')]
        assert got == want, got
        pos = {i: n for n, i in enumerate(ids)}
        assert max(pos[id(p)] for p in m.bbox_head.parameters()) + 1 == pos[id(m.neck.deconv_layers[5].conv.weight)], 'head -> neck -> backbone'
        assert pos[id(m.neck.deconv_layers[0].bn.bias)] + 1 == min(pos[id(p)] for p in m.backbone.parameters() if p.requires_grad)


def test_bridge_and_compute_mode_refusals_name_the_neck():
    import torch as _t
    from pointtinybenchmark_amd import autograd_bridge
    from pointtinybenchmark_amd.training import BackwardEngine
    m, _ = _models()
    m.neck.eval()
    assert 'CTResNetNeck in eval() mode' in autograd_bridge.unsupported_reason(m)
    m.neck.train()
    with pytest.raises(NotImplementedError, match='CTResNetNeck.*fp32 compute mode only'):
        m.set_compute_dtype('bf16')
    m.backbone.compute_dtype = _t.bfloat16
    assert 'CTResNetNeck' in autograd_bridge.unsupported_reason(m) and 'fp32 compute mode only' in autograd_bridge.unsupported_reason(m)
    with pytest.raises(NotImplementedError, match='CTResNetNeck.*fp32 compute mode only'):
        BackwardEngine(m, two_streams=False)
