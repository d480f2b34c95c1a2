"""-m gpu: the native trainer's Adam / AdamW step (``cpr_adam_step``, csrc/optim.hip) -- the kernel against an fp64
restatement and torch.optim.Adam / AdamW on the same device, the trainer against ``loss.backward()`` + clip_grad_norm_ +
torch.optim on the autograd bridge (CPR and P2P, fp32 and bf16), resume through torch.optim-format state dicts, and two
ranks sharing the GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.gen_golden import CPR_CASES
from pointtinybenchmark_amd import ops, synthetic
from tests.conftest import free_port
from tests.test_gpu_cpr_parity import build_hip_locator, to_cuda

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _clip_coef(norm2, max_norm, grad_scale):
    """The kernel's clip coefficient, in its fp32 arithmetic (sgd_kernel's expression)."""
    f = np.float32
    coef = f(grad_scale)
    if max_norm > 0:
        tn = f(math.sqrt(norm2)) * f(grad_scale)
        coef = coef * min(f(max_norm) / (tn + f(1e-6)), f(1.0))
    return float(coef)


def _adam64(p, m, v, g, t, lr, betas, eps, wd, decoupled):
    b1, b2 = betas
    if decoupled:
        p = p * (1 - lr * wd)
    elif wd:
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr / (1 - b1 ** t) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps)
    return p, m, v


def _run_kernel(p0, grads, n, off, lr, betas, eps, wd, decoupled, max_norm, gs):
    """10 steps of ops.adam_step on views [off, off + n) of guarded buffers; -> (p, m, v, coefs, guards intact)."""
    dev = 'cuda'
    guard = float('-inf')
    bufs = [torch.full((off + n + 67,), guard, device=dev) for _ in range(3)]
    p, m, v = (b[off:off + n] for b in bufs)
    p.copy_(p0)
    m.zero_()
    v.zero_()
    gbuf = torch.zeros((off + n + 67,), device=dev)
    g = gbuf[off:off + n]
    norm2 = torch.zeros((1,), device=dev, dtype=torch.float64)
    ws = torch.empty((1024,), device=dev, dtype=torch.float64)
    coefs = []
    for t, gr in enumerate(grads, 1):
        g.copy_(gr)
        if max_norm > 0:
            ops.grad_sumsq(g, norm2, ws, accumulate=False)
        ops.adam_step(p, g, m, v, norm2, lr, betas, eps, wd, t, max_norm, gs, decoupled=decoupled)
        coefs.append(_clip_coef(float(norm2) if max_norm > 0 else 0.0, max_norm, gs))
    torch.cuda.synchronize()
    intact = all(bool((b[:off] == guard).all()) and bool((b[off + n:] == guard).all()) for b in bufs)
    return p.clone(), m.clone(), v.clone(), coefs, intact


CLIP_MODES = [('off', 1.0), ('inactive', 0.5), ('active', 0.5), ('active', 1.0)]


@pytest.mark.parametrize('n, off', [(1, 0), (3, 0), (4097, 0), (4097, 1), ((1 << 22) + 3, 0)])
@pytest.mark.parametrize('clip, gs', CLIP_MODES)
@pytest.mark.parametrize('decoupled', [False, True])
@pytest.mark.parametrize('wd', [0.0, 1e-4])
def test_adam_kernel_vs_fp64_and_torch(n, off, clip, gs, decoupled, wd):
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    gen = torch.Generator().manual_seed(n + 7 * off)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (0.1 + 0.3 * k) for k in range(10)]
    zero = torch.zeros(n, dtype=torch.bool)
    zero[2::5] = True                                  # elements whose gradient is always zero
    for gr in grads:
        gr[zero] = 0
    norm = float(grads[0].double().norm())
    max_norm = {'off': 0.0, 'inactive': 1e9, 'active': 0.3 * norm * gs}[clip]
    grads_d = [gr.cuda() for gr in grads]
    p, m, v, coefs, intact = _run_kernel(p0.cuda(), grads_d, n, off, lr, betas, eps, wd, decoupled, max_norm, gs)
    assert intact, 'the kernel wrote outside [0, n)'
    if clip == 'active':
        assert coefs[0] < gs * 0.5, coefs
    else:
        assert all(c == gs for c in coefs)
    p2, m2, v2, _, _ = _run_kernel(p0.cuda(), grads_d, n, off, lr, betas, eps, wd, decoupled, max_norm, gs)
    assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2), 'repeat launches must be bit-equal'

    # torch.optim on the same device, fed the clipped gradient the kernel forms (grad * coef, one fp32 multiply)
    pt = p0.cuda().clone().requires_grad_(True)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([pt], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    # fp64 restatement
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t, (gr, c) in enumerate(zip(grads_d, coefs), 1):
        pt.grad = gr * c
        opt.step()
        p64, m64, v64 = _adam64(p64, m64, v64, gr.cpu().double() * c, t, lr, betas, eps, wd, decoupled)
    st = opt.state[pt]
    pt, mt, vt = pt.detach().cpu(), st['exp_avg'].cpu(), st['exp_avg_sq'].cpu()
    p, m, v = p.cpu(), m.cpu(), v.cpu()
    # the ulp scale of an element: its parameter, or lr where p crosses zero (the update's own rounding is lr-sized there:
    # one ulp of a moment whose value cancelled to ~0 moves p by ~lr * eps32)
    scale = torch.maximum(p64.abs(), torch.full_like(p64, lr))
    ulp = EPS32 * float(scale.max())
    err_hip, err_torch = float((p.double() - p64).abs().max()), float((pt.double() - p64).abs().max())
    assert err_hip <= 2 * err_torch + ulp, (err_hip, err_torch, ulp)
    # elementwise against torch: 32 ulp of that scale.  Up to 18 were measured, only at 2^22+3 elements (10 steps, a few
    # elements near a zero crossing of p); 8 held at the smaller sizes.  The fp64 bar above is the accuracy claim.
    d = (p.double() - pt.double()).abs()
    assert bool((d <= 32 * EPS32 * scale).all()), float((d / scale).max() / EPS32)
    for a, b in ((m, mt), (v, vt)):
        assert float((a - b).abs().max()) <= 1e-6 * max(float(b.abs().max()), 1e-30), float((a - b).abs().max())
    if not wd:
        assert torch.equal(p[zero], p0[zero]) and bool((m[zero] == 0).all()), 'a zero gradient must not move p'


# ------------------------------------------------------------------------------------------------ 2. CPR against the bridge
def _data(cfg, seed=None):
    batch = synthetic.synthetic_batch(cfg['batch'], cfg['height'], cfg['width'], cfg['num_gts'], cfg['num_classes'],
                                      cfg['seed'] if seed is None else seed, cfg.get('ragged', False))
    cb = to_cuda(batch)
    return dict(img=cb['img'], img_metas=cb['img_metas'], gt_bboxes=cb['gt_bboxes'], gt_labels=cb['gt_labels'])


def _bridge_step(model, opt, data):
    out = model.train_step(dict(data), opt)
    opt.zero_grad()
    out['loss'].backward()
    torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.requires_grad], 35.0)
    opt.step()
    return out['log_vars']['loss']


def _assert_params_close(ma, mb):
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    for k in pa:
        if pa[k].requires_grad:
            d = float((pa[k] - pb[k]).abs().max())
            assert d <= 2e-5 * max(float(pa[k].abs().max()), 1e-3), (k, d)


def _assert_losses_close(la, lb):
    for a, b in zip(la, lb):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(a)), (la, lb)


@pytest.mark.parametrize('kind', ['Adam', 'AdamW'])
def test_cpr_native_adam_matches_torch_adam_on_the_bridge(kind):
    """mmcv's OptimizerHook sequence -- loss.backward(), clip_grad_norm_(35), torch.optim.Adam / AdamW -- against the native
    trainer for three steps (the bars of test_gpu_autograd.test_torch_optimizer_and_clip_drive_the_drop_in_model).  The
    bridge's gradients agree with the trainer's to ~1e-6 of their scale, not bit for bit, and Adam turns any difference in
    an element whose gradient is near zero into an lr-sized step of the other sign: the torch side is handed the trainer's
    gradient after its backward, so what is compared is the clip + update."""
    from pointtinybenchmark_amd.training import CprTrainer
    cfg = CPR_CASES['cpr_r18_c3_128']
    data = _data(cfg)
    hp = dict(lr=1e-3, weight_decay=1e-4)
    ma, _ = build_hip_locator(cfg)
    tr = CprTrainer(ma, optimizer=dict(type=kind, **hp), max_norm=35.0)
    mb, _ = build_hip_locator(cfg)
    opt = getattr(torch.optim, kind)([p for p in mb.parameters() if p.requires_grad], foreach=False, **hp)
    la, lb = [], []
    for _ in range(3):
        la.append(float(ma._parse_losses(tr.forward_backward(**dict(data)))[1]['loss']))
        out = mb.train_step(dict(data), opt)
        opt.zero_grad()
        out['loss'].backward()
        with torch.no_grad():
            for pa, pb in zip(ma.parameters(), mb.parameters()):
                if pa.requires_grad:
                    pb.grad = pa.grad.clone()
        torch.nn.utils.clip_grad_norm_([p for p in mb.parameters() if p.requires_grad], 35.0)
        opt.step()
        tr.step()
        lb.append(out['log_vars']['loss'])
    torch.cuda.synchronize()
    assert la[0] == lb[0]
    _assert_losses_close(la, lb)
    assert la[2] != la[0], 'the optimizer must have moved the weights'
    _assert_params_close(ma, mb)


# ------------------------------------------------------------------------------------------------ 3. P2P from the config
def _p2p_model(bf16=False):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    model = P.build_detector(p2p_model_cfg(18)).cuda()
    model.load_state_dict(synthetic.locator_state_dict(18, 1, 0, 'p2p', 3, head_std=0.05), strict=True)
    if bf16:
        model.set_compute_dtype('bf16')
    model.train()
    return model


def _p2p_data():
    batch = synthetic.synthetic_batch(2, 128, 160, 6, 1, seed=4)
    return dict(img=batch['img'].cuda(), img_metas=batch['img_metas'], gt_bboxes=[b.cuda() for b in batch['gt_bboxes']],
                gt_labels=[l.cuda() for l in batch['gt_labels']])


def _tinyperson_cfg():
    # configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py:86-93
    return dict(optimizer=dict(type='Adam', lr=1e-4), optimizer_config=dict(grad_clip=dict(max_norm=35, norm_type=2)),
                lr_config=dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=1.0 / 3, step=[8, 11]))


@pytest.mark.parametrize('bf16', [False, True])
def test_p2p_from_config_adam_matches_the_bridge_and_trains(bf16):
    from pointtinybenchmark_amd.training import P2PTrainer
    data = _p2p_data()
    cfg = _tinyperson_cfg()
    ma, mb = _p2p_model(bf16), _p2p_model(bf16)
    tr = P2PTrainer.from_config(ma, cfg, iters_per_epoch=100)
    opt = torch.optim.Adam(list(mb.parameters()), lr=tr.schedule.lr(0), foreach=False)
    totals = [tr.train_step(dict(data))['log_vars']['loss']]
    lb = _bridge_step(mb, opt, data)
    torch.cuda.synchronize()
    if bf16:
        _assert_losses_close(totals, [lb])
    else:
        assert totals[0] == lb, (totals[0], lb)
    _assert_params_close(ma, mb)
    if bf16:    # the trained model's forward equals a fresh model loaded from the trainer's state_dict, bit for bit
        fresh = _p2p_model(True)
        fresh.load_state_dict(tr.state_dict())
        with torch.no_grad():
            a = ma.forward_train(**dict(data))
            b = fresh.forward_train(**dict(data))
        for k in a:
            xs, ys = (v if isinstance(v, (list, tuple)) else [v] for v in (a[k], b[k]))
            for x, y in zip(xs, ys):
                assert torch.equal(x, y), k
    for _ in range(3):
        out = tr.train_step(dict(data))
        assert np.isfinite(out['log_vars']['loss'])
        totals.append(out['log_vars']['loss'])
    assert totals[-1] < totals[0], totals


# ------------------------------------------------------------------------------------------------ 4. resume
@pytest.mark.parametrize('kind', ['SGD', 'Adam'])
def test_resume_from_state_dicts_is_bit_equal(kind):
    """2 steps, save model + optimizer state, rebuild everything, load, 2 more steps == 4 uninterrupted steps.  The
    schedule warms up over the four iterations, so the restored iteration count matters too."""
    from pointtinybenchmark_amd.training import CprTrainer, StepLrSchedule
    cfg = CPR_CASES['cpr_r18_c3_128']
    data = _data(cfg)
    optimizer = dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=1e-4) if kind == 'SGD' else dict(type='Adam', lr=1e-3)

    def trainer(model):
        return CprTrainer(model, optimizer=dict(optimizer), max_norm=35.0,
                          schedule=StepLrSchedule(optimizer['lr'], 2, step=(1,), warmup_iters=4, warmup_ratio=0.1))
    m0, _ = build_hip_locator(cfg)
    t0 = trainer(m0)
    for _ in range(4):
        t0.train_step(dict(data))
    m1, _ = build_hip_locator(cfg)
    t1 = trainer(m1)
    for _ in range(2):
        t1.train_step(dict(data))
    torch.cuda.synchronize()
    sd, osd = t1.state_dict(), t1.optimizer_state_dict()
    del t1, m1
    m2, _ = build_hip_locator(cfg)
    m2.load_state_dict(sd)
    t2 = trainer(m2)
    t2.load_optimizer_state_dict(osd)
    assert t2.steps == 2
    for _ in range(2):
        t2.train_step(dict(data))
    torch.cuda.synchronize()
    assert torch.equal(t2.flat_p, t0.flat_p), float((t2.flat_p - t0.flat_p).abs().max())


# ------------------------------------------------------------------------------------------------ 5. interop
def test_torch_adam_state_moves_into_the_native_trainer_and_back():
    from pointtinybenchmark_amd.training import CprTrainer
    cfg = CPR_CASES['cpr_r18_c3_128']
    data = _data(cfg)
    lr = 1e-3
    # torch -> native
    mb, _ = build_hip_locator(cfg)
    opt = torch.optim.Adam(list(mb.parameters()), lr=lr, foreach=False)
    for _ in range(2):
        _bridge_step(mb, opt, data)
    ma, _ = build_hip_locator(cfg)
    ma.load_state_dict(mb.state_dict())
    tr = CprTrainer(ma, optimizer=dict(type='Adam', lr=lr), max_norm=35.0)
    tr.load_optimizer_state_dict(opt.state_dict())
    assert tr.steps == 2
    la = tr.train_step(dict(data))['log_vars']['loss']
    lb = _bridge_step(mb, opt, data)
    torch.cuda.synchronize()
    _assert_losses_close([la], [lb])
    _assert_params_close(ma, mb)
    # native -> torch
    mc, _ = build_hip_locator(cfg)
    tc = CprTrainer(mc, optimizer=dict(type='Adam', lr=lr), max_norm=35.0)
    for _ in range(2):
        tc.train_step(dict(data))
    md, _ = build_hip_locator(cfg)
    md.load_state_dict(tc.state_dict())
    opt2 = torch.optim.Adam(list(md.parameters()), lr=lr, foreach=False)
    opt2.load_state_dict(tc.optimizer_state_dict())
    lc = tc.train_step(dict(data))['log_vars']['loss']
    ld = _bridge_step(md, opt2, data)
    torch.cuda.synchronize()
    _assert_losses_close([lc], [ld])
    _assert_params_close(mc, md)


# ------------------------------------------------------------------------------------------------ 6. two ranks
_TWO_RANK_ADAM = r'''
import os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, %(root)r)
rank, port, out = int(sys.argv[1]), sys.argv[2], sys.argv[3]
os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=port)
dist.init_process_group('gloo', rank=rank, world_size=2)          # both ranks share the one GPU: gloo, not RCCL
torch.cuda.set_device(0)
from oracle.gen_golden import CPR_CASES
from pointtinybenchmark_amd import synthetic
from pointtinybenchmark_amd.training import CprTrainer
from tests.test_gpu_cpr_parity import build_hip_locator, to_cuda
cfg = CPR_CASES['cpr_r18_c3_128']
batch = synthetic.synthetic_batch(4, cfg['height'], cfg['width'], cfg['num_gts'], cfg['num_classes'], 5, True)
cb = to_cuda(batch)
sl = slice(2 * rank, 2 * rank + 2)
data = dict(img=cb['img'][sl].contiguous(), img_metas=cb['img_metas'][sl], gt_bboxes=cb['gt_bboxes'][sl], gt_labels=cb['gt_labels'][sl])
m, _ = build_hip_locator(cfg)
tr = CprTrainer(m, optimizer=dict(type='Adam', lr=1e-3), bucket_mb=1.0, reducer='reduce_scatter')
for _ in range(2):
    tr.train_step(dict(data))
torch.cuda.synchronize()
torch.save(dict(p=tr.flat_p.cpu(), m=tr.exp_avg.cpu(), v=tr.exp_avg_sq.cpu(), world=tr.buckets.world_size), out + '.%%d' %% rank)
dist.destroy_process_group()
'''


def test_two_ranks_adam_stay_bit_equal(tmp_path):
    script = tmp_path / 'worker.py'
    script.write_text(_TWO_RANK_ADAM % dict(root=ROOT))
    port = str(free_port())
    out = str(tmp_path / 'res')
    procs = [subprocess.Popen([sys.executable, str(script), str(r), port, out], cwd=ROOT, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    logs = [p.communicate(timeout=600)[0].decode(errors='replace') for p in procs]
    assert all(p.returncode == 0 for p in procs), '\n'.join(l[-1500:] for l in logs)
    res = [torch.load(out + '.%d' % r) for r in range(2)]
    assert res[0]['world'] == 2
    for k in ('p', 'm', 'v'):
        assert torch.equal(res[0][k], res[1][k]), k
    assert float(res[0]['m'].abs().max()) > 0
