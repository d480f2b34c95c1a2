"""The native trainer's optimizer plumbing without a GPU: mmcv-style optimizer dicts, ``CprTrainer.from_config`` on the
P2P configs' Adam settings, its refusals, and torch.optim-format state dicts (the trainer is built on CPU, as in the gloo
tests; no kernel runs)."""
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P2P_CFG = 'configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py'
# configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py:86-93 (the same block: configs2/COCO/p2p/
# p2p_r50_fpns4_1x_fl_sl1_coco.py:141-143, configs2/DOTA/p2p/*.py:152-154)
ADAM = dict(type='Adam', lr=1e-4)
LR_CONFIG = dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=1.0 / 3, step=[8, 11])
IPE = 400       # iterations per epoch of the schedule checks


def p2p_config(**over):
    ref = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'reference_configs.json')))[P2P_CFG]
    cfg = dict(optimizer=dict(ADAM), optimizer_config=ref['optimizer_config'], lr_config=dict(LR_CONFIG))
    cfg.update(over)
    return cfg


def cpu_model(depth=18, frozen_stages=1):
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    torch.manual_seed(0)
    cfg = p2p_model_cfg(depth)
    cfg['backbone']['frozen_stages'] = frozen_stages
    return P.build_detector(cfg)


def test_from_config_reads_the_p2p_adam_block():
    from pointtinybenchmark_amd.config import Config
    from pointtinybenchmark_amd.training import P2PTrainer
    for cfg in (p2p_config(), Config(p2p_config())):
        tr = P2PTrainer.from_config(cpu_model(), cfg, IPE, two_streams=False)
        o = tr.optimizer
        assert o['type'] == 'Adam' and o['lr'] == 1e-4 and o['betas'] == (0.9, 0.999) and o['eps'] == 1e-8
        assert o['weight_decay'] == 0.0 and o['amsgrad'] is False
        assert tr.max_norm == 35
        assert tr.flat_m is None and tr.exp_avg.shape == tr.exp_avg_sq.shape == tr.flat_p.shape
        s = tr.schedule
        third = 1e-4 / 3
        want = {0: third, 250: 1e-4 * (1 - 0.5 * (1 - 1 / 3)), 499: 1e-4 * (1 - (1 / 500) * (1 - 1 / 3)), 500: 1e-4,
                8 * IPE - 1: 1e-4, 8 * IPE: 1e-5, 11 * IPE - 1: 1e-5, 11 * IPE: 1e-6}
        for it, lr in want.items():
            assert s.lr(it) == pytest.approx(lr, rel=1e-12), (it, s.lr(it), lr)


def test_from_config_without_clip_and_with_adamw_and_sgd():
    from pointtinybenchmark_amd.training import P2PTrainer
    tr = P2PTrainer.from_config(cpu_model(), p2p_config(optimizer_config=dict(grad_clip=None), lr_config=None), IPE,
                                two_streams=False)
    assert tr.max_norm is None and tr.schedule is None
    tr = P2PTrainer.from_config(cpu_model(), p2p_config(optimizer=dict(type='AdamW', lr=1e-4, betas=[0.8, 0.99])), IPE,
                                two_streams=False)
    assert tr.optimizer['type'] == 'AdamW' and tr.optimizer['weight_decay'] == 1e-2 and tr.optimizer['betas'] == (0.8, 0.99)
    tr = P2PTrainer.from_config(cpu_model(), p2p_config(optimizer=dict(type='SGD', lr=0.01, momentum=0.9,
                                                                       weight_decay=0.0001)), IPE, two_streams=False)
    assert tr.exp_avg is None and tr.flat_m is not None and (tr.lr, tr.momentum, tr.weight_decay) == (0.01, 0.9, 1e-4)


@pytest.mark.parametrize('over, match', [
    (dict(optimizer=dict(type='Adam', lr=1e-4, paramwise_cfg=dict(norm_decay_mult=0.))), 'paramwise_cfg'),
    (dict(optimizer=dict(type='Adam', lr=1e-4, amsgrad=True)), 'amsgrad'),
    (dict(optimizer=dict(type='SGD', lr=0.01, momentum=0.9, nesterov=True)), 'nesterov'),
    (dict(optimizer=dict(type='SGD', lr=0.01, momentum=0.9, dampening=0.1)), 'dampening'),
    (dict(optimizer=dict(type='RMSprop', lr=0.01)), 'RMSprop'),
    (dict(optimizer_config=dict(grad_clip=dict(max_norm=35, norm_type=1))), 'norm_type'),
    (dict(optimizer_config=dict(type='Fp16OptimizerHook', loss_scale=512.)), r"set_compute_dtype\('bf16'\)"),
    (dict(optimizer_config=dict(type='GradientCumulativeOptimizerHook', cumulative_iters=2)), 'GradientCumulative'),
    (dict(optimizer=None), 'no optimizer'),
])
def test_from_config_refuses_what_is_not_built(over, match):
    from pointtinybenchmark_amd.training import P2PTrainer
    with pytest.raises(ValueError, match=match):
        P2PTrainer.from_config(cpu_model(), p2p_config(**over), IPE, two_streams=False)


def test_optimizer_and_sgd_arguments_together_are_refused():
    from pointtinybenchmark_amd.training import P2PTrainer
    with pytest.raises(ValueError, match='not both'):
        P2PTrainer(cpu_model(), lr=0.01, optimizer=dict(ADAM), two_streams=False)


def test_default_trainer_is_the_sgd_trainer_of_before():
    from pointtinybenchmark_amd.training import P2PTrainer
    tr = P2PTrainer(cpu_model(), two_streams=False)
    assert (tr.lr, tr.momentum, tr.weight_decay, tr.max_norm) == (0.02, 0.9, 1e-4, 35.0)
    assert tr.optimizer['type'] == 'SGD' and tr.exp_avg is None and tr.flat_m.shape == tr.flat_p.shape


def _torch_adam_state(model, opt_cls=torch.optim.Adam, steps=3, **kw):
    """A torch optimizer over model.parameters() (frozen stages included, as mmcv's DefaultOptimizerConstructor) after
    ``steps`` steps on seeded gradients."""
    params = list(model.parameters())
    opt = opt_cls(params, lr=1e-4, **kw)
    g = torch.Generator().manual_seed(5)
    for _ in range(steps):
        for p in params:
            if p.requires_grad:
                p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt.state_dict()


def test_torch_adam_state_dict_loads_at_the_flat_offsets_and_exports_again():
    from pointtinybenchmark_amd.training import P2PTrainer
    model = cpu_model()
    params = list(model.parameters())
    assert any(not p.requires_grad for p in params), 'the fixture must have frozen parameters'
    sd = _torch_adam_state(model)
    assert len(sd['state']) == sum(p.requires_grad for p in params)
    tr = P2PTrainer(model, optimizer=dict(ADAM), two_streams=False)
    tr.load_optimizer_state_dict(sd)
    assert tr.steps == 3
    for i, p in enumerate(params):
        if not p.requires_grad:
            continue
        lo, hi = tr.offset[id(p)]
        assert torch.equal(tr.exp_avg[lo:hi], sd['state'][i]['exp_avg'].reshape(-1))
        assert torch.equal(tr.exp_avg_sq[lo:hi], sd['state'][i]['exp_avg_sq'].reshape(-1))
    out = tr.optimizer_state_dict()
    assert set(out['state']) == set(sd['state'])
    for i, st in sd['state'].items():
        assert out['state'][i]['step'].dtype == torch.float32 and out['state'][i]['step'].dim() == 0
        assert float(out['state'][i]['step']) == float(st['step'])
        assert torch.equal(out['state'][i]['exp_avg'], st['exp_avg'])
        assert torch.equal(out['state'][i]['exp_avg_sq'], st['exp_avg_sq'])
    g_out, g_ref = out['param_groups'][0], sd['param_groups'][0]
    assert set(g_ref) <= set(g_out) and g_out['params'] == g_ref['params']
    # and torch takes the export back
    opt = torch.optim.Adam(params, lr=1e-4)
    opt.load_state_dict(out)
    assert float(opt.state[params[-1]]['step']) == 3.0


def test_sgd_state_dict_round_trip_restores_steps():
    from pointtinybenchmark_amd.training import P2PTrainer
    model = cpu_model()
    params = list(model.parameters())
    opt = torch.optim.SGD(params, lr=0.02, momentum=0.9, weight_decay=1e-4)
    for p in params:
        if p.requires_grad:
            p.grad = torch.ones_like(p)
    opt.step()
    sd = opt.state_dict()
    tr = P2PTrainer(model, two_streams=False)
    tr.load_optimizer_state_dict(sd)
    assert tr.steps == 1                                     # the momentum is live: the first-step copy is not re-applied
    tr.steps = 7
    out = tr.optimizer_state_dict()
    assert out['param_groups'][0]['iteration'] == 7
    tr2 = P2PTrainer(cpu_model(), two_streams=False)
    tr2.load_optimizer_state_dict(out)
    assert tr2.steps == 7 and torch.equal(tr2.flat_m, tr.flat_m)


def test_loading_refuses_other_type_hyperparameters_and_shapes():
    from pointtinybenchmark_amd.training import P2PTrainer
    model = cpu_model()
    sd = _torch_adam_state(model, steps=1)
    with pytest.raises(ValueError, match='SGD trainer'):
        P2PTrainer(cpu_model(), two_streams=False).load_optimizer_state_dict(sd)
    with pytest.raises(ValueError, match='AdamW'):
        P2PTrainer(cpu_model(), optimizer=dict(type='AdamW', lr=1e-4, weight_decay=0.),
                   two_streams=False).load_optimizer_state_dict(sd)
    with pytest.raises(ValueError, match='eps'):
        P2PTrainer(cpu_model(), optimizer=dict(type='Adam', lr=1e-4, eps=1e-6),
                   two_streams=False).load_optimizer_state_dict(sd)
    tr = P2PTrainer(cpu_model(), optimizer=dict(type='Adam', lr=0.5), two_streams=False)     # lr: the schedule's
    tr.load_optimizer_state_dict(sd)
    assert tr.steps == 1
    bad = _torch_adam_state(cpu_model(depth=34), steps=1)
    with pytest.raises(ValueError):
        P2PTrainer(cpu_model(), optimizer=dict(ADAM), two_streams=False).load_optimizer_state_dict(bad)
    i = next(iter(sd['state']))
    sd['state'][i]['exp_avg'] = sd['state'][i]['exp_avg'][..., :1]
    before = tr.exp_avg.clone()
    with pytest.raises(ValueError, match='shape'):
        tr.load_optimizer_state_dict(sd)
    assert torch.equal(tr.exp_avg, before), 'a refused load must leave the state as it was'


def test_adam_step_is_in_the_c_abi():
    from pointtinybenchmark_amd import _lib, ops
    assert 'cpr_adam_step' in _lib.SIGNATURES and callable(ops.adam_step)
    with pytest.raises(_lib.CprHipError):
        ops.adam_step(*[torch.zeros(4)] * 4, torch.zeros(1, dtype=torch.float64), 1e-3, (0.9, 0.999), 1e-8, 0., 1, 0., 1.)
