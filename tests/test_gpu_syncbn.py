"""-m gpu: SyncBN -- BatchNorm batch statistics over the rows of every rank (norm_cfg=dict(type='SyncBN'), torch.nn.SyncBatchNorm).

The oracle is fp64 torch ``F.batch_norm(training=True)`` on the concatenation of all ranks' rows: what SyncBatchNorm is defined to equal
(torch.nn.SyncBatchNorm itself needs one device per rank).  1. the split finalize kernels of csrc/bn_train.hip, one process playing R
ranks; 2. one rank is BatchNorm bit for bit; 3. two processes on the one GPU under gloo; 4. the refusals."""
import copy
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import cpr_oracle as O
from oracle.gen_golden import CPR_CASES
from pointtinybenchmark_amd import ops, synthetic
from tests.conftest import free_port
from tests.test_gpu_cpr_parity import build_hip_locator, to_cuda

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5


def _rel_l2(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


# ------------------------------------------------------------------------------------------------ 1. kernels, one process = R ranks
# the chunks each "rank" holds (NHWC); the maps of the issue split at image boundaries
CASES = {
    '3x7x9x64_2+1': [(2, 7, 9, 64), (1, 7, 9, 64)],
    '4x5x5x2048_1+1+2': [(1, 5, 5, 2048), (1, 5, 5, 2048), (2, 5, 5, 2048)],          # two channel groups of 1024, three ranks
    'one_row_rank': [(1, 1, 1, 64), (1, 2, 3, 64)],                                   # M2_r = 0 on the first rank
    '2x40x40x256_1+1': [(1, 40, 40, 256), (1, 40, 40, 256)],
}


def _chunks(shapes, variant, seed):
    """The data of test_gpu_bn_batch_stats.test_kernels_match_fp64_torch per chunk; variant: 0.0 / 1e3 -- every chunk at offset * std --
    or 'split': the chunks alternate between +1e3 * std and -1e3 * std, so the between-rank term n_r * (mean_r - mean)^2 dominates."""
    torch.manual_seed(seed)
    C = shapes[0][-1]
    dev = 'cuda'
    std = 1.0 + torch.rand(C, device=dev)
    bias = 0.3 * torch.randn(C, device=dev)
    ys = []
    for r, shp in enumerate(shapes):
        off = (1e3 if r % 2 == 0 else -1e3) if variant == 'split' else variant
        ys.append((torch.randn(shp, device=dev) * std + off * std + bias).contiguous())
    p = dict(gamma=1.0 + 0.5 * torch.randn(C, device=dev), beta=0.5 * torch.randn(C, device=dev),
             rm=0.1 * torch.randn(C, device=dev), rv=1.0 + torch.rand(C, device=dev))
    douts = [torch.randn(shp, device=dev) for shp in shapes]
    return ys, douts, p


def _play_ranks(ys, douts, p):
    """Every chunk is one rank: local -> stacked records (the all-gather) -> one merge PER RANK (own map, own buffers)."""
    C = ys[0].shape[-1]
    recs = torch.stack([ops.bn_sync_local_stats(y)[0] for y in ys])
    assert recs.shape == (len(ys), 2 * C + 1) and recs.dtype == torch.float64
    out = []
    for y in ys:
        rm, rv = p['rm'].clone(), p['rv'].clone()
        nbt = torch.zeros((), device='cuda', dtype=torch.int64)
        st = ops.bn_sync_merge_stats(recs, y, p['gamma'], p['beta'], rm, rv, nbt, 0.1, EPS)
        z = ops.bn_apply(y, st.scale, st.cshift, center=st.center, relu=True)
        out.append(dict(st=st, rm=rm, rv=rv, nbt=nbt, z=z))
    loc = [ops.bn_sync_local_bwd(d, y, o['st'].cmean, o['st'].rstd, mask=o['z'], center=o['st'].center)
           for y, d, o in zip(ys, douts, out)]
    brecs = torch.stack([l[0] for l in loc])
    assert brecs.shape == (len(ys), 2 * C)
    for y, d, o, l in zip(ys, douts, out, loc):
        o['dy'] = ops.bn_sync_merge_bwd(brecs, l[1], o['st'].count, d, y, o['st'].cmean, o['st'].rstd, p['gamma'], mask=o['z'],
                                        center=o['st'].center)
        o['dgamma'], o['dbeta'] = l[2], l[3]
    torch.cuda.synchronize()
    return recs, out


def _check_against_oracle(ys, douts, p, recs, out):
    C = ys[0].shape[-1]
    rows = [int(y.numel() // C) for y in ys]
    assert [float(v) for v in recs[:, 2 * C]] == [float(n) for n in rows]            # the count travels as an exact integer value
    # fp64 torch on the concatenation of all ranks' rows
    x = torch.cat([y.reshape(-1, C) for y in ys]).double().requires_grad_(True)
    g = p['gamma'].double().requires_grad_(True)
    b = p['beta'].double().requires_grad_(True)
    rm, rv = p['rm'].double().clone(), p['rv'].double().clone()
    lin = F.batch_norm(x, rm, rv, g, b, True, 0.1, EPS)
    z_ref = F.relu(lin).detach()
    # the ReLU mask of the backward is the kernel's own recorded output (as the product path: mask = the block's output map)
    mask = (torch.cat([o['z'].reshape(-1, C) for o in out]) > 0).double()
    dall = torch.cat([d.reshape(-1, C) for d in douts]).double()
    (lin * mask * dall).sum().backward()
    xd = x.detach()
    mu_ref, var_ref = xd.mean(0), xd.var(0, unbiased=False)
    sd_ref = var_ref.sqrt()
    for o in out:
        st = o['st']
        assert ((st.mean.double() - mu_ref).abs() <= 1e-6 * sd_ref + 2.0 ** -24 * mu_ref.abs()).all()
        var_k = 1.0 / st.rstd.double() ** 2 - EPS
        assert ((var_k - var_ref).abs() <= 1e-5 * var_ref).all()
        assert torch.allclose(st.scale.double(), p['gamma'].double() * st.rstd.double(), rtol=1e-6, atol=0)
        assert ((o['rm'].double() - rm).abs() <= 1e-5 * rm.abs() + 1e-7).all()
        assert ((o['rv'].double() - rv).abs() <= 1e-5 * rv.abs()).all()
        assert int(o['nbt']) == 1
        assert float(st.count) == float(sum(rows))
    z = torch.cat([o['z'].reshape(-1, C) for o in out])
    assert float((z.double() - z_ref).abs().max()) <= 1e-5 * float(z_ref.abs().max())
    # what every rank uses is a function of the gathered records and the rank order only: the same bits on every rank
    for o in out[1:]:
        for k in ('mean', 'rstd', 'scale', 'shift'):
            assert torch.equal(getattr(o['st'], k), getattr(out[0]['st'], k)), k
        assert torch.equal(o['rm'], out[0]['rm']) and torch.equal(o['rv'], out[0]['rv'])
    # backward: dy of all ranks, the summed parameter gradients, and each rank's own (LOCAL) parameter-gradient sums
    dy = torch.cat([o['dy'].reshape(-1, C) for o in out])
    assert _rel_l2(dy, x.grad) <= 1e-5, _rel_l2(dy, x.grad)
    assert _rel_l2(sum(o['dgamma'].double() for o in out), g.grad) <= 1e-5
    assert _rel_l2(sum(o['dbeta'].double() for o in out), b.grad) <= 1e-5
    xhat = (xd - mu_ref) / (var_ref + EPS).sqrt()
    gm = mask * dall
    lo = 0
    for n, o in zip(rows, out):
        assert _rel_l2(o['dgamma'], (gm[lo:lo + n] * xhat[lo:lo + n]).sum(0)) <= 1e-5
        assert _rel_l2(o['dbeta'], gm[lo:lo + n].sum(0)) <= 1e-5
        lo += n


@pytest.mark.parametrize('variant', [0.0, 1e3, 'split'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_split_kernels_match_fp64_torch_on_all_rows(case, variant):
    shapes = CASES[case]
    ys, douts, p = _chunks(shapes, variant, seed=sum(sum(s) for s in shapes))
    recs, out = _play_ranks(ys, douts, p)
    _check_against_oracle(ys, douts, p, recs, out)
    # another rank order: the same bars (the merge order changes the last bits at most)
    perm = list(range(len(ys)))[::-1]
    ys2, douts2 = [ys[i] for i in perm], [douts[i] for i in perm]
    recs2, out2 = _play_ranks(ys2, douts2, p)
    assert torch.equal(recs2, recs[perm])                                            # what a rank saw does not depend on the others
    _check_against_oracle(ys2, douts2, p, recs2, out2)


def test_momentum_none_is_the_cumulative_average():
    torch.manual_seed(4)
    C = 64
    ys = [torch.randn(1, 3, 4, C, device='cuda'), torch.randn(2, 3, 4, C, device='cuda')]
    bn = nn.BatchNorm2d(C, momentum=None).cuda().double()
    rm, rv = torch.randn(C, device='cuda'), torch.rand(C, device='cuda') + 1
    bn.running_mean.copy_(rm)
    bn.running_var.copy_(rv)
    bn.num_batches_tracked.fill_(3)
    nbt = torch.full((), 3, device='cuda', dtype=torch.int64)
    recs = torch.stack([ops.bn_sync_local_stats(y)[0] for y in ys])
    ops.bn_sync_merge_stats(recs, ys[1], bn.weight.float(), bn.bias.float(), rm, rv, nbt, None, EPS)
    bn.train()
    bn(torch.cat(ys).double().permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    assert int(nbt) == 4
    assert torch.allclose(rm.double(), bn.running_mean, rtol=1e-5, atol=1e-7)
    assert torch.allclose(rv.double(), bn.running_var, rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------------ the locator with SyncBN
def build_locator(cfg, norm_type, frozen_stages=1):
    """tests.test_gpu_cpr_parity.build_hip_locator with the backbone's norm_cfg type set and norm_eval=False (built that way from the
    config, not switched afterwards)."""
    import pointtinybenchmark_amd as P
    orig = P.build_detector

    def patched(model, *a, **kw):
        model = copy.deepcopy(model)
        model['backbone'].update(norm_cfg=dict(type=norm_type, requires_grad=True), norm_eval=False, frozen_stages=frozen_stages)
        return orig(model, *a, **kw)
    P.build_detector = patched
    try:
        return build_hip_locator(cfg)
    finally:
        P.build_detector = orig


def _batch(cfg, n=None):
    b = synthetic.synthetic_batch(n or cfg['batch'], cfg['height'], cfg['width'], cfg['num_gts'], cfg['num_classes'], cfg['seed'],
                                  cfg.get('ragged', False))
    cb = to_cuda(b)
    return b, dict(img=cb['img'], img_metas=cb['img_metas'], gt_bboxes=cb['gt_bboxes'], gt_labels=cb['gt_labels'])


def _flat(v):
    return torch.stack(v) if isinstance(v, list) else v


# ------------------------------------------------------------------------------------------------ 2. one rank: BatchNorm, bit for bit
def test_world_size_one_is_batchnorm_bit_for_bit():
    import torch.distributed as dist
    from pointtinybenchmark_amd.training import CprTrainer
    cfg = CPR_CASES['cpr_r18_c3_128']
    _, data = _batch(cfg)

    def run(norm_type, convert=False):
        m, _ = build_locator(cfg, norm_type)
        if convert:
            m = nn.SyncBatchNorm.convert_sync_batchnorm(m)
        kinds = {type(v) for v in m.backbone.modules() if isinstance(v, nn.modules.batchnorm._BatchNorm)}
        assert kinds == {nn.BatchNorm2d if norm_type == 'BN' and not convert else nn.SyncBatchNorm}
        assert m.backbone.batch_stats_active()
        with torch.no_grad():
            losses = {k: _flat(v).clone() for k, v in m.forward_train(**data).items()}
        tr = CprTrainer(m)
        tr.forward_backward(**data)
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.requires_grad}
        bufs = {k: v.clone() for k, v in m.state_dict().items() if 'running' in k or 'num_batches' in k}
        return m, losses, grads, bufs

    def same(got, want):
        for a, b in zip(got[1:], want[1:]):
            assert list(a) == list(b)
            for k in a:
                assert torch.equal(a[k], b[k]), k
    ref = run('BN')
    assert any(int(v) == 2 for k, v in ref[3].items() if 'num_batches' in k)            # the two forwards moved the trained stages' buffers
    sync = run('SyncBN')                                                                 # no process group
    same(sync, ref)
    same(run('BN', convert=True), ref)
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % free_port(), rank=0, world_size=1)
    try:
        same(run('SyncBN'), ref)                                                         # inside a one-rank group
    finally:
        dist.destroy_process_group()
    # same names and state-dict keys: checkpoints load both ways
    assert list(sync[0].state_dict()) == list(ref[0].state_dict())
    sync[0].load_state_dict(ref[0].state_dict(), strict=True)
    ref[0].load_state_dict(sync[0].state_dict(), strict=True)


# ------------------------------------------------------------------------------------------------ 3. two ranks on the one GPU
SPLIT = (3, 1)          # four images: rank 0 holds three, rank 1 one

_WORKER = r'''
import os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, %(root)r)
rank, port, out = int(sys.argv[1]), sys.argv[2], sys.argv[3]
os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=port)
dist.init_process_group('gloo', rank=rank, world_size=2)          # both ranks share the one GPU: RCCL refuses that, gloo does not
solo = [dist.new_group([r]) for r in range(2)][rank]              # a one-rank group: a trainer on it reduces nothing
torch.cuda.set_device(0)
from oracle.gen_golden import CPR_CASES
from pointtinybenchmark_amd import synthetic
from pointtinybenchmark_amd.backbones.resnet import ResNet
from pointtinybenchmark_amd.training import BackwardEngine, CprTrainer
from tests.test_gpu_syncbn import SPLIT, build_locator, stage_douts, _batch
cfg = CPR_CASES['cpr_r18_c3_128']
lo, hi = sum(SPLIT[:rank]), sum(SPLIT[:rank + 1])
_, full = _batch(cfg, 4)
data = dict(img=full['img'][lo:hi].contiguous(), img_metas=full['img_metas'][lo:hi], gt_bboxes=full['gt_bboxes'][lo:hi],
            gt_labels=full['gt_labels'][lo:hi])
res = {}

# (a) (b) (c) (e): the backbone alone
sd = {k[len('backbone.'):]: v for k, v in synthetic.locator_state_dict(18, 1, 0, 'cpr', 3, 0.3).items() if k.startswith('backbone.')}
bb = ResNet(18, frozen_stages=1, norm_eval=False, norm_cfg=dict(type='SyncBN', requires_grad=True)).cuda()
bb.load_state_dict(sd, strict=True)
bb.train()
eng = BackwardEngine(bb)
eng._sink = {}
tape = []
outs = bb(data['img'], tape=tape)
assert all(g is not None for r in tape for g in r['groups'].values()), 'every trained BatchNorm must have synchronised'
douts = stage_douts([tuple(o.shape) for o in outs], 4)
d_stage = {i: douts[i][lo:hi].permute(0, 2, 3, 1).contiguous().cuda() for i in range(1, 4)}     # stage 0 is frozen
eng._backward_backbone(bb, tape, d_stage)
named = [(k, p) for k, p in bb.named_parameters() if p.requires_grad]
grads = eng.collect([p for _, p in named])
torch.cuda.synchronize()
res['outs'] = [o.cpu() for o in outs]
res['grads'] = {k: g.cpu() for (k, _), g in zip(named, grads)}
res['bufs'] = {k: v.cpu().clone() for k, v in bb.state_dict().items() if 'running' in k or 'num_batches' in k}
bb.eval()
with torch.no_grad():
    res['eval_outs'] = [o.cpu() for o in bb(data['img'])]
res['eval_sd'] = {k: v.cpu().clone() for k, v in bb.state_dict().items()}

# (d) one CprTrainer step on the world group; the bridge against a trainer that reduces nothing
m1, _ = build_locator(cfg, 'SyncBN')
tr = CprTrainer(m1, lr=0.01, bucket_mb=1.0, group=dist.group.WORLD)
tr.train_step(dict(data))
torch.cuda.synchronize()
res['p'] = tr.flat_p.cpu()
res['world'] = tr.buckets.world_size
res['step_bufs'] = {k: v.cpu().clone() for k, v in m1.state_dict().items() if 'running' in k}
m2, _ = build_locator(cfg, 'SyncBN')
t2 = CprTrainer(m2, group=solo)
t2.forward_backward(**data)
torch.cuda.synchronize()
want = {k: p.grad.clone() for k, p in m2.named_parameters() if p.requires_grad}
m3, _ = build_locator(cfg, 'SyncBN')
o3 = m3.train_step(dict(data))
o3['loss'].backward()
torch.cuda.synchronize()
res['bridge_equal'] = all(p.grad is not None and torch.equal(p.grad, want[k]) for k, p in m3.named_parameters() if p.requires_grad)
res['bridge_bufs_equal'] = all(torch.equal(v, m2.state_dict()[k]) for k, v in m3.state_dict().items() if 'running' in k)
torch.save(res, out + '.%%d' %% rank)
dist.destroy_process_group()
'''


def stage_douts(shapes, n_total):
    """Fixed random upstream gradients on the four stage outputs of the WHOLE batch (NCHW, CPU); a rank takes its images."""
    g = torch.Generator().manual_seed(11)
    return [torch.randn((n_total,) + tuple(s[1:]), generator=g) for s in shapes]


@pytest.fixture(scope='module')
def two_ranks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('syncbn')
    script = tmp / 'worker.py'
    script.write_text(_WORKER % dict(root=ROOT))
    port, out = str(free_port()), str(tmp / 'res')
    procs = [subprocess.Popen([sys.executable, str(script), str(r), port, out], cwd=ROOT, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=300)[0].decode(errors='replace'))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), '\n'.join(l[-3000:] for l in logs)
    return [torch.load(out + '.%d' % r) for r in range(2)]


@pytest.fixture(scope='module')
def four_image_oracle():
    """The fp64 restatement (oracle.cpr_oracle.resnet_forward in float64) on all four images with batch statistics over all four for the
    trained stages -- the patch of tests/test_gpu_bn_batch_stats._patch_oracle, scoped to this computation -- and its autograd under
    loss = sum_i <out_i, dout_i>."""
    from tests.test_gpu_bn_batch_stats import _stage_of
    cfg = CPR_CASES['cpr_r18_c3_128']
    b, _ = _batch(cfg, 4)
    sd = {k: v.double() for k, v in synthetic.locator_state_dict(18, 1, 0, 'cpr', 3, 0.3).items() if k.startswith('backbone.')}
    def stage(k):
        return 0 if k.startswith(('backbone.conv1', 'backbone.bn1')) else int(k[len('backbone.layer')])
    trainable = [k for k in sd if stage(k) > 1 and 'running' not in k and 'num_batches' not in k]       # frozen_stages=1
    for k in trainable:
        sd[k].requires_grad_(True)
    bufs = {}
    orig = O._bn_eval

    def bn(x, sdd, p, eps=1e-5):
        if _stage_of(p) <= 1:
            return orig(x, sdd, p, eps)
        bufs[p] = [sdd[p + '.running_mean'].detach().clone(), sdd[p + '.running_var'].detach().clone()]
        return F.batch_norm(x, bufs[p][0], bufs[p][1], sdd[p + '.weight'], sdd[p + '.bias'], True, 0.1, eps)
    O._bn_eval = bn
    try:
        outs = O.resnet_forward(sd, b['img'].double(), 18)
    finally:
        O._bn_eval = orig
    douts = stage_douts([tuple(o.shape) for o in outs], 4)
    sum((o * d.double()).sum() for o, d in zip(outs, douts)).backward()
    return dict(outs=[o.detach() for o in outs], grads={k[len('backbone.'):]: sd[k].grad for k in trainable}, bufs=bufs, img=b['img'])


def test_two_ranks_forward_matches_the_oracle_on_all_images(two_ranks, four_image_oracle):
    """(a) the stage outputs of the two ranks, concatenated, against batch statistics over all four images: the bar of
    test_backbone_forward_matches_patched_oracle."""
    for i, ref in enumerate(four_image_oracle['outs']):
        got = torch.cat([two_ranks[r]['outs'][i] for r in range(2)])
        assert got.shape == ref.shape and _rel_l2(got, ref) <= 1e-4, (i, _rel_l2(got, ref))


def test_two_ranks_summed_gradients_match_fp64_autograd(two_ranks, four_image_oracle):
    """(b) loss_r = <out_r, dout_r>: the sum over the ranks of the backbone parameter gradients against fp64 autograd of the restatement
    on all four images, at the end-to-end bars of batch statistics (tests/test_gpu_bn_batch_stats.py: one ReLU within
    rounding of 0 moves a channel's BatchNorm backward, so no fp32 implementation holds the eval-BN step's 2e-3)."""
    ref = four_image_oracle['grads']
    got = {k: two_ranks[0]['grads'][k].double() + two_ranks[1]['grads'][k].double() for k in two_ranks[0]['grads']}
    assert sorted(got) == sorted(ref)
    top = max(float(v.abs().max()) for v in ref.values())
    live = [k for k in sorted(ref) if float(ref[k].abs().max()) > 1e-6 * top]
    a = torch.cat([got[k].flatten() for k in live])
    b = torch.cat([ref[k].flatten() for k in live])
    cos = float(a @ b / (a.norm() * b.norm()))
    worst = sorted(((_rel_l2(got[k], ref[k]), k) for k in live), reverse=True)
    print('cosine %.6f, worst per-tensor rel-L2 %s' % (cos, worst[:3]))
    assert cos >= 0.999, cos
    assert worst[0][0] <= 5e-2, worst[:6]


def test_two_ranks_hold_the_same_running_buffers(two_ranks, four_image_oracle):
    """(c) running_mean / running_var / num_batches_tracked of every BatchNorm: torch.equal across the ranks (and, for the trained
    stages, the statistics of all four images)."""
    a, b = two_ranks[0]['bufs'], two_ranks[1]['bufs']
    assert list(a) == list(b) and len(a) == 3 * 20
    for k in a:
        assert torch.equal(a[k], b[k]), k
    n = 0
    for p, (rm, rv) in four_image_oracle['bufs'].items():
        q = p[len('backbone.'):]
        assert int(a[q + '.num_batches_tracked']) == 1
        for got, want in ((a[q + '.running_mean'], rm), (a[q + '.running_var'], rv)):
            assert torch.allclose(got.double(), want, rtol=1e-4, atol=1e-5 * float(want.abs().max())), q
        n += 1
    assert n == 15                                                   # layer2..layer4 of R18: 4 + 1 norms per stage


def test_two_ranks_trainer_step_and_bridge(two_ranks):
    """(d) one CprTrainer step with group=: the same parameters on both ranks; loss.backward() through the autograd bridge gives each
    rank the gradients of the native trainer (a trainer on a one-rank group: nothing reduced, BatchNorm still synchronised)."""
    assert two_ranks[0]['world'] == 2
    assert torch.equal(two_ranks[0]['p'], two_ranks[1]['p'])
    for k, v in two_ranks[0]['step_bufs'].items():
        assert torch.equal(v, two_ranks[1]['step_bufs'][k]), k
    for r in range(2):
        assert two_ranks[r]['bridge_equal'] and two_ranks[r]['bridge_bufs_equal'], r


def test_two_ranks_eval_folds_the_synchronised_buffers(two_ranks, four_image_oracle):
    """(e) model.eval() afterwards folds the buffers the synchronised forward left: the bar of
    test_eval_after_train_uses_the_updated_buffers."""
    lo = 0
    for r in range(2):
        sd = {'backbone.' + k: v for k, v in two_ranks[r]['eval_sd'].items()}
        ref = O.resnet_forward(sd, four_image_oracle['img'][lo:lo + SPLIT[r]], 18)
        lo += SPLIT[r]
        for a, b in zip(two_ranks[r]['eval_outs'], ref):
            assert _rel_l2(a, b) <= 1e-4


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_bf16_with_syncbn_batch_statistics_is_refused():
    from pointtinybenchmark_amd import autograd_bridge
    cfg = CPR_CASES['cpr_r18_c3_128']
    m, _ = build_locator(cfg, 'SyncBN')
    m.set_compute_dtype('bf16')
    _, data = _batch(cfg)
    assert 'norm_eval' in autograd_bridge.unsupported_reason(m)
    with torch.no_grad(), pytest.raises(NotImplementedError, match='norm_eval'):
        m.forward_train(**data)


def test_a_rank_without_rows_is_refused():
    C = 64
    with pytest.raises(ValueError, match='no rows'):
        ops.bn_sync_local_stats(torch.empty((0, 4, 4, C), device='cuda'))
    # more than one value per channel over the whole group: one rank with one row falls short, two one-row ranks do not
    y = torch.randn(1, 1, 1, C, device='cuda')
    rec, _ = ops.bn_sync_local_stats(y)
    ones, zeros = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
    with pytest.raises(ValueError, match='more than 1 value'):
        ops.bn_sync_merge_stats(rec[None], y, ones, zeros)
    y2 = torch.randn(1, 1, 1, C, device='cuda')
    st = ops.bn_sync_merge_stats(torch.stack([rec, ops.bn_sync_local_stats(y2)[0]]), y, ones, zeros)
    torch.cuda.synchronize()
    want = torch.cat([y, y2]).reshape(2, C).double().mean(0)
    assert torch.allclose(st.mean.double(), want, rtol=1e-6, atol=1e-7) and float(st.count) == 2.0
