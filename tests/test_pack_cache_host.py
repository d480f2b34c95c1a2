"""The pack cache's in-place refresh protocol without a GPU (layers._PackCache): which jobs ``refresh_all`` selects, the device
tables it builds and the entries it re-stamps.  CPU tensors stand in for the device ones and the C ABI is recorded, not called."""
import ctypes
import struct
import types

import pytest
import torch
import torch.nn as nn

from pointtinybenchmark_amd import _lib, layers, ops


@pytest.fixture
def launches(monkeypatch):
    """Every multi-tensor launch refresh_all makes, as (function, job count, launch extent, table bytes)."""
    got = []

    def call(fn, table, n, extent, stream):
        got.append((fn, n, extent, ctypes.string_at(table, 64 * n)))
    monkeypatch.setattr(_lib, 'call', call)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)       # no producer events
    monkeypatch.setattr(layers, 'REFRESH_IN_PLACE', [True])
    return got


def fold(cache, bn, job=True):
    """A folded-BN entry whose refresh is a FoldJob (job=False: the rebuilt value has none)."""
    def make():
        with torch.no_grad():
            scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).contiguous()
            return scale, (bn.bias - bn.running_mean * scale).contiguous()
    return cache.get(('bn', id(bn)), [bn.weight, bn.bias, bn.running_mean, bn.running_var], make,
                     lambda val: layers.FoldJob(bn, val) if job else None)


def dgrad(cache, conv, bn, dtype=torch.float32):
    """A data-gradient pack linked to the fold job of ``bn``."""
    scale, _ = fold(cache, bn)
    w = conv.weight
    return cache.get(('dgrad', id(conv), dtype), [w, bn.weight, bn.running_var],
                     lambda: ops.PackedConv((w.detach() * scale[:, None, None, None]).flip(2, 3).permute(1, 0, 2, 3), 1, 1, dtype),
                     lambda pc: layers.PackJob(w, pc, 1, cache._jobs[('bn', id(bn))]))


def stale(cache, key):
    """True when the next ``get`` of ``key`` rebuilds the entry: its version moved and nothing re-stamped it."""
    e = cache._d[key]
    return e.ver != cache._ver(e.tensors)


def test_a_rebuild_without_a_job_leaves_no_job(launches):
    c, t = layers._PackCache(), torch.zeros(4)
    c.get('k', [t], lambda: 'old', lambda val: types.SimpleNamespace(value=val, fold=None))
    assert 'k' in c._jobs
    t.add_(1.0)                                  # the version moves: the next get rebuilds
    assert c.get('k', [t], lambda: 'new', lambda val: None) == 'new'
    assert 'k' not in c._jobs
    c.refresh_all()
    assert launches == []


def test_b_a_job_whose_value_is_not_the_entry_value_is_never_refreshed(launches):
    c, bn = layers._PackCache(), nn.BatchNorm2d(64)
    fold(c, bn)
    layers.bump_weight_epoch()
    c.refresh_all()
    assert [fn for fn, *_ in launches] == ['cpr_bn_fold_multi']
    assert not stale(c, ('bn', id(bn)))           # refreshed: re-stamped with the new epoch

    # a refresh callable that hands back a job for some other value
    c2, bn2 = layers._PackCache(), nn.BatchNorm2d(64)
    c2.get(('bn', id(bn2)), [bn2.weight, bn2.bias, bn2.running_mean, bn2.running_var], lambda: (torch.ones(64), torch.zeros(64)),
           lambda val: layers.FoldJob(bn2, (torch.ones(64), torch.zeros(64))))
    assert c2._live() == []

    # the stale-job sequence: a job, the version moves, the same key rebuilt by a refresh that has no job
    with torch.no_grad():
        bn.weight.mul_(2.0)
    fold(c, bn, job=False)
    layers.bump_weight_epoch()
    launches.clear()
    c.refresh_all()
    assert launches == []
    assert stale(c, ('bn', id(bn)))               # not re-stamped: the new value is rebuilt from the current weights


def test_c_a_pack_whose_fold_was_rebuilt_is_not_refreshed(launches):
    c, bn, conv = layers._PackCache(), nn.BatchNorm2d(64), nn.Conv2d(32, 64, 3, padding=1, bias=False)
    dgrad(c, conv, bn)
    assert [type(j) for j in c._jobs.values()] == [layers.FoldJob, layers.PackJob]
    assert c._jobs[('dgrad', id(conv), torch.float32)].fold is c._jobs[('bn', id(bn))]
    with torch.no_grad():
        bn.running_mean.add_(1.0)                # the fold (not the pack: running_mean is not among its tensors) is rebuilt
    fold(c, bn)
    live = [j for _, j in c._live()]
    assert live == [c._jobs[('bn', id(bn))]]
    layers.bump_weight_epoch()
    c.refresh_all()
    assert [(fn, n) for fn, n, *_ in launches] == [('cpr_bn_fold_multi', 1)]
    assert stale(c, ('dgrad', id(conv), torch.float32))


def test_d_refresh_in_place_off_selects_and_launches_nothing(launches):
    c, bn, conv = layers._PackCache(), nn.BatchNorm2d(64), nn.Conv2d(32, 64, 3, padding=1, bias=False)
    dgrad(c, conv, bn)
    layers.REFRESH_IN_PLACE[0] = False           # jobs registered before the switch stay inactive
    layers.bump_weight_epoch()
    assert c._live() == []
    c.refresh_all()
    assert launches == []
    assert all(stale(c, k) for k in c._d)
    layers.REFRESH_IN_PLACE[0] = True
    layers.bump_weight_epoch()
    c.refresh_all()
    assert [fn for fn, *_ in launches] == ['cpr_bn_fold_multi', 'cpr_pack_weights_multi']
    assert not any(stale(c, k) for k in c._d)


def test_tables_hold_the_csrc_pack_hip_rows_and_are_rebuilt_only_when_they_change(launches):
    c = layers._PackCache()
    bn, bn2 = nn.BatchNorm2d(64), nn.BatchNorm2d(128)
    conv = nn.Conv2d(64, 64, 3, padding=1, bias=False)
    conv16 = nn.Conv2d(64, 128, 1, bias=False)
    pc32 = dgrad(c, conv, bn)
    pc16 = dgrad(c, conv16, bn2, torch.bfloat16)
    fold2 = c._jobs[('bn', id(bn2))].value
    layers.bump_weight_epoch()
    c.refresh_all()
    (f, nf, max_c, ft), (p, np16, blocks16, pt), (q, np32, blocks32, qt) = launches
    assert (f, p, q) == ('cpr_bn_fold_multi', 'cpr_pack_weights_bf16_multi', 'cpr_pack_weights_multi')
    assert (nf, np16, np32, max_c) == (2, 1, 1, 128)
    # FoldJob: gamma, beta, mean, var, scale, shift, inv (null), C, eps
    assert struct.unpack('<7Qif', ft[64:]) == (bn2.weight.data_ptr(), bn2.bias.data_ptr(), bn2.running_mean.data_ptr(),
                                               bn2.running_var.data_ptr(), fold2[0].data_ptr(), fold2[1].data_ptr(), 0, 128,
                                               pytest.approx(1e-5))
    # PackJob (bf16): w, scale, out, frag (null), O, I, KH, KW, transpose, block0, nblocks, pad; 128 x 64 x 1 x 1 -> 16 blocks
    assert struct.unpack('<4Q8i', pt) == (conv16.weight.data_ptr(), fold2[0].data_ptr(), pc16.w.data_ptr(), 0,
                                          128, 64, 1, 1, 1, 0, 16, 0) and blocks16 == 16
    # Pack32Job: w, scale, out, nblocks, pad, O, I, KH, KW, colsp, Kpad, transpose, block0; 64 rows x 576 -> 64 blocks (the cap)
    assert struct.unpack('<3Q10i', qt) == (conv.weight.data_ptr(), c._jobs[('bn', id(bn))].value[0].data_ptr(), pc32.w.data_ptr(),
                                           64, 0, 64, 64, 3, 3, 64, 576, 1, 0) and blocks32 == 64
    assert not any(stale(c, k) for k in c._d)

    tables = c._tables
    layers.bump_weight_epoch()
    c.refresh_all()
    assert c._tables is tables                  # same pointers, same jobs: the device tables are reused
    with torch.no_grad():
        conv.weight.mul_(0.5)                   # the fp32 pack is rebuilt: its output buffer moves
    assert dgrad(c, conv, bn) is not pc32       # (pc32 stays referenced: its buffer cannot be handed to the new pack)
    layers.bump_weight_epoch()
    c.refresh_all()
    assert c._tables is not tables
