"""The trainable ResNet stem (frozen_stages=-1) on the host: the native trainer's parameter order and the autograd bridge's
support check.  CPU only: no kernel runs."""
import pytest
import torch
import torch.nn as nn

import pointtinybenchmark_amd as P
from pointtinybenchmark_amd.autograd_bridge import unsupported_reason
from pointtinybenchmark_amd.training import P2PTrainer


def _model(frozen_stages, norm_eval=True, depth=18):
    from bench import p2p_model_cfg
    cfg = p2p_model_cfg(depth)
    cfg['backbone'].update(frozen_stages=frozen_stages, norm_eval=norm_eval)
    m = P.build_detector(cfg)
    m.train()
    return m


def _order(m):
    t = P2PTrainer.__new__(P2PTrainer)
    t.model = m
    return t._backward_order()


@pytest.mark.parametrize('depth', [18, 50])
def test_backward_order_puts_the_stem_last(depth):
    m = _model(-1, depth=depth)
    bb = m.backbone
    order = _order(m)
    assert order[-3:] == [bb.conv1.weight, bb.bn1.weight, bb.bn1.bias]
    assert {id(p) for p in order} == {id(p) for p in m.parameters() if p.requires_grad}
    # every model with a frozen stem keeps its layout: the same list as before, i.e. without the three stem entries
    m0 = _model(0, depth=depth)
    assert [n for n, _ in _named(m0, _order(m0))] == [n for n, _ in _named(m, order)][:-3]


def _named(m, order):
    names = {id(p): n for n, p in m.named_parameters()}
    return [(names[id(p)], p) for p in order]


@pytest.mark.parametrize('frozen_stages', [0, 1, 2])
def test_backward_order_unchanged_with_a_frozen_stem(frozen_stages):
    m = _model(frozen_stages)
    order = _order(m)
    assert not any(p is m.backbone.conv1.weight or p is m.backbone.bn1.weight for p in order)
    assert {id(p) for p in order} == {id(p) for p in m.parameters() if p.requires_grad}


def test_bridge_accepts_the_standard_stem_and_refuses_the_rest():
    m = _model(-1)
    assert unsupported_reason(m) is None
    m = _model(-1, norm_eval=False)
    assert unsupported_reason(m) is None
    m.backbone.compute_dtype = torch.bfloat16            # bf16 together with batch statistics stays refused
    assert 'batch statistics' in unsupported_reason(m)
    m = _model(-1)
    m.backbone.conv1 = nn.Conv2d(3, 64, 5, 2, 2, bias=False)
    reason = unsupported_reason(m)
    assert reason is not None and '(64, 3, 5, 5)' in reason
    m = _model(-1)
    for p in m.backbone.layer1.parameters():
        p.requires_grad_(False)
    assert 'layer1' in unsupported_reason(m)


def test_frozen_conv1_with_a_trainable_bn1_keeps_its_rule():
    m = _model(-1)
    m.backbone.conv1.weight.requires_grad_(False)
    bb = m.backbone
    order = _order(m)
    assert order[-2:] == [bb.bn1.weight, bb.bn1.bias]
    assert {id(p) for p in order} == {id(p) for p in m.parameters() if p.requires_grad}
    assert unsupported_reason(m) is None
