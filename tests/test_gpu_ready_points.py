"""-m gpu: the ready points of the backbone families (tests/ready_point_check.py): one forward_backward of the checked trainer per family,
on the locator, input size and batch of that family's own GPU test file.  At every ``_done`` the declared prefix of the NaN-filled flat
buffer is written, the points sweep the buffer front to back and reach its end, and the whole buffer is finite afterwards."""
import pytest

from tests.ready_point_check import run_checked_backward

pytestmark = pytest.mark.gpu


def _res2net():
    from tests import test_gpu_res2net as T
    img, metas, boxes, labels = T._batch()
    return 'p2p', T._locator('p2p', frozen_stages=1), dict(img=img, img_metas=metas, gt_bboxes=boxes, gt_labels=labels)


def _resnest():
    from tests import test_gpu_resnest as T
    img, metas, boxes, labels = T._batch()
    return 'p2p', T._locator('p2p', frozen_stages=1), dict(img=img, img_metas=metas, gt_bboxes=boxes, gt_labels=labels)


def _resnext():
    from tests import test_gpu_resnext as T
    return 'cpr', T._locator(), T._data()


def _regnet(arch):
    from tests import test_gpu_regnet as T
    return 'p2p', T._locator('p2p', arch=arch), T._data()


def _mobilenet_v2():
    from tests import test_gpu_mobilenet_v2 as T
    return 'p2p', T._locator('p2p'), T._data()


def _hrnet_hrfpn():
    from tests import test_gpu_hrnet as T
    return 'p2p', T.build_locator('p2p_hrfpn'), T._data()


def _r50_batch_stats():
    from oracle.gen_golden import CPR_CASES
    from tests import test_gpu_bn_batch_stats as T
    cfg = CPR_CASES['cpr_r50_c1_160_spread']
    return 'cpr', T._bs_locator(cfg)[0], T._batch(cfg)[1]


def _r18_trainable_stem():
    from tests import test_gpu_stem_train as T
    return 'p2p', T._p2p_model(), T._p2p_data()


def _r50_v1d():
    from tests import test_gpu_resnet_variants as T
    return 'p2p', T._locator('p2p', 'v1d', 50), T._data((70, 90))


def _r50_dilated():
    from tests import test_gpu_dilated as T
    return 'p2p', T._locator('p2p', depth=50), T._data('p2p')


FAMILIES = {
    'res2net': _res2net,
    'resnest': _resnest,
    'resnext': _resnext,
    'regnetx_1.6gf_padded': lambda: _regnet('regnetx_1.6gf'),
    'regnetx_800mf': lambda: _regnet('regnetx_800mf'),
    'mobilenet_v2_trainable_stem': _mobilenet_v2,
    'hrnet_w32_tiny_hrfpn': _hrnet_hrfpn,
    'r50_norm_eval_false': _r50_batch_stats,
    'r18_frozen_stages_-1': _r18_trainable_stem,
    'r50_deep_stem_avg_down': _r50_v1d,
    'r50_dilated': _r50_dilated,
}


@pytest.mark.parametrize('family', list(FAMILIES))
def test_ready_points_only_cover_finished_gradients(family):
    from pointtinybenchmark_amd.training import CprTrainer, P2PTrainer
    head, m, data = FAMILIES[family]()
    assert any(p.requires_grad for p in m.backbone.parameters()), 'the family under test must train'
    tr, seen = run_checked_backward(CprTrainer if head == 'cpr' else P2PTrainer, m, data)
    assert {id(p) for p in tr.params} == {id(p) for p in m.parameters() if p.requires_grad}
    # the backbone's own ready points were reached: more points than the head and the neck alone declare
    first_bb = min(tr.offset[id(p)][0] for p in m.backbone.parameters() if p.requires_grad)
    assert sum(1 for end in seen if end > first_bb) >= 2, seen
