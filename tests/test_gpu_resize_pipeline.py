"""-m gpu: the device Resize / test-time-augmentation pipeline (cpr_preprocess_jobs_u8, cpr_scale_clip_flip_boxes,
GpuImagePipeline, GpuTestTimeAug).  Pixels bit-equal to the numpy chain crop -> fixed-point resize -> flip -> image tail
(tests/test_resize_host.py, oracle.data_oracle.image_tail); boxes and metas equal to what the reference's own classes recorded in
tests/golden/resize_pipeline.json; the batches drive forward_train / forward_test to the same results as inputs built on the host.
Nothing here reads the reference tree."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import data_oracle as DO
from tests.test_resize_host import MEAN, STD, build_pipeline, case_image, f32, load_golden, numpy_chain

pytestmark = pytest.mark.gpu
GOLD = load_golden()['cases']
TRAIN_CASES = sorted(k for k, c in GOLD.items() if 'draws' in c)
AUG_CASES = sorted(k for k, c in GOLD.items() if 'augs' in c)


def _boxes(case):
    return f32(case['boxes_bits']).reshape(-1, 4)


def _sample(case):
    b = _boxes(case)
    return dict(img=case_image(case), gt_bboxes=b, gt_labels=np.zeros(len(b), np.int64), filename='a.jpg')


def _check_image(nhwc, want):
    """nhwc (Hp, Wp, 4) from the device against the numpy chain's (ph, pw, 3): bit-equal, zeros everywhere else."""
    ph, pw = want.shape[:2]
    assert nhwc.shape[0] >= ph and nhwc.shape[1] >= pw
    assert np.array_equal(nhwc[:ph, :pw, :3], want)
    assert not nhwc[:, :, 3].any() and not nhwc[ph:].any() and not nhwc[:, pw:].any()


def _check_meta(m, ref):
    assert list(m['img_shape']) == ref['img_shape'] and list(m['pad_shape']) == ref['pad_shape']
    assert m['flip'] == ref['flip'] and m['flip_direction'] == ref['flip_direction']
    assert m['scale_factor'].dtype == np.float32 and m['scale_factor'].view(np.uint32).tolist() == ref['scale_factor_bits']
    if ref.get('tile_offset') is not None:
        assert list(m['tile_offset']) == ref['tile_offset']
    else:
        assert 'tile_offset' not in m


@pytest.mark.parametrize('name', TRAIN_CASES)
def test_resized_batch_matches_numpy_chain_and_reference_records(name):
    """One image N times through one random stream (ragged outputs where the scale is drawn): pixels, boxes, metas."""
    case = GOLD[name]
    pipe = build_pipeline(case, 'cuda')
    s = _sample(case)
    batch = pipe([s] * len(case['draws']), np.random.RandomState(case['seed']))
    nhwc = batch['img'].permute(0, 2, 3, 1).cpu().numpy()
    assert batch['img'].shape[1] == 4 and batch['img'].stride(1) == 1 and nhwc.shape[1] % 32 == 0 and nhwc.shape[2] % 32 == 0
    h, w = case['hw']
    for i, ref in enumerate(case['draws']):
        dh, dw = ref['img_shape'][:2]
        _check_image(nhwc[i], numpy_chain(s['img'], (0, 0, w, h), dw, dh, ref['flip']))
        _check_meta(batch['img_metas'][i], ref)
        got = batch['gt_bboxes'][i].cpu().numpy()
        assert got.view(np.uint32).tolist() == ref['boxes_bits'], 'boxes of draw %d' % i


def test_ragged_batch_is_one_launch_of_different_sources():
    """Two different decoded sizes at (667, 400) plus an up-scaled portrait image: every slot padded to the batch maximum."""
    from pointtinybenchmark_amd.datasets import GpuImagePipeline
    cases = [GOLD['coco_480x640_at_667x400'], GOLD['coco_427x640_at_667x400'], dict(GOLD['coco_500x375_at_1333x800'], hw=[250, 187])]
    samples = [_sample(c) for c in cases]
    pipe = GpuImagePipeline(img_scale=(667, 400), flip_ratio=0.5)

    class Draws:
        vals = [0.9, 0.1, 0.2]

        def rand(self):
            return self.vals.pop(0)
    batch = pipe(samples, Draws())
    nhwc = batch['img'].permute(0, 2, 3, 1).cpu().numpy()
    assert nhwc.shape[:3] == (3, 544, 608)
    for i, (s, flip, (dh, dw)) in enumerate(zip(samples, (False, True, True), ((400, 533), (400, 600), (535, 400)))):
        h, w = s['img'].shape[:2]
        assert batch['img_metas'][i]['img_shape'] == (dh, dw, 3) and batch['img_metas'][i]['flip'] == flip
        _check_image(nhwc[i], numpy_chain(s['img'], (0, 0, w, h), dw, dh, flip))


@pytest.mark.parametrize('name', AUG_CASES)
def test_test_time_augmentations_match_numpy_chain_and_reference_records(name):
    """Tiles (also pulled back to the border, also of an image smaller than the tile) x scales x flips from one upload."""
    case = GOLD[name]
    tta = build_pipeline(case, 'cuda')
    s = _sample(case)
    out = tta(s)
    assert len(out['img']) == len(out['img_metas']) == len(out['gt_bboxes']) == len(case['augs'])
    for img, metas, boxes, ref in zip(out['img'], out['img_metas'], out['gt_bboxes'], case['augs']):
        assert img.shape[0] == 1 and img.shape[1] == 4 and img.stride(1) == 1 and len(metas) == 1 and len(boxes) == 1
        assert list(img.shape[2:]) == ref['pad_shape'][:2]
        dh, dw = ref['img_shape'][:2]
        _check_image(img.permute(0, 2, 3, 1)[0].cpu().numpy(), numpy_chain(s['img'], tuple(ref['crop']), dw, dh, ref['flip']))
        _check_meta(metas[0], ref)
        assert boxes[0].cpu().numpy().view(np.uint32).tolist() == ref['boxes_bits']


def _legacy_kernel(imgs, flips, Hp, Wp):
    """cpr_preprocess_u8 called directly on a stack of equally sized images: the output the scale-1 path has always had."""
    from pointtinybenchmark_amd import _lib, ops
    stack = torch.from_numpy(np.stack(imgs)).cuda()
    n, H, W = stack.shape[:3]
    out = torch.empty((n, Hp, Wp, 4), device='cuda', dtype=torch.float32)
    m = (ctypes.c_float * 3)(*np.array(MEAN, np.float32).tolist())
    sd = (ctypes.c_float * 3)(*(1.0 / np.float64(np.array(STD, np.float32))).astype(np.float32).tolist())
    _lib.call('cpr_preprocess_u8', ops._ptr(stack), ops._ptr(torch.tensor(flips, dtype=torch.int32, device='cuda')),
              ctypes.cast(m, ctypes.c_void_p), ctypes.cast(sd, ctypes.c_void_p), 1, ops._ptr(out), n, H, W, Hp, Wp, ops._stream())
    return out


def test_scale_one_paths_keep_their_bits():
    """Resize(scale_factor=[1.0]): a single-shape batch still runs the stacked kernel and equals its output bit for bit; a ragged
    one (now one launch of the job kernel, identity resize) equals the per-image launches it replaces."""
    from pointtinybenchmark_amd.datasets import GpuImagePipeline
    rng = np.random.RandomState(5)
    pipe = GpuImagePipeline(flip_ratio=0.5)
    assert not pipe.resizes

    class Draws:
        def __init__(self, vals):
            self.vals = list(vals)

        def rand(self):
            return self.vals.pop(0)
    imgs = [rng.randint(0, 256, (96, 130, 3)).astype(np.uint8) for _ in range(3)]
    box = np.array([[-3.0, 4.0, 20.0, 99.0], [100.0, 10.0, 140.0, 50.0]], np.float32)
    batch = pipe([dict(img=im, gt_bboxes=box, gt_labels=np.zeros(2, np.int64)) for im in imgs], Draws([0.1, 0.9, 0.3]))
    want = _legacy_kernel(imgs, [1, 0, 1], 96, 160)
    assert torch.equal(batch['img'].permute(0, 2, 3, 1), want)
    for i, flip in enumerate((True, False, True)):
        b = DO.resize_clip_bboxes(box, (96, 130, 3))
        assert np.array_equal(batch['gt_bboxes'][i].cpu().numpy(), DO.bbox_flip(b, (96, 130)) if flip else b)
        assert batch['img_metas'][i]['scale_factor'].tolist() == [1.0] * 4 and batch['img_metas'][i]['pad_shape'] == (96, 160, 3)
    ragged = [rng.randint(0, 256, hw + (3,)).astype(np.uint8) for hw in ((100, 90), (64, 127), (97, 33))]
    batch = pipe([dict(img=im, gt_bboxes=box, gt_labels=np.zeros(2, np.int64)) for im in ragged], Draws([0.1, 0.9, 0.3]))
    nhwc = batch['img'].permute(0, 2, 3, 1)
    assert tuple(nhwc.shape) == (3, 128, 128, 4)
    for i, (im, flip) in enumerate(zip(ragged, (1, 0, 1))):
        assert torch.equal(nhwc[i:i + 1], _legacy_kernel([im], [flip], 128, 128)), i
        b = DO.resize_clip_bboxes(box, im.shape)
        assert np.array_equal(batch['gt_bboxes'][i].cpu().numpy(), DO.bbox_flip(b, im.shape[:2]) if flip else b)


def _numpy_boxes(boxes, sf4, img_shape, flip):
    """Resize._resize_bboxes then RandomFlip.bbox_flip, restated (pinned against the reference bodies by the golden file)."""
    b = DO.resize_clip_bboxes((boxes * sf4).astype(np.float32), img_shape)
    return DO.bbox_flip(b, img_shape[:2]) if flip else b


def test_resized_ragged_batch_feeds_forward_train():
    """Two ragged images at (667, 400) through the pipeline and forward_train of the small R18 CPR model: the same losses as the float
    NCHW batch and boxes built on the host by the numpy chain."""
    from oracle.gen_golden import CPR_CASES
    from pointtinybenchmark_amd.datasets import GpuImagePipeline
    from tests.test_gpu_cpr_parity import build_hip_locator
    m, _ = build_hip_locator(CPR_CASES['cpr_r18_c3_128'])
    rng = np.random.RandomState(11)
    samples = []
    for k, (h, w) in enumerate(((480, 640), (427, 640))):
        xy = rng.uniform(8, min(h, w) - 8, (4 + k, 2)).astype(np.float32)
        boxes = np.concatenate([xy - 8, xy + 8], 1)
        samples.append(dict(img=rng.randint(0, 256, (h, w, 3)).astype(np.uint8), gt_bboxes=boxes,
                            gt_labels=np.arange(len(boxes), dtype=np.int64) % 3, gt_bboxes_ignore=np.zeros((0, 4), np.float32),
                            gt_true_bboxes=boxes + 1))

    class Draws:
        vals = [0.7, 0.2]

        def rand(self):
            return self.vals.pop(0)
    pipe = GpuImagePipeline(img_scale=(667, 400), flip_ratio=0.5)
    batch = pipe(samples, Draws())
    sizes, flips = ((400, 533), (400, 600)), (False, True)
    nchw = np.zeros((2, 3, 416, 608), np.float32)
    gtb = []
    for i, (s, (dh, dw), flip) in enumerate(zip(samples, sizes, flips)):
        h, w = s['img'].shape[:2]
        t = numpy_chain(s['img'], (0, 0, w, h), dw, dh, flip)
        nchw[i, :, :t.shape[0], :t.shape[1]] = t.transpose(2, 0, 1)
        sf4 = np.array([dw / w, dh / h, dw / w, dh / h], dtype=np.float32)
        gtb.append(torch.from_numpy(_numpy_boxes(s['gt_bboxes'], sf4, (dh, dw, 3), flip)).cuda())
        assert torch.equal(batch['gt_bboxes'][i], gtb[i])
    assert tuple(batch['img'].shape) == (2, 4, 416, 608)
    with torch.no_grad():
        a = m.forward_train(batch['img'], batch['img_metas'], batch['gt_bboxes'], batch['gt_labels'])
        b = m.forward_train(torch.from_numpy(nchw).cuda(), batch['img_metas'], gtb, batch['gt_labels'])
    a, b = {k: float(v) for k, v in a.items()}, {k: float(v) for k, v in b.items()}
    assert a == b and all(np.isfinite(v) for v in a.values()), (a, b)


def test_tiled_flipped_image_feeds_forward_test():
    """One 300x200 image through GpuTestTimeAug (128x128 tiles, 32 px overlap, flip) and forward_test of the small P2P model: the same
    detections as the lists of float NCHW tiles and metas built on the host by the numpy chain."""
    import pointtinybenchmark_amd as P
    from bench import p2p_model_cfg
    from pointtinybenchmark_amd import synthetic
    m = P.build_detector(p2p_model_cfg(18)).cuda()
    m.load_state_dict(synthetic.locator_state_dict(18, 1, 0, 'p2p', 5, head_std=0.15), strict=True)
    m.eval()
    case = GOLD['tiles_300x200_flip']
    img = case_image(case)
    tta = build_pipeline(case, 'cuda')
    out = tta(dict(img=img))
    assert len(out['img']) == 12 and set(out) == {'img', 'img_metas'}
    imgs, metas = [], []
    for ref in case['augs']:
        dh, dw = ref['img_shape'][:2]
        t = numpy_chain(img, tuple(ref['crop']), dw, dh, ref['flip'])
        imgs.append(torch.from_numpy(np.ascontiguousarray(t.transpose(2, 0, 1)[None])).cuda())
        metas.append([dict(img_shape=tuple(ref['img_shape']), pad_shape=tuple(ref['pad_shape']),
                           scale_factor=f32(ref['scale_factor_bits']), flip=ref['flip'], flip_direction=ref['flip_direction'],
                           tile_offset=tuple(ref['tile_offset']))])
    with torch.no_grad():
        (dets, labels), = m.forward_test(out['img'], out['img_metas'], rescale=True)
        (d2, l2), = m.forward_test(imgs, metas, rescale=True)
    assert dets.shape[0] > 0 and dets.shape[1] == 5
    assert torch.equal(dets, d2) and torch.equal(labels, l2)


def test_bad_job_tables_are_argument_errors():
    """Nothing is launched: the entry point refuses a null table, ops.preprocess_jobs refuses geometry that leaves the image or the
    output on the host copy of the table."""
    from pointtinybenchmark_amd import _lib, ops
    out = torch.zeros((64 * 64 * 4,), device='cuda')
    m = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    with pytest.raises(_lib.CprHipError, match='invalid argument'):
        _lib.call('cpr_preprocess_jobs_u8', None, 3, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(m, ctypes.c_void_p), 1,
                  ops._ptr(out), 64 * 64, ops._stream())
    with pytest.raises(_lib.CprHipError, match='invalid argument'):
        _lib.call('cpr_preprocess_jobs_u8', ops._ptr(out), -1, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(m, ctypes.c_void_p), 1,
                  ops._ptr(out), 64 * 64, ops._stream())
    assert _lib.call('cpr_preprocess_jobs_u8', None, 0, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(m, ctypes.c_void_p), 1,
                     ops._ptr(out), 64 * 64, ops._stream()) == 0
    src = torch.zeros((32, 48, 3), dtype=torch.uint8, device='cuda')
    good = dict(src=src.data_ptr(), out_off=0, pitch=48 * 3, src_w=48, src_h=32, x0=8, y0=8, cw=40, ch=24, dw=64, dh=40, flip=0,
                Hp=64, Wp=64)

    def table(**kw):
        j = np.zeros((1,), dtype=np.dtype(ops.PREPROCESS_JOB))
        for k, v in dict(good, **kw).items():
            j[k] = v
        return j
    for bad in (dict(cw=41), dict(y0=9), dict(x0=-1), dict(src=0), dict(dw=0), dict(dh=65), dict(out_off=1), dict(pitch=100)):
        with pytest.raises(_lib.CprHipError, match='invalid argument'):
            ops.preprocess_jobs(table(**bad), MEAN, STD, True, out)
    ops.preprocess_jobs(table(), MEAN, STD, True, out)
    torch.cuda.synchronize()
    assert not bool(out.view(64, 64, 4)[40:].any()) and not bool(out.view(64, 64, 4)[:, :, 3].any())
    assert bool(torch.isfinite(out).all())
