"""Host side of the device Resize / test-time-augmentation pipeline (no GPU):

* ``resize_linear_u8``: OpenCV's 8-bit fixed-point ``cv2.resize(..., INTER_LINEAR)`` restated in plain integer arithmetic -- the
  contract the HIP kernel (csrc/preprocess.hip, cpr_preprocess_jobs_u8) is held to bit for bit by tests/test_gpu_resize_pipeline.py.
  cv2 is un-vendored and not installed: PARITY UNPINNED.  What CAN be checked is checked here: identity sizes return the source, and
  every pixel stays within the scheme's own rounding budget of an fp64 bilinear with the same half-pixel geometry.
* The host restatement of Resize / MultiScaleFlipAug / CroppedTilesFlipAug (sizes, scale_factor, random draws, augmentation order)
  against tests/golden/resize_pipeline.json, recorded by tools/gen_resize_golden.py from the reference's own classes.
* ``GpuImagePipeline.from_config`` on the shipped train / test pipelines (needs the reference tree; skipped without it)."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'resize_pipeline.json')
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


# ---------------------------------------------------------------------------------------------------------------- the contract
def linear_taps(s, d, clamp_coefficient):
    """Per axis of cv2.resize INTER_LINEAR, 8-bit: source extent s -> d.  Returns (k0, k1, c0, c1): the two tap indices and their
    11-bit coefficients for every output index.
    x axis (clamp_coefficient=True): a tap that leaves the source is clamped AND its fraction zeroed (xofs / ialpha of resize.cpp).
    y axis (False): the fraction stays, the two ROWS are clamped (yofs / ibeta; resizeGeneric_Invoker clips sy + k)."""
    i = np.arange(d, dtype=np.float64)
    scale = 1.0 / (float(d) / s)
    f = ((i + 0.5) * scale - 0.5).astype(np.float32)
    k = np.floor(f).astype(np.int64)
    f = (f - k.astype(np.float32)).astype(np.float32)
    if clamp_coefficient:
        lo, hi = k < 0, k >= s - 1
        k[lo], f[lo] = 0, 0
        k[hi], f[hi] = s - 1, 0
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)     # saturate_cast<short>: rint, half to even
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return np.clip(k, 0, s - 1), np.clip(k + 1, 0, s - 1), c0, c1


def resize_linear_u8(img, dw, dh):
    """uint8 (h, w, c) -> uint8 (dh, dw, c): horizontal pass in int32, vertical pass with the >> 4, >> 16, + 2 >> 2 shifts."""
    sh, sw = img.shape[:2]
    kx0, kx1, a0, a1 = linear_taps(sw, dw, True)
    ky0, ky1, b0, b1 = linear_taps(sh, dh, False)
    S = img.astype(np.int64)
    R = S[:, kx0] * a0[None, :, None] + S[:, kx1] * a1[None, :, None]
    R0, R1 = R[ky0], R[ky1]
    u = (((b0[:, None, None] * (R0 >> 4)) >> 16) + ((b1[:, None, None] * (R1 >> 4)) >> 16) + 2) >> 2
    return np.clip(u, 0, 255).astype(np.uint8)


def bilinear_fp64(img, dw, dh):
    """Exact bilinear with the same half-pixel geometry (= F.interpolate(mode='bilinear', align_corners=False) in fp64)."""
    def axis(s, d):
        f = np.clip((np.arange(d, dtype=np.float64) + 0.5) * (s / d) - 0.5, 0, s - 1)
        k = np.minimum(np.floor(f).astype(np.int64), max(s - 2, 0))
        return k, np.minimum(k + 1, s - 1), f - k
    sh, sw = img.shape[:2]
    kx0, kx1, fx = axis(sw, dw)
    ky0, ky1, fy = axis(sh, dh)
    S = img.astype(np.float64)
    R = S[:, kx0] * (1 - fx)[None, :, None] + S[:, kx1] * fx[None, :, None]
    return R[ky0] * (1 - fy)[:, None, None] + R[ky1] * fy[:, None, None]


def numpy_chain(img, crop, dw, dh, flip, size_divisor=32, mean=MEAN, std=STD, to_rgb=True):
    """crop -> fixed-point resize -> flip -> Normalize -> Pad, as (Hp, Wp, 3) float32 (oracle.data_oracle.image_tail is the tail)."""
    from oracle import data_oracle as DO
    x0, y0, cw, ch = crop
    r = resize_linear_u8(np.ascontiguousarray(img[y0:y0 + ch, x0:x0 + cw]), dw, dh)
    return DO.image_tail(r, flip, mean, std, to_rgb, size_divisor)


def case_image(case):
    h, w = case['hw']
    return np.random.RandomState(case['seed'] + 1000).randint(0, 256, (h, w, 3)).astype(np.uint8)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def build_pipeline(case, device='cpu'):
    """The golden case's Resize / wrapper arguments -> GpuImagePipeline or GpuTestTimeAug."""
    from pointtinybenchmark_amd.datasets import GpuImagePipeline, GpuTestTimeAug

    def tup(v):
        return [tuple(x) for x in v] if isinstance(v[0], list) else tuple(v)
    kw = dict(case['resize'])
    if kw.get('img_scale') is not None:
        kw['img_scale'] = tup(kw['img_scale'])
    if kw.get('ratio_range') is not None:
        kw['ratio_range'] = tuple(kw['ratio_range'])
    if 'wrapper' not in case:
        return GpuImagePipeline(flip_ratio=case['flip_ratio'], device=device, **kw)
    w = dict(case['wrapper'])
    for k in ('img_scale', 'tile_shape', 'tile_overlap'):
        if w.get(k) is not None:
            w[k] = tup(w[k])
    return GpuTestTimeAug(GpuImagePipeline(scale_factor=None, device=device, keys=('img', 'gt_bboxes'), **kw), **w)


# ---------------------------------------------------------------------------------------------------------------- tests
def test_fixed_point_resize_is_identity_at_identity_sizes():
    rng = np.random.RandomState(0)
    for h, w in ((1, 1), (7, 5), (64, 33), (128, 128)):
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        assert np.array_equal(resize_linear_u8(img, w, h), img)
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)      # every value
    assert np.array_equal(resize_linear_u8(img, 16, 16), img)
    # one identity axis: a row-constant image stays row-constant with its values, whatever the other axis does
    img = np.repeat(rng.randint(0, 256, (1, 12, 3)).astype(np.uint8), 9, axis=0)
    assert np.array_equal(resize_linear_u8(img, 12, 23), np.repeat(img[:1], 23, axis=0))
    # an exact 2:1 reduction is the (a + b + c + d + 2) >> 2 of OpenCV's own shortcut to INTER_AREA
    img = rng.randint(0, 256, (10, 14, 3)).astype(np.int64)
    want = (img[0::2, 0::2] + img[1::2, 0::2] + img[0::2, 1::2] + img[1::2, 1::2] + 2) >> 2
    assert np.array_equal(resize_linear_u8(img.astype(np.uint8), 7, 5), want.astype(np.uint8))


def _jobs_of(case):
    """Every (crop, dw, dh) the case resizes."""
    if 'augs' in case:
        return [(tuple(a['crop']), a['img_shape'][1], a['img_shape'][0]) for a in case['augs']]
    h, w = case['hw']
    return [((0, 0, w, h), d['img_shape'][1], d['img_shape'][0]) for d in case['draws']]


def test_fixed_point_resize_stays_within_its_rounding_budget_of_fp64_bilinear():
    """|u8 - exact| < 1.0 on every pixel of every golden case.  Derived, not measured: the two 11-bit coefficient roundings
    contribute <= 0.5 / 2048 * 255 * 2 = 0.125 per pass, the >> 4 / >> 16 truncations < 0.1 together, the final rounding 0.5."""
    worst = 0.0
    seen = set()
    for name, case in load_golden()['cases'].items():
        img = case_image(case)
        for crop, dw, dh in _jobs_of(case):
            if (name, crop, dw, dh) in seen:
                continue
            seen.add((name, crop, dw, dh))
            x0, y0, cw, ch = crop
            src = img[y0:y0 + ch, x0:x0 + cw]
            err = np.abs(resize_linear_u8(src, dw, dh).astype(np.float64) - bilinear_fp64(src, dw, dh)).max()
            print('%-28s %4dx%-4d -> %4dx%-4d  max|u8 - exact| = %.4f' % (name, ch, cw, dh, dw, err))
            worst = max(worst, float(err))
            assert err < 1.0, (name, crop, dw, dh, err)
    assert len(seen) >= 11, len(seen)
    print('worst over %d resizes: %.4f' % (len(seen), worst))


@pytest.mark.parametrize('name', sorted(load_golden()['cases']) if os.path.exists(GOLDEN) else [])
def test_host_restatement_reproduces_the_reference_classes(name):
    """Sizes, scale_factor bits, random draws (Resize's before RandomFlip's, per sample) and the augmentation order of the wrappers,
    as the reference's own Resize / RandomFlip / MultiScaleFlipAug / CroppedTilesFlipAug produced them."""
    case = load_golden()['cases'][name]
    pipe = build_pipeline(case)
    h, w = case['hw']
    if 'augs' in case:
        augs = pipe.augmentations(h, w)
        assert len(augs) == len(case['augs'])
        for (crop, sc, flip, direction, off), ref in zip(augs, case['augs']):
            plan = pipe.pipeline._plan(0, crop, flip=flip, **{pipe.scale_key: sc})
            assert list(crop) == ref['crop'] and flip == ref['flip'] and direction == ref['flip_direction']
            assert (None if off is None else list(off)) == ref['tile_offset']
            assert [plan['dh'], plan['dw'], 3] == ref['img_shape']
            assert plan['scale_factor'].view(np.uint32).tolist() == ref['scale_factor_bits']
            assert list(plan['scale']) == ref['scale']
            d = pipe.pipeline.size_divisor
            assert [(plan['dh'] + d - 1) // d * d, (plan['dw'] + d - 1) // d * d, 3] == ref['pad_shape']
        return
    rng = np.random.RandomState(case['seed'])
    for ref in case['draws']:
        scale = pipe._random_scale(rng) if pipe.img_scale is not None else None
        flip = pipe.flip_ratio > 0 and rng.rand() < pipe.flip_ratio
        plan = pipe._plan(0, (0, 0, w, h), scale, pipe.scale_factor, flip)
        assert list(plan['scale']) == ref['scale'] and bool(flip) == ref['flip']
        assert [plan['dh'], plan['dw'], 3] == ref['img_shape']
        assert plan['scale_factor'].view(np.uint32).tolist() == ref['scale_factor_bits']


def test_bad_options_are_named():
    from pointtinybenchmark_amd.datasets import GpuImagePipeline, GpuTestTimeAug
    with pytest.raises(ValueError, match='backend'):
        GpuImagePipeline(img_scale=(667, 400), backend='pillow', device='cpu')
    with pytest.raises(ValueError, match='direction'):
        GpuImagePipeline(img_scale=(667, 400), flip_direction='vertical', device='cpu')
    inner = GpuImagePipeline(scale_factor=None, device='cpu')
    with pytest.raises(ValueError, match='flip_direction'):
        GpuTestTimeAug(inner, img_scale=(667, 400), flip=True, flip_direction=['horizontal', 'diagonal'])
    with pytest.raises(ValueError, match='RandomCrop'):
        GpuImagePipeline.from_config([dict(type='LoadImageFromFile'), dict(type='RandomCrop', crop_size=(5, 5))], device='cpu')
    with pytest.raises(ValueError, match='pad_val'):
        GpuImagePipeline.from_config([dict(type='Resize', img_scale=(667, 400)), dict(type='Pad', size_divisor=32, pad_val=3)],
                                     device='cpu')
    with pytest.raises(ValueError, match='with_mask'):
        GpuImagePipeline.from_config([dict(type='LoadAnnotations', with_bbox=True, with_mask=True),
                                      dict(type='Resize', img_scale=(667, 400))], device='cpu')
    with pytest.raises(ValueError, match='GpuTestTimeAug'):
        inner([dict(img=np.zeros((4, 4, 3), np.uint8))])          # a bare Resize has no scale of its own


def test_single_scale_pipeline_draws_nothing_for_resize():
    """Existing callers hand in an rng that only has .rand(): a single-scale Resize must not ask it for anything else."""
    from pointtinybenchmark_amd.datasets import GpuImagePipeline

    class OnlyRand:
        def rand(self):
            return 0.25
    pipe = GpuImagePipeline(img_scale=(667, 400), flip_ratio=0.5, device='cpu')
    assert pipe._random_scale(OnlyRand()) == (667, 400)


def _reference_configs():
    from oracle.gen_golden_configs import CONFIGS
    return [c for c in CONFIGS if '_base_/models' not in c]


@pytest.mark.parametrize('rel', _reference_configs())
def test_from_config_builds_the_shipped_pipelines(rel):
    """train_pipeline and test_pipeline of every shipped coarsepointv2 / p2p config whose model builds, as the files stand."""
    from oracle import ref_loader
    if not ref_loader.available():
        pytest.skip('needs the reference tree')
    from pointtinybenchmark_amd.config import Config
    from pointtinybenchmark_amd.datasets import GpuImagePipeline, GpuTestTimeAug
    cfg = Config.fromfile(os.path.join(ref_loader.REF_ROOT, rel))
    train = GpuImagePipeline.from_config(cfg.data.train.pipeline, device='cpu')
    assert isinstance(train, GpuImagePipeline) and 'gt_bboxes' in train.keys and train.flip_ratio == 0.5
    want = {'COCO/p2p/p2p_r50_fpns4_1x_fl_sl1_coco.py': [(1333, 800)], 'DOTA/p2p': [(1024, 1024)], 'COCO': [(667, 400)]}
    scale = next((v for k, v in want.items() if k in rel), None)
    if 'DOTA/coarsepointv2' in rel or 'TinyPersonV2' in rel:
        scale = None
    assert train.img_scale == scale and train.resizes == (scale is not None)
    test = GpuImagePipeline.from_config(cfg.data.test.pipeline, device='cpu')
    assert isinstance(test, GpuTestTimeAug) and not test.flip
    tiled = 'DOTA/p2p' in rel or 'TinyPersonV2/p2p' in rel
    assert (test.tile_shape is not None) == tiled, (rel, test.tile_shape)
    assert test.scales == (scale if scale is not None and not tiled else [1.0])
    assert len(test.augmentations(2000, 3000)) == (1 if not tiled else 12 if 'DOTA' in rel else 24)
