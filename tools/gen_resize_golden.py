"""Sizes, draws, boxes and augmentation order of the reference's Resize / RandomFlip / Pad / MultiScaleFlipAug / CroppedTilesFlipAug
(needs the reference tree; the .json travels):
  python tools/gen_resize_golden.py
  tests/golden/resize_pipeline.json
The reference's own classes are cut out of its pipeline files and executed (the modules import mmcv, which is not installed) with a
stand-in ``mmcv`` whose imrescale / imresize are mmcv's size arithmetic around the numpy restatement of cv2.resize
(tests/test_resize_host.py: resize_linear_u8), under fixed numpy seeds.  Pixels are not recorded -- the GPU tests rebuild them from
the same restatement -- only what the host side must reproduce exactly:
  per case      hw, seed (image: case_image), resize / wrapper arguments, flip_ratio, boxes_bits (input gt_bboxes, float32 bits)
  draws[]       train-style cases, N_DRAWS samples from ONE random stream: scale, flip, img_shape, pad_shape, scale_factor_bits,
                boxes_bits (after Resize._resize_bboxes and RandomFlip.bbox_flip)
  augs[]        wrapper cases, in the wrapper's order: crop (x0, y0, cw, ch = what Resize was handed), tile_offset, scale, flip,
                flip_direction, img_shape, pad_shape, scale_factor_bits, boxes_bits"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import data_oracle as DO  # noqa: E402
from tests.test_resize_host import GOLDEN, case_image, resize_linear_u8  # noqa: E402

N_DRAWS = 6
INNER = [dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Pad', size_divisor=32), dict(type='Collect', keys=['img'])]
CASES = {
    'coco_480x640_at_667x400': dict(hw=(480, 640), seed=1, resize=dict(img_scale=(667, 400), keep_ratio=True)),
    'coco_427x640_at_667x400': dict(hw=(427, 640), seed=2, resize=dict(img_scale=(667, 400), keep_ratio=True)),
    'coco_500x375_at_1333x800': dict(hw=(500, 375), seed=3, resize=dict(img_scale=(1333, 800), keep_ratio=True)),
    'range_1333x640_to_800': dict(hw=(240, 320), seed=4, resize=dict(img_scale=[(1333, 640), (1333, 800)], multiscale_mode='range',
                                                                      keep_ratio=True)),
    'value_two_scales': dict(hw=(427, 640), seed=5, resize=dict(img_scale=[(1333, 800), (667, 400)], multiscale_mode='value',
                                                                 keep_ratio=True)),
    'ratio_range': dict(hw=(480, 640), seed=6, resize=dict(img_scale=(667, 400), ratio_range=(0.8, 1.2), keep_ratio=True)),
    'keep_ratio_false': dict(hw=(427, 640), seed=7, resize=dict(img_scale=(512, 384), keep_ratio=False)),
    'scale_factor_half': dict(hw=(427, 641), seed=8, resize=dict(scale_factor=[0.5], keep_ratio=True)),
    'overhanging_boxes': dict(hw=(375, 500), seed=9, n_boxes=40, resize=dict(img_scale=(667, 400), keep_ratio=True)),
    'tiles_300x200_flip': dict(hw=(300, 200), seed=10, resize=dict(keep_ratio=True),
                               wrapper=dict(tile_shape=(128, 128), tile_overlap=(32, 32), scale_factor=[1.0], flip=True)),
    'tiles_image_smaller_than_tile': dict(hw=(100, 90), seed=11, resize=dict(keep_ratio=True),
                                          wrapper=dict(tile_shape=(128, 128), tile_overlap=(32, 32), scale_factor=[1.0, 1.5], flip=True)),
    'multiscale_flip': dict(hw=(213, 320), seed=12, resize=dict(keep_ratio=True),
                            wrapper=dict(img_scale=[(667, 400), (1333, 800)], flip=True)),
}


def case_boxes(case):
    """16 x 16 pseudo boxes around points up to 12 px outside the image: some overhang every border."""
    h, w = case['hw']
    c = np.random.RandomState(case['seed'] + 2000).uniform(-12, 12 + np.array([w, h]), (case.get('n_boxes', 12), 2))
    return np.concatenate([c - 8, c + 8], axis=1).astype(np.float32)


class _Mmcv:
    """mmcv's image functions as far as the pipeline classes call them (mmcv/image/geometric.py restated around the numpy resize)."""
    log = []

    @staticmethod
    def is_list_of(seq, typ):
        return isinstance(seq, list) and all(isinstance(v, typ) for v in seq)

    @staticmethod
    def imresize(img, size, return_scale=False, interpolation='bilinear', out=None, backend=None):
        assert backend in (None, 'cv2') and interpolation == 'bilinear'
        h, w = img.shape[:2]
        _Mmcv.log.append((h, w))
        resized = resize_linear_u8(img, size[0], size[1])
        return (resized, size[0] / w, size[1] / h) if return_scale else resized

    @staticmethod
    def imrescale(img, scale, return_scale=False, interpolation='bilinear', backend=None):
        h, w = img.shape[:2]
        assert isinstance(scale, tuple)
        sf = min(max(scale) / max(h, w), min(scale) / min(h, w))
        new_size = (int(w * float(sf) + 0.5), int(h * float(sf) + 0.5))
        resized = _Mmcv.imresize(img, new_size, interpolation=interpolation, backend=backend)
        return (resized, sf) if return_scale else resized

    @staticmethod
    def imflip(img, direction='horizontal'):
        assert direction == 'horizontal'
        return np.flip(img, axis=1)

    @staticmethod
    def impad_to_multiple(img, divisor, pad_val=0):
        h, w = img.shape[:2]
        out = np.full(((h + divisor - 1) // divisor * divisor, (w + divisor - 1) // divisor * divisor, img.shape[2]), pad_val, img.dtype)
        out[:h, :w] = img
        return out


def _class(path, name):
    src = open(path).read()
    start = src.index('class %s' % name)
    end = src.find('\n@PIPELINES', start)
    return src[start:end if end > 0 else len(src)]


def reference_classes():
    import warnings
    P = DO.T + 'datasets/pipelines/'
    ns = dict(np=np, mmcv=_Mmcv, warnings=warnings)
    for name in ('Resize', 'RandomFlip', 'Pad'):
        exec(_class(P + 'transforms.py', name), ns)

    class Compose:
        def __init__(self, transforms):
            self.ts = [ns[t['type']](**{k: v for k, v in t.items() if k != 'type'}) for t in transforms
                       if t['type'] in ('Resize', 'RandomFlip', 'Pad')]

        def __call__(self, results):
            for t in self.ts:
                results = t(results)
            return results
    ns['Compose'] = Compose
    exec(_class(P + 'test_time_aug.py', 'MultiScaleFlipAug'), ns)
    exec(_class(P + 'rtest_time_aug.py', 'CroppedTilesFlipAug'), ns)
    return ns


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()


def record(res):
    return dict(scale=[(float(v) if isinstance(v, float) else int(v)) for v in res['scale']], flip=bool(res['flip']),
                flip_direction=res['flip_direction'], img_shape=[int(v) for v in res['img_shape']],
                pad_shape=[int(v) for v in res['pad_shape']], scale_factor_bits=bits(res['scale_factor']),
                boxes_bits=bits(res['gt_bboxes']))


def run_case(ns, case):
    img, boxes = case_image(case), case_boxes(case)
    out = dict(hw=list(case['hw']), seed=case['seed'], resize=case['resize'], boxes_bits=bits(boxes))
    base = dict(img=img, img_shape=img.shape, ori_shape=img.shape, img_fields=['img'], bbox_fields=['gt_bboxes'], gt_bboxes=boxes)
    if 'wrapper' in case:
        out['wrapper'] = case['wrapper']
        cls = ns['CroppedTilesFlipAug' if 'tile_shape' in case['wrapper'] else 'MultiScaleFlipAug']
        aug = cls(transforms=[dict(t) for t in INNER], **case['wrapper'])
        _Mmcv.log = []
        res = aug(dict(base))
        n = len(res['img'])
        assert len(_Mmcv.log) == n
        out['augs'] = []
        for k in range(n):
            r = record({key: res[key][k] for key in res})
            off = res['tile_offset'][k] if 'tile_offset' in res else None
            h_in, w_in = _Mmcv.log[k]
            r.update(tile_offset=None if off is None else [int(v) for v in off],
                     crop=[int(off[0]) if off else 0, int(off[1]) if off else 0, w_in, h_in])
            out['augs'].append(r)
        return out
    out['flip_ratio'] = 0.5
    resize, flip, pad = ns['Resize'](**case['resize']), ns['RandomFlip'](flip_ratio=0.5), ns['Pad'](size_divisor=32)
    np.random.seed(case['seed'])
    out['draws'] = [record(pad(flip(resize(dict(base))))) for _ in range(N_DRAWS)]
    return out


def main():
    assert os.path.isdir(DO.T), 'needs the reference tree'
    ns = reference_classes()
    out = dict(n_draws=N_DRAWS, cases={name: run_case(ns, case) for name, case in CASES.items()})
    with open(GOLDEN, 'w') as f:
        json.dump(out, f, sort_keys=True)
    print(GOLDEN, os.path.getsize(GOLDEN), 'bytes')
    for name, c in out['cases'].items():
        print('%-32s' % name, [(d['scale'], d['flip'], d['img_shape']) for d in c.get('draws', c.get('augs'))][:4])


if __name__ == '__main__':
    main()
