"""Device side of the train / test image pipelines of the CPR / P2P configs (configs2/*/coarsepointv2, configs2/*/p2p):

    Resize(img_scale | scale_factor, multiscale_mode, ratio_range, keep_ratio)
                                                sizes / draws on the host (transforms.py:66-321, mmcv.rescale_size restated); pixels:
                                                cv2's 8-bit fixed-point bilinear on the device; boxes: scaled, clipped to the resized
                                                image (bbox_clip_border=True, transforms.py:241-249) -- same kernel as the flip
    RandomFlip(flip_ratio)                      decision on the host, pixels + boxes flipped on the device
    Normalize(mean, std, to_rgb) -> Pad(size_divisor) -> DefaultFormatBundle -> collate
                                                fused with the resize: uint8 HWC -> (N,Hp,Wp,4) fp32 channels-last
    Collect(keys=...)                           same keys / img_metas entries as the reference hands to forward_train
    MultiScaleFlipAug / CroppedTilesFlipAug     GpuTestTimeAug: every tile x scale x flip of one image from ONE upload, ONE launch

One launch (cpr_preprocess_jobs_u8) covers a whole batch, ragged or resized.  A batch of equally sized images at scale 1 -- the
TinyPersonV2 / DOTA-CPR configs, ``Resize(scale_factor=[1.0])`` -- keeps the stacked kernel it always used (cpr_preprocess_u8).

The result's ``img`` is an NCHW-shaped channels-last view with 4 channels (4th = 0): ResNet.forward consumes it without a
layout pass.  Images of different (resized) sizes are batched by padding to the largest (mmcv collate pads to the batch
maximum as well)."""
import numpy as np
import torch

from .. import _lib, ops


def pil_bgr_loader(path):
    """uint8 HxWx3 BGR like mmcv.imread(cv2 backend) hands to the pipeline (PIL decodes RGB)."""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert('RGB'))[:, :, ::-1])


def rescale_size(w, h, scale):
    """mmcv.rescale_size((w, h), scale) for a tuple ``scale`` = (max long edge, max short edge), with mmcv's _scale_size rounding."""
    sf = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return int(w * float(sf) + 0.5), int(h * float(sf) + 0.5)


def _scale_list(img_scale):
    """``img_scale`` of Resize / MultiScaleFlipAug: one (long, short) pair or a list of pairs -> list of tuples."""
    if isinstance(img_scale, (list, tuple)) and len(img_scale) and isinstance(img_scale[0], (list, tuple)):
        return [tuple(v) for v in img_scale]
    return [tuple(img_scale)]


def _pad_to(v, d):
    return (v + d - 1) // d * d


class GpuImagePipeline:
    def __init__(self, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), to_rgb=True, size_divisor=32,
                 flip_ratio=0.0, scale_factor=1.0, device='cuda',
                 keys=('img', 'gt_bboxes', 'gt_labels', 'gt_bboxes_ignore', 'gt_true_bboxes'), bbox_clip_border=True,
                 img_scale=None, multiscale_mode='range', ratio_range=None, keep_ratio=True, backend='cv2',
                 flip_direction='horizontal', meta_keys=None):
        """The Resize arguments are those of transforms.py:66-103.  ``scale_factor=None`` together with ``img_scale=None`` is the
        bare ``Resize(keep_ratio=True)`` inside a test-time wrapper: the scale then comes from GpuTestTimeAug."""
        if backend != 'cv2':
            raise ValueError("Resize backend=%r is not built (only 'cv2': the kernel restates OpenCV's fixed-point bilinear)" % (backend,))
        if flip_direction != 'horizontal':
            raise ValueError("RandomFlip direction=%r is not built (only 'horizontal')" % (flip_direction,))
        if isinstance(scale_factor, (list, tuple)):
            if len(scale_factor) != 1:
                # transforms.py:295 would call random_select(self.img_scale) with img_scale None: the reference cannot run it either
                raise ValueError('Resize scale_factor=%r: a list of more than one factor is not built' % (scale_factor,))
            scale_factor = scale_factor[0]
        if img_scale is not None:
            if scale_factor is not None and float(scale_factor) != 1.0:
                raise ValueError('img_scale and scale_factor cannot be both set')
            scale_factor = None
            img_scale = _scale_list(img_scale)
            if ratio_range is not None:
                assert len(img_scale) == 1
            elif multiscale_mode not in ('value', 'range'):
                raise ValueError('Resize multiscale_mode=%r is not built' % (multiscale_mode,))
            elif multiscale_mode == 'range' and len(img_scale) > 1:
                assert len(img_scale) == 2
        self.img_scale, self.multiscale_mode, self.ratio_range = img_scale, multiscale_mode, ratio_range
        self.keep_ratio = bool(keep_ratio)
        self.scale_factor = None if scale_factor is None else float(scale_factor)
        self.mean = np.array(mean, dtype=np.float32)
        self.std = np.array(std, dtype=np.float32)
        # mmcv.imnormalize_: stdinv = 1 / np.float64(std), applied to a float32 image (cv2 converts the scalar to float)
        self.stdinv = (1.0 / np.float64(self.std)).astype(np.float32)
        self.to_rgb, self.size_divisor, self.flip_ratio = bool(to_rgb), int(size_divisor), float(flip_ratio)
        self.device, self.keys = device, tuple(keys)
        self.meta_keys = None if meta_keys is None else tuple(meta_keys)
        self.bbox_clip_border = bool(bbox_clip_border)       # Resize's default (transforms.py:66)

    @property
    def resizes(self):
        """False for the scale-1 configs: Resize is the identity there and the stacked kernel serves a uniform batch."""
        return not (self.img_scale is None and self.scale_factor == 1.0)

    # ---- Resize on the host: which size, which scale_factor (transforms.py:105-239) ----
    def _random_scale(self, rng):
        """Resize._random_scale with the draws of random_sample_ratio / random_sample / random_select; a single scale draws nothing."""
        if self.ratio_range is not None:
            lo, hi = self.ratio_range
            assert lo <= hi
            ratio = rng.random_sample() * (hi - lo) + lo
            return int(self.img_scale[0][0] * ratio), int(self.img_scale[0][1] * ratio)
        if len(self.img_scale) == 1:
            return self.img_scale[0]
        if self.multiscale_mode == 'range':
            longs, shorts = [max(s) for s in self.img_scale], [min(s) for s in self.img_scale]
            long_edge = rng.randint(min(longs), max(longs) + 1)
            return long_edge, rng.randint(min(shorts), max(shorts) + 1)
        return self.img_scale[rng.randint(len(self.img_scale))]

    def _plan(self, src, crop, scale=None, scale_factor=None, flip=False, **extra):
        """One output image: source sample ``src``, crop (x0, y0, cw, ch), and what Resize.__call__ -> _resize_img make of it."""
        w, h = crop[2], crop[3]
        if scale is None:
            assert isinstance(scale_factor, float), 'scale_factor must be a float (transforms.py:302)'
            scale = (int(w * scale_factor), int(h * scale_factor))
        dw, dh = rescale_size(w, h, scale) if self.keep_ratio else (int(scale[0]), int(scale[1]))
        w_scale, h_scale = dw / w, dh / h
        return dict(src=src, crop=tuple(int(v) for v in crop), dw=dw, dh=dh, flip=bool(flip), scale=tuple(scale),
                    scale_factor=np.array([w_scale, h_scale, w_scale, h_scale], dtype=np.float32), **extra)

    def __call__(self, samples, rng=None):
        """samples: list of dicts with ``img`` (uint8 HxWx3 BGR, numpy or torch) and the gt_* numpy fields.  Random draws are taken
        per sample, Resize's before RandomFlip's, as a per-sample pipeline takes them from one stream."""
        if self.img_scale is None and self.scale_factor is None:
            raise ValueError('this pipeline has a bare Resize: its scale comes from GpuTestTimeAug')
        rng = rng or np.random
        plans = []
        for i, s in enumerate(samples):
            h, w = s['img'].shape[:2]
            scale = self._random_scale(rng) if self.img_scale is not None else None
            flip = self.flip_ratio > 0 and rng.rand() < self.flip_ratio
            plans.append(self._plan(i, (0, 0, w, h), scale, self.scale_factor, flip, flip_direction='horizontal' if flip else None))
        shapes = [tuple(s['img'].shape) for s in samples]
        if not self.resizes and all(s == shapes[0] for s in shapes):
            return self._stacked(samples, plans)
        return self._run(samples, plans)

    # ---- scale 1, one shape: the stacked kernels ----
    def _stacked(self, samples, plans):
        n = len(samples)
        flips = np.array([int(p['flip']) for p in plans], dtype=np.int32)
        H, W = samples[0]['img'].shape[:2]
        d = self.size_divisor
        Hp, Wp = _pad_to(H, d), _pad_to(W, d)
        dev = self.device
        out = torch.empty((n, Hp, Wp, 4), device=dev, dtype=torch.float32)
        stack = torch.from_numpy(np.stack([np.asarray(s['img']) for s in samples])).to(dev)
        self._launch(stack, torch.from_numpy(flips).to(dev), out, n, H, W, Hp, Wp)
        batch = dict(img=ops.as_nchw(out), img_metas=[self._meta(samples[p['src']], p) for p in plans])
        img_hw = torch.tensor([[H, W]] * n, dtype=torch.int32, device=dev).reshape(-1)
        self._annotations(batch, samples, plans, torch.from_numpy(flips).to(dev), img_hw, None)
        return batch

    def _launch(self, img_u8, flips, out, n, H, W, Hp, Wp):
        assert img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.shape[-1] == 3
        import ctypes
        m = (ctypes.c_float * 3)(*self.mean.tolist())
        s = (ctypes.c_float * 3)(*self.stdinv.tolist())
        _lib.call('cpr_preprocess_u8', ops._ptr(img_u8), ops._ptr(flips), ctypes.cast(m, ctypes.c_void_p),
                  ctypes.cast(s, ctypes.c_void_p), int(self.to_rgb), ops._ptr(out), n, H, W, Hp, Wp, ops._stream())

    # ---- everything else: one job per output image, one launch ----
    def _sources(self, samples, used):
        """Device address, row pitch and size of every sample in ``used``: host images travel in ONE copy."""
        src, host, keep = {}, [], []
        for i in used:
            im = samples[i]['img']
            if torch.is_tensor(im) and im.is_cuda:
                assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.stride(2) == 1 and im.stride(1) == 3
                src[i] = (im.data_ptr(), im.stride(0), im.shape[1], im.shape[0])
                keep.append(im)
            else:
                a = np.ascontiguousarray(np.asarray(im))
                assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3, (a.dtype, a.shape)
                host.append((i, a))
        if host:
            flat = torch.from_numpy(np.concatenate([a.reshape(-1) for _, a in host])).to(self.device)
            keep.append(flat)
            off = 0
            for i, a in host:
                src[i] = (flat.data_ptr() + off, a.shape[1] * 3, a.shape[1], a.shape[0])
                off += a.size
        return src, keep

    def _run(self, samples, plans, batched=True):
        n, d, dev = len(plans), self.size_divisor, self.device
        pads = [(_pad_to(p['dh'], d), _pad_to(p['dw'], d)) for p in plans]
        if batched:                                    # collate: every slot padded to the batch maximum
            slots = [(max(h for h, _ in pads), max(w for _, w in pads))] * n
        else:                                          # test-time augmentations: one image each, each its own size
            slots = pads
        offs = np.concatenate([[0], np.cumsum([h * w for h, w in slots])]).astype(np.int64)
        out = torch.empty((int(offs[-1]) * 4,), device=dev, dtype=torch.float32)
        src, keep = self._sources(samples, sorted({p['src'] for p in plans}))
        jobs = np.zeros((n,), dtype=np.dtype(ops.PREPROCESS_JOB))
        for k, (p, (Hp, Wp)) in enumerate(zip(plans, slots)):
            ptr, pitch, sw, sh = src[p['src']]
            jobs[k] = (ptr, offs[k], 0.0, 0.0, pitch, sw, sh) + p['crop'] + (p['dw'], p['dh'], int(p['flip']), Hp, Wp)
        ops.preprocess_jobs(jobs, self.mean, self.stdinv, self.to_rgb, out)
        del keep                                       # stream-ordered: the launch above is queued in front of any reuse
        flips_d = torch.tensor([int(p['flip']) for p in plans], dtype=torch.int32, device=dev)
        img_hw = torch.tensor([[p['dh'], p['dw']] for p in plans], dtype=torch.int32, device=dev).reshape(-1)
        scale4 = torch.from_numpy(np.stack([p['scale_factor'] for p in plans])).to(dev)
        metas = [self._meta(samples[p['src']], p) for p in plans]
        if batched:
            batch = dict(img=ops.as_nchw(out.view(n, slots[0][0], slots[0][1], 4)), img_metas=metas)
            self._annotations(batch, samples, plans, flips_d, img_hw, scale4)
            return batch
        imgs = [ops.as_nchw(out[int(offs[k]) * 4:int(offs[k + 1]) * 4].view(1, Hp, Wp, 4)) for k, (Hp, Wp) in enumerate(slots)]
        batch = dict(img=imgs, img_metas=[[m] for m in metas])
        flat = {}
        self._annotations(flat, samples, plans, flips_d, img_hw, scale4)
        batch.update({k: [[t] for t in v] for k, v in flat.items()})   # per augmentation: a batch of one image
        return batch

    def _meta(self, s, p):
        d = self.size_divisor
        h, w = p['dh'], p['dw']
        m = dict(filename=s.get('filename'), ori_filename=s.get('ori_filename'),
                 ori_shape=s.get('ori_shape', tuple(s['img'].shape)), img_shape=(h, w, 3),
                 pad_shape=(_pad_to(h, d), _pad_to(w, d), 3), scale_factor=p['scale_factor'], flip=p['flip'],
                 flip_direction=p.get('flip_direction'), img_norm_cfg=dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb))
        if 'tile_offset' in p:
            m['tile_offset'] = p['tile_offset']
        for k in self.meta_keys or ():
            if k not in m:
                m[k] = s.get(k)
        return m

    def _annotations(self, batch, samples, plans, flips_d, img_hw, scale4):
        per = [samples[p['src']] for p in plans]
        for key in ('gt_bboxes', 'gt_bboxes_ignore', 'gt_true_bboxes'):   # = the pipeline's bbox_fields (loading.py:246-278)
            if key in self.keys and all(key in s for s in per):
                batch[key] = self._boxes([s[key] for s in per], flips_d, img_hw, scale4)
        for key in ('gt_labels', 'gt_anns_id'):
            if key in self.keys and all(key in s for s in per):
                counts = [len(s[key]) for s in per]              # one host->device copy, per-image views (cat_rows re-joins them)
                flat = np.concatenate([np.asarray(s[key], dtype=np.int64).reshape(-1) for s in per]) if sum(counts) else \
                    np.zeros((0,), np.int64)
                batch[key] = list(torch.split(torch.from_numpy(flat).to(self.device), counts))

    def _boxes(self, per_img, flips_d, img_hw, scale4=None):
        counts = [len(b) for b in per_img]
        flat = np.concatenate([np.asarray(b, dtype=np.float32).reshape(-1, 4) for b in per_img]) if sum(counts) else \
            np.zeros((0, 4), np.float32)
        t = torch.from_numpy(np.ascontiguousarray(flat)).to(self.device)
        if len(flat):
            img_of = torch.from_numpy(np.repeat(np.arange(len(counts), dtype=np.int32), counts)).to(self.device)
            if scale4 is None:
                _lib.call('cpr_clip_flip_boxes', ops._ptr(t), ops._ptr(img_of), ops._ptr(flips_d), ops._ptr(img_hw), len(flat),
                          int(self.bbox_clip_border), ops._stream())
            else:
                ops.scale_clip_flip_boxes(t, img_of, flips_d, img_hw, scale4, self.bbox_clip_border)
        return list(torch.split(t, counts))

    # ---- a reference pipeline list as it stands ----
    @classmethod
    def from_config(cls, pipeline_cfg, device='cuda'):
        """``train_pipeline`` / ``test_pipeline`` of a reference config -> GpuImagePipeline, or the GpuTestTimeAug around it.
        LoadImageFromFile / LoadAnnotations stay with the caller (CocoFmtDataset.load_sample); a transform or an option that is not
        built raises ValueError naming it."""
        kw = dict(device=device, scale_factor=None, keys=('img',))
        order = []
        for pos, t in enumerate(pipeline_cfg):
            t = dict(t)
            typ = t.pop('type')
            order.append(typ)
            if typ in ('MultiScaleFlipAug', 'CroppedTilesFlipAug'):
                if pos != len(pipeline_cfg) - 1 or any(o in _GEOMETRY for o in order):
                    raise ValueError('from_config: %s must come last and hold every image transform' % typ)
                pipe = cls.from_config(t.pop('transforms'), device)
                if isinstance(pipe, GpuTestTimeAug) or pipe.img_scale is not None or pipe.scale_factor is not None:
                    raise ValueError('from_config: the Resize inside %s must leave the scale to the wrapper' % typ)
                if typ == 'CroppedTilesFlipAug':
                    t['img_scale'] = t.pop('tile_scale', None)
                return GpuTestTimeAug(pipe, **t)
            opts = _UNDERSTOOD.get(typ)
            if opts is None:
                raise ValueError('from_config: transform %r is not built' % typ)
            for k, v in t.items():
                if k not in opts:
                    raise ValueError('from_config: %s option %r is not built' % (typ, k))
            if typ == 'LoadAnnotations':
                for k in ('with_mask', 'with_seg'):
                    if t.get(k):
                        raise ValueError('from_config: LoadAnnotations option %r is not built' % k)
            elif typ == 'Resize':
                if t.get('override'):
                    raise ValueError("from_config: Resize option 'override' is not built")
                t.pop('override', None)
                kw.update(t)
            elif typ == 'RandomFlip':
                ratio = t.get('flip_ratio')
                if isinstance(ratio, (list, tuple)) or isinstance(t.get('direction', 'horizontal'), (list, tuple)):
                    raise ValueError("from_config: RandomFlip with lists of ratios / directions is not built")
                kw.update(flip_ratio=0.0 if ratio is None else float(ratio), flip_direction=t.get('direction', 'horizontal'))
            elif typ == 'Normalize':
                kw.update(mean=t['mean'], std=t['std'], to_rgb=t.get('to_rgb', True))
            elif typ == 'Pad':
                if t.get('size') is not None or t.get('pad_val', 0) != 0 or not t.get('size_divisor'):
                    raise ValueError("from_config: Pad is built for size_divisor with pad_val=0 (got %r)" % (t,))
                kw.update(size_divisor=t['size_divisor'])
            elif typ == 'ImageToTensor':
                if list(t.get('keys', ['img'])) != ['img']:
                    raise ValueError("from_config: ImageToTensor option 'keys' other than ['img'] is not built")
            elif typ == 'Collect':
                kw.update(keys=tuple(t['keys']))
                if 'meta_keys' in t:
                    kw.update(meta_keys=tuple(t['meta_keys']))
        geo = [o for o in order if o in _GEOMETRY]
        if geo != [o for o in _GEOMETRY if o in geo] or 'Resize' not in geo:
            raise ValueError('from_config: expected Resize -> RandomFlip -> Normalize -> Pad, got %r' % (geo,))
        if 'Normalize' not in geo:
            kw.update(mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), to_rgb=False)     # (x - 0) * 1: the uint8 values as floats
        if 'Pad' not in geo:
            kw.update(size_divisor=1)
        return cls(**kw)


_GEOMETRY = ('Resize', 'RandomFlip', 'Normalize', 'Pad')
_UNDERSTOOD = {
    'LoadImageFromFile': (),
    'LoadAnnotations': ('with_bbox', 'with_label', 'with_mask', 'with_seg'),
    'Resize': ('img_scale', 'multiscale_mode', 'ratio_range', 'keep_ratio', 'bbox_clip_border', 'backend', 'override', 'scale_factor'),
    'RandomFlip': ('flip_ratio', 'direction'),
    'Normalize': ('mean', 'std', 'to_rgb'),
    'Pad': ('size', 'size_divisor', 'pad_val'),
    'DefaultFormatBundle': (),
    'ImageToTensor': ('keys',),
    'Collect': ('keys', 'meta_keys'),
}


class GpuTestTimeAug:
    """MultiScaleFlipAug (test_time_aug.py) and, with ``tile_shape``, the fork's CroppedTilesFlipAug (rtest_time_aug.py:37-67) around
    a GpuImagePipeline whose Resize leaves the scale open.  One sample per call, as the reference's test loaders hand them over; the
    image is uploaded once, tiles are crop rectangles of that upload, and every tile x scale x flip is a job of ONE launch.
    Returns ``img`` / ``img_metas`` (and the collected gt_* keys) as lists over augmentations: BasicLocator.forward_test's format.
    ``flip`` / ``flip_direction`` are handed to the inner transforms, not drawn; the annotation fields see the inner Resize and
    RandomFlip only (the wrappers do not move boxes into a tile)."""

    def __init__(self, pipeline, img_scale=None, scale_factor=None, flip=False, flip_direction='horizontal', tile_shape=None,
                 tile_overlap=None):
        if (img_scale is None) == (scale_factor is None):
            raise ValueError('exactly one of img_scale and scale_factor must be set')
        if img_scale is not None:
            self.scales = _scale_list(img_scale)
            self.scale_key = 'scale'
        else:
            self.scales = list(scale_factor) if isinstance(scale_factor, (list, tuple)) else [scale_factor]
            self.scale_key = 'scale_factor'
        self.flip = bool(flip)
        self.flip_direction = list(flip_direction) if isinstance(flip_direction, (list, tuple)) else [flip_direction]
        for d in self.flip_direction:
            if d != 'horizontal':
                raise ValueError("flip_direction=%r is not built (only 'horizontal')" % (d,))
        if (tile_shape is None) != (tile_overlap is None):
            raise ValueError('tile_shape and tile_overlap go together')
        self.tile_shape = None if tile_shape is None else tuple(tile_shape)
        self.tile_overlap = None if tile_overlap is None else tuple(tile_overlap)
        self.pipeline = pipeline

    def augmentations(self, h, w):
        """[(crop (x0, y0, cw, ch), scale value, flip, flip_direction, tile_offset or None)] in the reference's loop order."""
        if self.tile_shape is None:                     # MultiScaleFlipAug.__call__
            flip_args = [(False, None)] + ([(True, d) for d in self.flip_direction] if self.flip else [])
            return [((0, 0, w, h), sc, f, d, None) for sc in self.scales for f, d in flip_args]
        out = []                                        # CroppedTilesFlipAug.__call__: rows, columns, scales, flips, directions
        (w_ovr, h_ovr), (w_s, h_s) = self.tile_overlap, self.tile_shape
        for h_off in range(0, max(1, h - h_ovr), h_s - h_ovr):
            if h_off > 0:
                h_off = min(h - h_s, h_off)
            for w_off in range(0, max(1, w - w_ovr), w_s - w_ovr):
                if w_off > 0:
                    w_off = min(w - w_s, w_off)
                crop = (w_off, h_off, min(w_s, w - w_off), min(h_s, h - h_off))      # the slice img[h_off:h_off + h_s, ...]
                for sc in self.scales:
                    for f in ([False, True] if self.flip else [False]):
                        for d in self.flip_direction:
                            out.append((crop, sc, f, d, (w_off, h_off)))
        return out

    def __call__(self, sample, rng=None):
        h, w = sample['img'].shape[:2]
        plans = []
        for crop, sc, f, d, off in self.augmentations(h, w):
            extra = dict(flip_direction=d)
            if off is not None:
                extra['tile_offset'] = off
            plans.append(self.pipeline._plan(0, crop, flip=f, **{self.scale_key: sc}, **extra))
        return self.pipeline._run([sample], plans, batched=False)
