"""BasicLocator detector (T/mmdet/models/point/detectors/locator.py:6-32 on top of
SingleStageDetector/BaseDetector: T/mmdet/models/detectors/single_stage.py:35-104, base.py:114-247).
The drop-in boundary: ``forward_train(img, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore, gt_true_bboxes)
-> dict of losses`` and ``simple_test(img, img_metas, rescale, **gt_kwargs)``."""
import os
from collections import OrderedDict

import torch
import torch.distributed as dist
import torch.nn as nn

from ..ops import from_nchw as ops_from_nchw
from ..registry import DETECTORS, build_backbone, build_head, build_neck


@DETECTORS.register_module()
class BasicLocator(nn.Module):
    def __init__(self, backbone, neck=None, bbox_head=None, train_cfg=None, test_cfg=None, pretrained=None,
                 init_cfg=None):
        super().__init__()
        backbone = dict(backbone)
        backbone.setdefault('pretrained', pretrained)  # no checkpoints offline; weights arrive via load_state_dict
        self.backbone = build_backbone(backbone)
        self.neck = build_neck(neck) if neck is not None else None
        bbox_head = dict(bbox_head)
        bbox_head.update(train_cfg=train_cfg)
        bbox_head.update(test_cfg=test_cfg)
        self.bbox_head = build_head(bbox_head)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg

    def set_compute_dtype(self, dtype):
        """'fp32' (default: exact fp32 MFMA, the parity mode) or 'bf16' (BASELINE.json configs[4]: bf16 activations and
        weights from the stem output on, fp32 accumulate / statistics / losses).  Parameters stay fp32 masters."""
        dt = {'fp32': torch.float32, 'bf16': torch.bfloat16, torch.float32: torch.float32,
              torch.bfloat16: torch.bfloat16}[dtype]
        groups = getattr(self.backbone, 'groups', 1)
        if dt != torch.float32 and groups > 1:
            raise NotImplementedError('a grouped backbone (ResNeXt groups=%d) runs in the fp32 compute mode only: the bf16 compute mode '
                                      'has no grouped convolution' % groups)
        dilations = tuple(getattr(self.backbone, 'dilations', ()))
        if dt != torch.float32 and any(d != 1 for d in dilations):
            raise NotImplementedError('a dilated backbone (dilations=%r) runs in the fp32 compute mode only: the bf16 compute mode has no '
                                      'dilated convolution' % (dilations,))
        scales = getattr(self.backbone, 'scales', 0)
        if dt != torch.float32 and scales:
            raise NotImplementedError('a Res2Net backbone (scales=%d) runs in the fp32 compute mode only: the bf16 compute mode has no '
                                      'slice convolution' % scales)
        if dt != torch.float32 and getattr(self.backbone, 'fp32_only', None):      # a RegNet backbone (backbones/regnet.py)
            raise NotImplementedError(self.backbone.fp32_only)
        if dt != torch.float32 and getattr(self.neck, 'fp32_only', None):               # a CTResNetNeck (necks/ct_resnet_neck.py)
            raise NotImplementedError(self.neck.fp32_only)
        self.backbone.compute_dtype = dt
        return self

    @property
    def with_neck(self):
        return self.neck is not None

    def extract_feat(self, img):
        x = self.backbone(img)
        if self.with_neck:
            x = self.neck(x)
        return x

    # Independent images can be pushed through backbone -> neck -> head towers as ``num_streams`` sub-batches on
    # separate HIP streams: the deep layers launch fewer workgroups than the chip has slots (tile quantisation), and
    # blocks of another sub-batch's kernel fill those idle CUs.  The loss runs once on the re-joined batch (its
    # normalisers are batch-level).  Set with ``model.num_streams = k`` or CPR_STREAMS=k; 1 = single stream.
    num_streams = 1

    def _towers_multistream(self, img, k):
        head = self.bbox_head
        n = img.shape[0]
        k = max(1, min(k, n))
        bounds = [round(i * n / k) for i in range(k + 1)]
        main = torch.cuda.current_stream()
        if not hasattr(self, '_streams') or len(self._streams) < k:
            self._streams = [torch.cuda.Stream() for _ in range(k)]
        parts = []
        for i in range(k):
            s = self._streams[i]
            s.wait_stream(main)
            with torch.cuda.stream(s):
                feats = self.extract_feat(img[bounds[i]:bounds[i + 1]])
                cls_feat, _ = head(feats)
                parts.append(cls_feat)
        for i in range(k):
            main.wait_stream(self._streams[i])
        nlvl = len(parts[0])
        out = []
        for lvl in range(nlvl):
            t = torch.cat([ops_from_nchw(p[lvl]) for p in parts], dim=0)
            for p in parts:
                p[lvl].record_stream(main)
            out.append(t.permute(0, 3, 1, 2))
        return out, out

    # (Rounds 2-5 carried a hipGraph replay of backbone .. logit projection for the reference's samples_per_gpu = 2.  Measured in round 5 it
    # LOST to eager launches in both modes -- fp32 514 vs 558 img/s, configs[4] 526 vs 608: the capture needs whole-tensor statistics
    # buffers that the eager path fuses away, and at B = 2 the step is bound by tile quantisation over 256 CUs, not by launch
    # gaps -- so it was removed in round 6 together with its weight-signature tracking; git history has it.)

    def forward_train(self, img, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_true_bboxes=None):
        batch_input_shape = tuple(img[0].size()[-2:])
        for m in img_metas:
            m['batch_input_shape'] = batch_input_shape
        # (whenever autograd is on, in train() AND eval() mode -- the reference's forward_train is differentiable in either, e.g.
        # fine-tuning with the whole model in eval() for its frozen norm layers; validation losses belong under torch.no_grad(), which
        # keeps the forward-only path and holds no tapes.  CPR_AUTOGRAD=0 switches the bridge off altogether)
        if torch.is_grad_enabled() and img.is_cuda and os.environ.get('CPR_AUTOGRAD', '1') != '0' and \
                any(p.requires_grad for p in self.parameters()):
            # autograd is on: the losses must carry a graph, as the reference's do (its driver calls loss.backward():
            # T/mmdet/models/detectors/base.py:214-247 + mmcv OptimizerHook).  The recorded forward / HIP backward pair sits
            # behind torch.autograd.Functions (autograd_bridge.py); same loss values as the forward-only path below
            from .. import autograd_bridge
            why = autograd_bridge.unsupported_reason(self, gt_bboxes, gt_labels)
            if why is None:
                return autograd_bridge.forward_train(self, img, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore,
                                                     gt_true_bboxes)
            autograd_bridge.warn_once(why)
        k = int(os.environ.get('CPR_STREAMS', self.num_streams))
        # batch statistics are taken over the whole batch: a backbone with training-mode BatchNorm (norm_eval=False) runs single-stream
        if k > 1 and img.is_cuda and hasattr(self.bbox_head, 'loss') and not self.backbone.batch_stats_active():
            outs = self._towers_multistream(img, k)
            return self.bbox_head.loss(*outs, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=gt_bboxes_ignore,
                                       **({'gt_true_bboxes': gt_true_bboxes} if 'CPR' in type(self.bbox_head).__name__
                                          else {}))
        if self.with_neck and hasattr(self.neck, 'forward_lazy') and hasattr(self.bbox_head, 'forward_train_lazy') and \
                not getattr(self.neck, 'materialised', False):      # (a [.., BFP] neck hands over materialised levels)
            lazy = self.neck.forward_lazy(self.backbone(img), out_b8=getattr(self.bbox_head, 'accepts_b8', False))
            return self.bbox_head.forward_train_lazy(lazy, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore,
                                                     gt_true_bboxes)
        x = self.extract_feat(img)
        return self.bbox_head.forward_train(x, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore, gt_true_bboxes)

    def simple_test(self, img, img_metas, rescale=False, **kwargs):
        """Returns the head's refine output: list[(dets (G,6+), labels)] (bbox2result is host-side glue)."""
        feat = self.extract_feat(img)
        return self.bbox_head.simple_test(feat, img_metas, rescale=rescale, **kwargs)

    def forward_test(self, imgs, img_metas, **kwargs):
        for k in list(kwargs):  # the fork unwraps the per-aug lists of gt_* kwargs (base.py:147-150)
            if k.startswith('gt_') and isinstance(kwargs[k], (list, tuple)) and len(kwargs[k]) == 1 \
                    and isinstance(kwargs[k][0], (list, tuple)):
                kwargs[k] = kwargs[k][0]
        if isinstance(imgs, (list, tuple)):
            if len(imgs) > 1:          # test-time augmentation (base.py:152-157 -> single_stage.py:106-135)
                return self.aug_test(list(imgs), list(img_metas), **kwargs)
            imgs, img_metas = imgs[0], img_metas[0]
        return self.simple_test(imgs, img_metas, **kwargs)

    def extract_feats(self, imgs):
        return [self.extract_feat(img) for img in imgs]

    def aug_test(self, imgs, img_metas, rescale=False, **kwargs):
        """T/mmdet/models/detectors/single_stage.py:106-135: one forward per augmentation (one image each), merged by the head
        (P2PHead.aug_test_bboxes: the fork's tile / flip merge).  Returns the head's [(dets, labels)] (bbox2result is host glue)."""
        assert hasattr(self.bbox_head, 'aug_test_bboxes'), \
            '%s does not support test-time augmentation' % type(self.bbox_head).__name__
        return self.bbox_head.aug_test_bboxes(self.extract_feats(imgs), img_metas, rescale=rescale)

    def forward(self, img, img_metas, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(img, img_metas, **kwargs)
        return self.forward_test(img, img_metas, **kwargs)

    @staticmethod
    def _parse_losses(losses):
        """base.py:179-212: sum every key containing 'loss'; log vars averaged over ranks."""
        log_vars = OrderedDict()
        for name, value in losses.items():
            if isinstance(value, torch.Tensor):
                log_vars[name] = value.mean()
            elif isinstance(value, list):
                log_vars[name] = sum(v.mean() for v in value)
            else:
                raise TypeError('%s is not a tensor or list of tensors' % name)
        loss = sum(v for k, v in log_vars.items() if 'loss' in k)
        log_vars['loss'] = loss
        for name, value in log_vars.items():
            if dist.is_available() and dist.is_initialized():
                value = value.data.clone()
                dist.all_reduce(value.div_(dist.get_world_size()))
            log_vars[name] = value.item()
        return loss, log_vars

    def train_step(self, data, optimizer=None):
        """base.py:214-247.  With autograd enabled (how mmcv's runner calls it) ``loss`` carries a graph: ``loss.backward()``
        fills ``p.grad`` of every trainable parameter through the HIP backward kernels (autograd_bridge.py)."""
        losses = self(**data)
        loss, log_vars = self._parse_losses(losses)
        return dict(loss=loss, log_vars=log_vars, num_samples=len(data['img_metas']))
