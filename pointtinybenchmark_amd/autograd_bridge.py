"""``loss.backward()`` for the drop-in classes: the recorded forward / HIP backward of ``training.BackwardEngine`` behind
``torch.autograd.Function``s, so that the reference's own training driver runs them unmodified --
``BaseDetector.train_step`` returns a loss WITH a graph (T/mmdet/models/detectors/base.py:214-247), mmcv's ``OptimizerHook``
calls ``loss.backward()`` + ``clip_grad_norm_`` + ``optimizer.step()``, and ``MMDistributedDataParallel`` / torch DDP
(T/mmdet/apis/train.py:75-83) hooks the parameters' gradient accumulators and all-reduces buckets while the backward runs.

One Function per module boundary at which a TRUE gradient tensor exists (the lazy GroupNorm hand-offs inside the neck / head
chain have none: a raw map travels with a pending affine):

    image -> _StemFn (a trainable stem, frozen_stages=-1) -> _StageFn (layer1)            d(pooled stem map) between them
    image -> stem + frozen stages (no graph)
          -> _StageFn (layer2) -> _StageFn (layer3) -> _StageFn (layer4)          d(stage output) between them
          -> _LateralsFn: lateral 1x1 convs + GN + top-down adds -> the lateral sums the output convs read   d(lateral sums)
          -> _HeadLossFn: FPN 3x3 output conv(s) (+ a PAFPN's bottom-up path) + extra pyramid levels + head towers + projection + point stage + losses -> the loss vector
             (add_extra_convs='on_input': the last stage's output is one more input of it, d(stage output) comes back from it too)
    An HRFPN neck (necks/hrfpn.py) has one such boundary, its reduced map: _LateralsFn runs the per-level 1x1 convs and the fuse
    (d(reduced map) behind it), _HeadLossFn the pools, the biased output convs and the head.
    A CTResNetNeck (necks/ct_resnet_neck.py) too, its output map: _LateralsFn runs the whole neck on the last stage's output (in
    train() mode: batch statistics; an eval() neck is reported by unsupported_reason), _HeadLossFn the head alone.

Every Function takes its trainable parameters as explicit inputs, so they sit in the autograd graph as leaves: gradient
accumulators fire per Function -- the head's 9.4 MB of gradients (63 % of the backward's time) are final and on the wire while
the neck and backbone still compute, as with the trainer's own buckets.  The arithmetic is the trainer's kernel for kernel:
``p.grad`` after ``loss.backward()`` is BIT-equal to ``CprTrainer.forward_backward``'s (tests/test_gpu_autograd.py), which is
pinned to ``loss.backward()`` through the reference's own modules by tests/golden/cpr_grads_*.npz.

Both compute modes (round 5: the bf16 mode = mixed precision, the reference analogue being mmcv's ``Fp16OptimizerHook`` around an
unmodified ``loss.backward()``, T/mmdet/apis/train.py:116-119 -- see ``Bridge.carrier`` for how bf16 maps cross the Function
boundaries), every CPRHead option set that runs forward (``CPRHead.train_step_supported``) with one FPN output level, P2PHead with any number of
FPN output levels (extra pyramid levels beyond the laterals included) and points per cell, a frozen stem (standard or deep) or the standard trainable one (conv1 7x7/2, 3 -> 64; a trainable deep stem is refused).  Anything else keeps
the forward-only path and warns once.  SyncBN (nn.SyncBatchNorm in the backbone, a process group of more than one rank): the recorded
tapes carry each BatchNorm's group, so _StemFn / _StageFn synchronise their batch-statistics backward as the native trainer does -- every
rank issues the exchanges in program order on its main stream; dgamma / dbeta stay rank-local sums for DDP's reducer to average."""
import os
import warnings

import torch
from torch.autograd.function import once_differentiable

from .training import _BFP_UNDER_CPR, BackwardEngine, P2PBackwardEngine, _bfp_of, _inner_neck, _is_ctneck, _is_hrfpn


class _GtPack:
    """The non-tensor arguments of the head's loss (lists of per-image tensors, metas) carried through Function.apply."""

    def __init__(self, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore, gt_true_bboxes):
        self.img_metas, self.gt_bboxes, self.gt_labels = img_metas, gt_bboxes, gt_labels
        self.gt_bboxes_ignore, self.gt_true_bboxes = gt_bboxes_ignore, gt_true_bboxes


class Bridge:
    """Per-model state of the bridge: the backward engine (gradients into fresh tensors instead of ``p.grad``) and the
    parameter lists each Function takes."""

    def __init__(self, model, engine=None):
        """engine: an object with the segment API of training.BackwardEngine (tests drive the Functions with a CPU stand-in
        under gloo: tests/test_host_cpu.py); default: the HIP backward rules for the model's head."""
        self.model = model
        head = model.bbox_head
        if engine is None:
            two = os.environ.get('CPR_TRAIN_STREAMS', '2') != '1'
            engine = (P2PBackwardEngine if type(head).__name__ == 'P2PHead' else BackwardEngine)(model, two_streams=two)
        if getattr(engine, '_sink', None) is None:
            engine._sink = {}           # gradients go to fresh tensors handed to torch (any engine, also a caller's own)
        self.engine = engine
        bb, neck, bfp = model.backbone, _inner_neck(model.neck), _bfp_of(model.neck)
        self._maps = {}         # bf16 compute mode: data_ptr of an fp32 carrier -> the bf16 map it stands for (see carrier())
        self.darknet = bool(getattr(bb, 'darknet', False))      # one Function as well (_DarknetFn): its record is one, stem included
        self.hrnet = bool(getattr(bb, 'hrnet', False))
        if self.hrnet or self.darknet:      # HRNet, a DAG of branches: one Function from the image to the branch outputs (_HRNetFn), every parameter its input
            self.stem_params, self.stage_params = [], []
            self.backbone_params = [p for p in bb.parameters() if p.requires_grad]
        else:
            self.stem_params = [p for m in (getattr(bb, 'conv1', None), getattr(bb, 'bn1', None)) if m is not None
                                for p in m.parameters() if p.requires_grad]
            self.stage_params = [[p for p in getattr(bb, name).parameters() if p.requires_grad] for name in bb.res_layers]
        # (an HRFPN's reduction conv -- its per-level 1x1 convs -- plays the laterals' part: the same Function)
        # (a CTResNetNeck as a whole too: its output map is the boundary, nothing of it sits behind)
        ct = _is_ctneck(neck)
        self.lateral_params = [p for cm in ([neck.reduction_conv] if _is_hrfpn(neck) else [neck] if ct else neck.lateral_convs)
                               for p in cm.parameters() if p.requires_grad]
        # (a PAFPN's bottom-up modules sit between the output convs and the head: the same Function)
        # (so does the refine layer of a BFP behind the neck)
        neck_out = [] if ct else list(neck.fpn_convs) + list(getattr(neck, 'downsample_convs', ())) + list(getattr(neck, 'pafpn_convs', ()))
        if bfp is not None and bfp.refine_type is not None:
            neck_out.append(bfp.refine)
        self.head_params = [p for p in [q for cm in neck_out for q in cm.parameters()] + list(head.parameters())
                            if p.requires_grad]
        # add_extra_convs='on_input': the first extra conv reads the last backbone stage's output, one more differentiable input
        self.extra_on_input = bool(getattr(neck, 'extra_levels', 0)) and neck.add_extra_convs == 'on_input'
        self.signature = signature(model)

    # ---- mixed precision (bf16 compute mode) behind the same Functions.  The recorded maps are bf16, the gradients the backward
    # kernels hand from segment to segment are fp32 -- and autograd casts a gradient to the dtype of the output it belongs to, so
    # a bf16 map cannot be a Function output without rounding every boundary gradient to 8 bits.  The boundary therefore carries
    # an fp32 STAND-IN of the map's shape (all strides 0: one element of storage, never read or written); the Functions look
    # the real map up here.  fp32 maps pass through unchanged.
    def carrier(self, real):
        if real.dtype == torch.float32:
            return real
        ph = torch.empty_strided(tuple(real.shape), (0,) * real.dim(), dtype=torch.float32, device=real.device)
        self._maps[ph.data_ptr()] = real
        return ph

    def real(self, t):
        if t.dtype == torch.float32 and self._maps and t.dim() > 0 and all(s == 0 for s in t.stride()):
            return self._maps.get(t.data_ptr(), t)
        return t


def signature(model):
    return tuple(p.requires_grad for p in model.parameters())


def unsupported_reason(model, gt_bboxes=None, gt_labels=None):
    """None when ``forward_train`` can be differentiable, else why not."""
    bb, neck, head = model.backbone, model.neck, model.bbox_head
    if _bfp_of(neck) is not None:       # neck=[FPN | PAFPN, BFP] (necks/bfp.py NeckSequence checks the chain when it is built)
        if type(head).__name__ == 'CPRHead':
            return _BFP_UNDER_CPR
        neck = _inner_neck(neck)
    if _is_ctneck(neck):
        if bb.compute_dtype != torch.float32:
            return neck.fp32_only
        if not neck.training:
            from .necks.ct_resnet_neck import EVAL_TAPE
            return EVAL_TAPE
        n_outs = 1
    elif neck is None or type(neck).__name__ not in ('FPN', 'PAFPN', 'HRFPN') or len(neck.fpn_convs) < 1:
        return 'needs an FPN neck'
    elif _is_hrfpn(neck):
        n_outs = neck.num_outs
        if n_outs != 1 and type(head).__name__ == 'CPRHead':
            return 'CPRHead takes one pyramid level (cpr_head.py:487); this HRFPN has %d output levels' % n_outs
    else:
        n_outs = min(len(neck.lateral_convs), neck.num_outs) + getattr(neck, 'extra_levels', 0)    # outputs, not fpn_convs: max-pool extras
    if n_outs != 1 and type(head).__name__ == 'CPRHead' and type(neck).__name__ == 'PAFPN':
        return 'CPRHead takes one pyramid level (cpr_head.py:487); this PAFPN has %d output levels' % n_outs
    if n_outs != 1 and type(head).__name__ != 'P2PHead':
        return 'needs an FPN neck with num_outs == 1 (every shipped CPR config; CPRHead asserts one level, cpr_head.py:487)'
    if bb.compute_dtype != torch.float32 and getattr(bb, 'groups', 1) > 1:
        return 'a grouped backbone (ResNeXt groups=%d) runs in the fp32 compute mode only, not with the bf16 compute mode' % bb.groups
    if bb.compute_dtype != torch.float32 and any(d != 1 for d in getattr(bb, 'dilations', ())):
        return 'a dilated backbone (dilations=%r) runs in the fp32 compute mode only, not with the bf16 compute mode' % (tuple(bb.dilations),)
    if getattr(bb, 'scales', 0):          # a Res2Net backbone (backbones/res2net.py)
        if bb.compute_dtype != torch.float32:
            return 'a Res2Net backbone (scales=%d) runs in the fp32 compute mode only, not with the bf16 compute mode' % bb.scales
    if getattr(bb, 'fp32_only', None) and bb.compute_dtype != torch.float32:      # a RegNet backbone (backbones/regnet.py)
        return bb.fp32_only
    if bb.compute_dtype != torch.float32 and bb.batch_stats_active():
        return 'BatchNorm batch statistics (ResNet norm_eval=False) run in the fp32 compute mode only, not with the bf16 compute mode'
    if bb.compute_dtype != torch.float32 and type(head).__name__ not in ('CPRHead', 'P2PHead'):
        return 'the mixed-precision step (bf16 compute mode) covers the CPR and P2P locators'
    if any(p.requires_grad for p in bb.stem_parameters()) and bb.stem_train_reason() is not None:
        return bb.stem_train_reason()
    sparse = getattr(bb, 'sparse_outputs', False)      # MobileNetV2: out_indices picks among layer1 .. layer7, conv2
    hrnet = getattr(bb, 'hrnet', False)                # HRNet: no out_indices, no frozen_stages -- any (conv, BN) pair may be frozen, as a whole
    if hrnet and bb.freeze_reason() is not None:
        return bb.freeze_reason()
    if getattr(bb, 'darknet', False):                  # Darknet: out_indices picks among conv1, conv_res_block1 .. 5; pairs as HRNet's
        return bb.freeze_reason() or _head_reason(model, head, n_outs, gt_bboxes, gt_labels)
    if not (sparse or hrnet) and tuple(bb.out_indices) != tuple(range(len(bb.res_layers))):
        return 'out_indices must name every stage'
    for i, name in enumerate(() if hrnet else bb.res_layers):
        first = [next(blk.parameters()) for blk in bb.stage_blocks(i)] if sparse else [blk.conv1.weight for blk in getattr(bb, name)]
        if len({p.requires_grad for p in first}) > 1:
            return 'stage %s is partly frozen' % name
    return _head_reason(model, head, n_outs, gt_bboxes, gt_labels)


def _head_reason(model, head, n_outs, gt_bboxes, gt_labels):
    bb = model.backbone
    kind = type(head).__name__
    if kind == 'CPRHead':
        R = 1
        if gt_bboxes is not None and gt_labels is not None and len(gt_labels) and len(gt_labels[0]):
            R = max(1, int(gt_bboxes[0].shape[0]) // int(len(gt_labels[0])))     # (every image brings num_gts * R boxes: the head asserts)
        if not head.train_step_supported(R):
            return 'this CPRHead option set has no hand-written backward (CPRHead.train_step_supported)'
        if head.num_cls_fcs > 0 and bb.compute_dtype != torch.float32:
            return 'num_cls_fcs > 0 trains in the fp32 compute mode (the FC backward reads fp32 activations)'
    elif kind == 'P2PHead':
        if not getattr(head, 'train_cfg', None):
            return 'P2PHead trains with a train_cfg (the shipped P2P configs)'
        if len(head.strides) != n_outs:
            return 'P2PHead needs one FPN output per stride (%d strides, num_outs %d)' % (len(head.strides), n_outs)
    else:
        return 'no backward rules for head %s' % kind
    return None


_WARNED = set()


def warn_once(reason):
    if reason not in _WARNED:
        _WARNED.add(reason)
        warnings.warn('BasicLocator.forward_train was called with autograd enabled but returns losses WITHOUT a graph: %s.  '
                      'Wrap forward-only calls in torch.no_grad() to silence this.' % reason, stacklevel=3)


def get_bridge(model):
    br = getattr(model, '_autograd_bridge_state', None)
    if br is None or br.signature != signature(model):
        br = Bridge(model)
        model._autograd_bridge_state = br
    return br


# ------------------------------------------------------------------------------------------------ Functions
# Thin: every Function calls one forward_* / backward_* pair of the engine (training.BackwardEngine).  An autograd OUTPUT must
# not be reachable from its own ctx (ctx -> state -> output -> grad_fn -> ctx would be a reference cycle that keeps a batch of
# maps alive until the garbage collector runs): the engine's state holds the output's storage under another tensor object
# (``.detach()`` aliases), never the returned object itself.  This is part of the segment contract, for every engine (also a caller's
# own): the Functions do not look into a state, so ``forward_head_loss`` itself stores the loss vector's alias, not the vector.
_CONSUMED = 'the recorded forward of this step was already consumed (a second backward / retain_graph is not supported)'


class _StemFn(torch.autograd.Function):
    """The standard ResNet stem (conv1 7x7/2 + bn1 + ReLU + max-pool 3x3/2, resnet.py:630-637) when it trains: the image (no
    gradient) -> the pooled NHWC map; conv1.weight, bn1.weight, bn1.bias as inputs."""

    @staticmethod
    def forward(ctx, bridge, img, *params):
        out, rec = bridge.engine.forward_stem(img)
        ctx.bridge, ctx.rec, ctx.params = bridge, rec, params
        return bridge.carrier(out)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        eng = ctx.bridge.engine
        assert ctx.rec is not None, _CONSUMED
        eng.backward_stem(ctx.rec, dout.contiguous())
        grads = eng.collect(ctx.params)
        ctx.rec = None
        return (None, None) + grads


class _HRNetFn(torch.autograd.Function):
    """An HRNet backbone (backbones/hrnet.py), stem included: the image (no gradient) -> the NHWC branch outputs of stage4's last
    module; every trainable backbone parameter as an input.  Its branches exchange maps after every module, so there is no chain of
    single-input stages to cut it into: the backward is BackwardEngine._backward_backbone on the recorded forward, as the native
    trainer runs it."""

    @staticmethod
    def forward(ctx, bridge, img, *params):
        bb = bridge.model.backbone
        tape = []
        outs = bb.run(img, tape)
        tape[0]['stages'][-1]['modules'][-1]['out'] = [o.detach() for o in outs]      # (no output reachable from its own ctx)
        ctx.bridge, ctx.tape, ctx.params = bridge, tape, params
        ctx.set_materialize_grads(False)      # an output nobody differentiates hands None down, as in the native trainer
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *douts):
        eng, tape = ctx.bridge.engine, ctx.tape
        assert tape is not None, _CONSUMED
        d_stage = {k: d.contiguous() for k, d in enumerate(douts) if d is not None}
        eng._backward_backbone(ctx.bridge.model.backbone, tape, d_stage)
        grads = eng.collect(ctx.params)
        ctx.tape = None
        return (None, None) + grads


class _DarknetFn(torch.autograd.Function):
    """A Darknet backbone (backbones/darknet.py), conv1 included: the image (no gradient) -> the NHWC outputs of its ``out_indices``
    stages; every trainable backbone parameter as an input.  Its recorded forward is one record, walked by
    BackwardEngine._backward_backbone as the native trainer walks it, so both drivers run the same kernels in the same order."""

    @staticmethod
    def forward(ctx, bridge, img, *params):
        bb = bridge.model.backbone
        tape = []
        outs = bb.run(img, tape)
        # (no output reachable from its own ctx: a stage output is the next stage's recorded input, conv1's the first stage's)
        own = {id(o): o.detach() for o in outs}
        rec = tape[0]
        rec['a0'] = own.get(id(rec['a0']), rec['a0'])
        for srec in rec['stages']:
            for r in [srec] + srec['blocks']:
                for k, v in r.items():
                    if torch.is_tensor(v):
                        r[k] = own.get(id(v), v)
        ctx.bridge, ctx.tape, ctx.params = bridge, tape, params
        ctx.set_materialize_grads(False)      # an output nobody differentiates hands None down, as in the native trainer
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *douts):
        eng, tape = ctx.bridge.engine, ctx.tape
        assert tape is not None, _CONSUMED
        d_stage = {k: d.contiguous() for k, d in enumerate(douts) if d is not None}
        eng._backward_backbone(ctx.bridge.model.backbone, tape, d_stage)
        grads = eng.collect(ctx.params)
        ctx.tape = None
        return (None, None) + grads


class _StageFn(torch.autograd.Function):
    """One trainable ResNet stage (T/mmdet/models/backbones/resnet.py:262-302 per block) on an NHWC map."""

    @staticmethod
    def forward(ctx, bridge, stage, x, *params):
        out, tape = bridge.engine.forward_stage(stage, bridge.real(x))
        out = bridge.carrier(out)
        if tape and isinstance(tape[-1], dict) and tape[-1].get('out') is out:
            tape[-1]['out'] = out.detach()
        ctx.bridge, ctx.tape, ctx.params = bridge, tape, params
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        eng, tape = ctx.bridge.engine, ctx.tape
        assert tape is not None, _CONSUMED
        dx = eng.backward_stage(tape, dout.contiguous(), ctx.needs_input_grad[2])
        grads = eng.collect(ctx.params)
        ctx.tape = None
        return (None, None, dx) + grads


class _LateralsFn(torch.autograd.Function):
    """FPN lateral convs + GroupNorm + the top-down nearest-upsample adds (T/mmdet/models/necks/fpn.py:166-188) -> the lateral
    sums the output convs read: the finest alone when num_outs == 1, else one output per FPN output level, finest first."""

    @staticmethod
    def forward(ctx, bridge, n_in, *args):
        xs, params = args[:n_in], args[n_in:]
        lat, recs = bridge.engine.forward_laterals([bridge.real(x) for x in xs])
        ctx.bridge, ctx.recs, ctx.params, ctx.n_in = bridge, recs, params, n_in
        ctx.multi = isinstance(lat, (tuple, list))
        return tuple(bridge.carrier(t) for t in lat) if ctx.multi else bridge.carrier(lat)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dlat):
        eng = ctx.bridge.engine
        assert ctx.recs is not None, _CONSUMED
        need = [ctx.needs_input_grad[2 + i] for i in range(ctx.n_in)]
        d = [g.contiguous() for g in dlat] if ctx.multi else dlat[0].contiguous()
        dxs = eng.backward_laterals(ctx.recs, d, need)
        grads = eng.collect(ctx.params)
        ctx.recs = None
        return (None, None) + tuple(dxs) + grads


class _HeadLossFn(torch.autograd.Function):
    """FPN output conv -> head towers -> projection / output convs -> point stage -> the loss vector: (5,) for CPRHead
    (gt_loss, pos_loss, bag_acc, neg_loss, num_sample; cpr_head.py:1101-1229), (B, 2) for P2PHead (loss_cls, loss_pts per
    image; p2p_head.py:172-248).  Everything between the finest lateral sum and the losses hands raw maps + pending GroupNorm
    affines from layer to layer, so this is the smallest unit with a true gradient on both sides."""

    @staticmethod
    def forward(ctx, bridge, pack, n_lat, *args):
        """args: n_lat maps -- the lateral sums, then (a neck with add_extra_convs='on_input': ``bridge.extra_on_input``) the last
        backbone stage's output, which the first extra conv reads --, then the parameters."""
        eng = bridge.engine
        lats, params = args[:n_lat], args[n_lat:]
        kw = {}
        if bridge.extra_on_input:
            kw['extra_src'] = bridge.real(lats[-1])
            lats = lats[:-1]
        lat = bridge.real(lats[0]) if len(lats) == 1 else tuple(bridge.real(t) for t in lats)
        out, state = eng.forward_head_loss(lat, pack.img_metas, pack.gt_bboxes, pack.gt_labels,
                                           pack.gt_bboxes_ignore, pack.gt_true_bboxes, **kw)
        ctx.bridge, ctx.state, ctx.params, ctx.n_lat = bridge, state, params, n_lat
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        eng = ctx.bridge.engine
        assert ctx.state is not None, _CONSUMED
        # what torch hands over: d(total) / d(loss vector) -- ones where _parse_losses summed a term, zero on bag_acc; a scaled
        # total (loss scaling, gradient accumulation) arrives as that scale.  The loss-backward kernels multiply by it on the device
        kw = {}
        if ctx.bridge.extra_on_input:
            kw['need_src'] = ctx.needs_input_grad[3 + ctx.n_lat - 1]
        dlat = eng.backward_head_loss(ctx.state, gout.contiguous().float(), **kw)
        grads = eng.collect(ctx.params)
        ctx.state = None
        return (None, None, None) + (tuple(dlat) if ctx.n_lat > 1 else (dlat,)) + grads


# ------------------------------------------------------------------------------------------------ entry point
def forward_train(model, img, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_true_bboxes=None):
    """BasicLocator.forward_train with a graph: the same dict of losses, differentiable wrt every trainable parameter.  The
    CPR losses are the forward-only values up to fp32 summation order (<= 2e-6 relative, asserted by tests/test_gpu_train_step.py:
    the recorded forward fuses the producer GroupNorm into the 3x3 consumers' loads where the forward-only path materialises it
    and runs Winograd); P2PNet's differ in the last bits for one more reason -- the recorded path keeps the 3x3 output convs on
    the conv kernel (its backward walks them) where the forward-only path uses the tap projection.  The recorded maps live until
    ``loss.backward()`` has run or the returned losses die: evaluate losses you do not differentiate under ``torch.no_grad()``."""
    bridge = get_bridge(model)
    eng = bridge.engine
    eng.begin_step()
    eng._sink.clear()
    bridge._maps.clear()
    bb, neck = model.backbone, _inner_neck(model.neck)
    if bridge.hrnet or bridge.darknet:
        if bridge.backbone_params:
            feats = list((_HRNetFn if bridge.hrnet else _DarknetFn).apply(bridge, img.detach(), *bridge.backbone_params))
        else:
            with torch.no_grad():
                feats = bb.run(img)
        return _neck_head_loss(model, bridge, feats, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore, gt_true_bboxes)
    if bridge.stem_params:
        x = _StemFn.apply(bridge, img.detach(), *bridge.stem_params)
    else:
        with torch.no_grad():
            # (ResNet.run_stem: with deep_stem ``bb.stem`` is the reference's Sequential; any other backbone runs its ``stem``)
            x = (getattr(bb, 'run_stem', None) or bb.stem)(img)
    feats = []
    sparse = getattr(bb, 'sparse_outputs', False)      # MobileNetV2: the outputs are the out_indices stages, nothing behind the last runs
    for i in range(bb.last_stage() + 1 if sparse else len(bb.res_layers)):
        params = bridge.stage_params[i]
        if params:
            x = _StageFn.apply(bridge, i, x, *params)
        else:
            with torch.no_grad():
                x = bb.run_stage(i, bridge.real(x))
        if not sparse or i in bb.out_indices:
            feats.append(x)
    return _neck_head_loss(model, bridge, feats, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore, gt_true_bboxes)


def _neck_head_loss(model, bridge, feats, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore, gt_true_bboxes):
    """The part of forward_train behind the backbone: feats, its NHWC outputs -> the dict of losses."""
    eng, neck = bridge.engine, _inner_neck(model.neck)
    if _is_ctneck(neck):      # it reads the last backbone map alone
        xs = feats[-1:]
    else:
        assert len(feats) == len(neck.in_channels)
        xs = feats if _is_hrfpn(neck) else feats[neck.start_level:neck.start_level + len(neck.lateral_convs)]
    lat = _LateralsFn.apply(bridge, len(xs), *xs, *bridge.lateral_params)
    lats = tuple(lat) if isinstance(lat, (tuple, list)) else (lat,)
    if bridge.extra_on_input:
        lats = lats + (feats[neck.backbone_end_level - 1],)
    pack = _GtPack(img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore, gt_true_bboxes)
    out = _HeadLossFn.apply(bridge, pack, len(lats), *lats, *bridge.head_params)
    bridge._maps.clear()          # every forward consumer has run; the backward reads the tapes
    return eng.loss_dict(out)
