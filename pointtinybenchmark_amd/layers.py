"""Parameter containers + the fused conv/norm building blocks used by backbone, neck and heads.

nn.Conv2d / nn.BatchNorm2d / nn.GroupNorm objects are used ONLY as parameter holders so the state-dict
keys match the reference checkpoint layout; their ``forward`` is never called -- all
compute goes through ``ops`` (HIP kernels)."""
import struct

import torch
import torch.nn as nn

from . import _lib, ops


_WEIGHT_EPOCH = [0]


def bump_weight_epoch():
    """Called by the native optimizer: its kernels update parameters through raw pointers, which torch's version counter
    does not see."""
    _WEIGHT_EPOCH[0] += 1


# False: every fold / pack lapses with the weight epoch and is rebuilt lazily (rounds 3-5; tests)
REFRESH_IN_PLACE = [True]

_FOLDS, _PACKS16, _PACKS32 = 'cpr_bn_fold_multi', 'cpr_pack_weights_bf16_multi', 'cpr_pack_weights_multi'
_PACKSG = 'cpr_pack_weights_grouped_multi'


class FoldJob:
    """Recomputes a folded BatchNorm's (scale, shift) in place: one 64-byte FoldJob row of cpr_bn_fold_multi (csrc/pack.hip)."""
    multi = _FOLDS
    fold = None
    _ROW = struct.Struct('<7Qif')

    def __init__(self, bn, value):
        self.bn, self.value, self.C = bn, value, bn.weight.numel()
        self._tensors = (bn.weight, bn.bias, bn.running_mean, bn.running_var) + tuple(value)

    def ptrs(self):
        """The device pointers of this job's row: gamma, beta, mean, var, scale, shift."""
        return tuple(map(torch.Tensor.data_ptr, self._tensors))

    def row(self, ptrs, extent):
        """-> (this job's table row, the launch extent with it: the widest channel count)."""
        return self._ROW.pack(*ptrs, 0, self.C, self.bn.eps), max(extent, self.C)


class PackJob:
    """Re-packs ``weight`` into the PackedConv ``value`` in place: one 64-byte row of cpr_pack_weights_bf16_multi (csrc/pack.hip
    PackJob: the bf16 [rows][K] image and the fragment image) or of cpr_pack_weights_multi (Pack32Job: the fp32 [rows][Kpad] image,
    after which the Winograd images are transformed again).  transpose: a data-gradient pack; ``fold``: the FoldJob whose scale it
    multiplies in."""
    _ROW16, _ROW32 = struct.Struct('<4Q8i'), struct.Struct('<3Q10i')

    def __init__(self, weight, value, transpose, fold):
        self.weight, self.value, self.transpose, self.fold = weight, value, transpose, fold
        self.shape = O, I, KH, KW = weight.shape
        rows, cols = (I, O) if transpose else (O, I)
        bf16 = value.dtype == torch.bfloat16
        self.multi = _PACKS16 if bf16 else _PACKS32
        self.nblocks = max(1, min(64, (rows * (KH * KW * cols // 2 if bf16 else value.Kpad) + 255) // 256))

    def ptrs(self):
        """The device pointers of this job's row: weight, scale, pack, fragment image (built on first use, frag_image)."""
        pc = self.value
        return (self.weight.data_ptr(), 0 if self.fold is None else self.fold.value[0].data_ptr(), pc.w.data_ptr(),
                0 if pc.wfrag is None else pc.wfrag.data_ptr())

    def row(self, ptrs, block0):
        """-> (this job's table row, the launch extent with it: the blocks of the jobs so far, this job's start at block0)."""
        pc, nb = self.value, self.nblocks
        if self.multi is _PACKS16:
            return self._ROW16.pack(*ptrs, *self.shape, self.transpose, block0, nb, 0), block0 + nb
        return self._ROW32.pack(*ptrs[:3], nb, 0, *self.shape, pc.Cin, pc.Kpad, self.transpose, block0), block0 + nb

    def refresh_images(self, stream):
        """The Winograd images of a refreshed fp32 pack: G g G^T again, in place (one launch each)."""
        pc = self.value
        for img, fn in ((pc.wino, 'cpr_wino_pack_weights'), (pc.wino32, 'cpr_wino32_pack_weights')):
            if img is not None:
                _lib.call(fn, pc.w.data_ptr(), img.data_ptr(), pc.Cin, pc.Cout, pc.Kpad, stream)


class GroupPackJob(PackJob):
    """The same for a grouped pack (ops.PackedConv with groups > 1): one 48-byte row of cpr_pack_weights_grouped_multi
    (csrc/conv_group.hip GroupPackJob).  It has no Winograd or fragment image."""
    multi = _PACKSG
    _ROWG = struct.Struct('<3Q6i')

    def __init__(self, weight, value, transpose, fold):
        self.weight, self.value, self.transpose, self.fold = weight, value, transpose, fold
        self.shape = tuple(weight.shape)
        self.nblocks = max(1, min(64, (value.w.numel() + 255) // 256))

    def ptrs(self):
        """The device pointers of this job's row: weight, scale, pack."""
        return (self.weight.data_ptr(), 0 if self.fold is None else self.fold.value[0].data_ptr(), self.value.w.data_ptr())

    def row(self, ptrs, block0):
        pc, nb = self.value, self.nblocks
        return self._ROWG.pack(*ptrs, pc.C, pc.cg, self.transpose, block0, nb, 0), block0 + nb


def _pack_job(pc, weight, transpose=0, fold=None):
    """The PackJob of a pack that a pack kernel built from an fp32 contiguous device weight; None for anything else (the strided
    layers' PhasedDgrad): that entry lapses with the weight epoch."""
    if isinstance(pc, ops.PackedConv) and weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous():
        return (GroupPackJob if pc.groups > 1 else PackJob)(weight, pc, transpose, fold)
    return None


class _Entry:
    __slots__ = ('tensors', 'ver', 'val', 'ready')

    def __init__(self, tensors, ver, val, ready):
        self.tensors, self.ver, self.val, self.ready = tensors, ver, val, ready


class _PackCache:
    """Repacked weights / folded norms, rebuilt when the source parameter is modified in place."""

    def __init__(self):
        self._d = {}             # key -> _Entry
        self._jobs = {}          # key -> FoldJob | PackJob of that key's current value: refresh_all recomputes it IN PLACE
        self._tables = None      # (row pointers, launches) of refresh_all's device job tables: None when a job came or went

    @staticmethod
    def _ver(tensors):
        ver = tuple((t.data_ptr(), t._version) for t in tensors)
        if any(t.requires_grad for t in tensors):
            ver = ver + (_WEIGHT_EPOCH[0],)
        return ver

    def get(self, key, tensors, make, refresh=None):
        """refresh (optional): val -> FoldJob | PackJob | None, how refresh_all recomputes ``val`` in place after the native trainer's
        optimizer step instead of letting the entry lapse.  A rebuild drops the key's previous job."""
        ver = self._ver(tensors)
        hit = self._d.get(key)
        if hit is not None and hit.ver == ver:
            hit.ready = ops.wait_ready(hit.ready)
            return hit.val
        val = make()
        job = refresh(val) if refresh is not None else None
        if self._jobs.pop(key, None) is not None or job is not None:
            self._tables = None
        if job is not None:
            self._jobs[key] = job
        # whatever make() enqueued (pack kernels, torch ops building a bf16 pack / a folded norm / a bias vector) ran on the
        # CURRENT stream: a reader on another stream (sub-batches of CPR_STREAMS > 1, the trainer's side stream) must order
        # itself behind it -- the event lives with the entry until it has completed
        self._d[key] = _Entry(list(tensors), ver, val, ops.record_ready())
        return val

    def _live(self):
        """(entry, job) of every job refresh_all recomputes: its value is still its entry's, and a pack linked to a fold only
        goes with that very fold job (a fold rebuilt since, or left without a job, lets the pack lapse and rebuild from it)."""
        if not REFRESH_IN_PLACE[0]:
            return []
        live = [(self._d[k], j) for k, j in self._jobs.items() if self._d[k].val is j.value]
        jobs = {j for _, j in live}
        return [(e, j) for e, j in live if j.fold is None or j.fold in jobs]

    def refresh_all(self):
        """Called by the native trainer right after its optimizer step (the parameters changed through raw pointers, the weight epoch
        was bumped): every live job is recomputed in place by ONE multi-tensor launch per kind -- folds first, the data-gradient
        packs multiply the refreshed scales in (csrc/pack.hip: bit for bit the single-tensor kernels) -- and its entry re-stamped with
        the current version, instead of ~320 lazy rebuilds -- launches, allocations and Python -- spread over the next step (4.3 of
        the 37 ms of a configs[4] step, profiles/round6_stale_packs_ab.txt).  Entries without a job lapse and rebuild as before."""
        live = self._live()
        if not live:
            return
        ptrs = [j.ptrs() for _, j in live]
        if self._tables is None or self._tables[0] != ptrs:       # the job set changed or a pointer moved
            rows = {_FOLDS: [], _PACKS16: [], _PACKS32: [], _PACKSG: []}
            extent = dict.fromkeys(rows, 0)
            for (_, j), p in zip(live, ptrs):
                row, extent[j.multi] = j.row(p, extent[j.multi])
                rows[j.multi].append(row)
            dev = live[0][0].tensors[0].device
            self._tables = ptrs, [(fn, torch.frombuffer(bytearray(b''.join(r)), dtype=torch.uint8).to(dev), len(r), extent[fn])
                                  for fn, r in rows.items() if r]
        stream = torch.cuda.current_stream().cuda_stream
        for fn, table, n, ext in self._tables[1]:
            _lib.call(fn, table.data_ptr(), n, ext, stream)
        for _, j in live:
            if j.multi is _PACKS32:
                j.refresh_images(stream)
        ready = ops.record_ready()
        for e, j in live:
            e.ver, e.ready = self._ver(e.tensors), ready
            if isinstance(j, PackJob):
                j.value.ready = ready


def packed_conv(cache, conv, dtype=torch.float32):
    return cache.get(('pc', id(conv), dtype), [conv.weight],
                     lambda: ops.PackedConv(conv.weight, conv.stride[0], conv.padding[0], dtype, groups=conv.groups,
                                            dilation=conv.dilation[0]),
                     lambda pc: _pack_job(pc, conv.weight))


# ---- dense fp32 layers whose maps sit at a padded channel pitch (pad channels exact zeros: RegNet blocks, the Res2Net 1x1 layers, an
# FPN lateral reading a RegNet stage in place): packs with zero rows / columns and folds with zero scale / shift in the pad.  None of
# these entries has a refresh job: they lapse with the weight epoch and rebuild from the refreshed parameters.
def _zero_embedded(weight, Op, Ip):
    """``weight`` (O, I, k, k) in the corner of an (Op, Ip, k, k) tensor of zeros."""
    O, I = weight.shape[:2]
    w = torch.zeros((Op, Ip) + tuple(weight.shape[2:]), device=weight.device, dtype=torch.float32)
    w[:O, :I].copy_(weight.detach())
    return w


def _zero_extended(t, Op):
    tp = t.new_zeros((Op,))
    tp[:t.numel()].copy_(t)
    return tp


def packed_conv_padded(cache, conv, Op, Ip):
    """packed_conv of the dense ``conv`` (O, I, k, k) at (Op, Ip): rows >= O and columns >= I zero."""
    if (Op, Ip) == tuple(conv.weight.shape[:2]):
        return packed_conv(cache, conv)
    assert conv.groups == 1
    return cache.get(('pc_pad', id(conv), Op, Ip), [conv.weight],
                     lambda: ops.PackedConv(_zero_embedded(conv.weight, Op, Ip), conv.stride[0], conv.padding[0]))


def folded_bn(cache, bn):
    """Eval-mode BatchNorm as a per-channel affine for the conv epilogue:
    scale = gamma / sqrt(var + eps), shift = beta - mean * scale."""
    def make():
        if bn.weight.is_cuda:
            return ops.bn_fold(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)[:2]
        with torch.no_grad():
            scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).float().contiguous()
            shift = (bn.bias - bn.running_mean * scale).float().contiguous()
        return scale, shift
    def job(val):
        ok = bn.weight.is_cuda and all(t.dtype == torch.float32 and t.is_contiguous()
                                       for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var, val[0], val[1]))
        return FoldJob(bn, val) if ok else None
    return cache.get(('bn', id(bn)), [bn.weight, bn.bias, bn.running_mean, bn.running_var], make, job)


def folded_bn_padded(cache, bn, Op):
    """folded_bn zero-extended to Op channels: relu(0 * 0 + 0) = 0 keeps the pad channels of the layer's output exact zeros."""
    if Op == bn.weight.numel():
        return folded_bn(cache, bn)
    return cache.get(('bn_pad', id(bn), Op), [bn.weight, bn.bias, bn.running_mean, bn.running_var],
                     lambda: tuple(_zero_extended(t, Op) for t in folded_bn(cache, bn)))


def bn_inv_sigma(cache, bn):
    """1 / sqrt(running_var + eps) of an eval-mode BatchNorm (the folded-BN parameter gradients, ops.bn_fold_bwd)."""
    return cache.get(('bn_is', id(bn)), [bn.running_var],
                     lambda: ops.bn_fold(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, True)[2])


def dgrad_packed(cache, conv, bn=None, dtype=torch.float32, pitch=None):
    """The packed weights of the data gradient of ``conv`` (ops.dgrad_pack; bf16 stride 1: PackedConv.for_dgrad_bf16) with the
    folded scale of the eval-mode ``bn`` multiplied in -- or the raw weights (bn None: a batch-statistics layer).  pitch (a grouped
    layer with eval-mode ``bn``): the channel pitch of its gradient maps."""
    w, stride, pad, dil = conv.weight, conv.stride[0], conv.padding[0], conv.dilation[0]
    if pitch is not None and pitch != w.shape[0]:
        assert bn is not None and conv.groups > 1 and dtype == torch.float32

        def make_p():
            scale, _ = folded_bn(cache, bn)
            return ops.dgrad_pack(w, stride, pad, scale=scale, groups=conv.groups, pitch=pitch)

        def job_p(pc):
            fold = cache._jobs.get(('bn', id(bn)))
            return None if fold is None else _pack_job(pc, w, 1, fold)
        return cache.get(('dgrad', id(conv), dtype, pitch), [w, bn.weight, bn.running_var], make_p, job_p)
    if bn is None:
        return cache.get(('dgrad_raw', id(conv)), [w], lambda: ops.dgrad_pack(w, stride, pad, groups=conv.groups, dilation=dil),
                         lambda pc: _pack_job(pc, w, 1))

    def make():
        scale, _ = folded_bn(cache, bn)
        if dtype == torch.float32 or stride != 1 or conv.groups > 1 or dil != 1:
            return ops.dgrad_pack(w, stride, pad, scale=scale, dtype=dtype, groups=conv.groups, dilation=dil)
        return ops.PackedConv.for_dgrad_bf16(w, pad, scale=scale)

    def job(pc):        # linked to the fold job of the scale make() multiplied in
        fold = cache._jobs.get(('bn', id(bn)))
        return None if fold is None else _pack_job(pc, w, 1, fold)
    return cache.get(('dgrad', id(conv), dtype), [w, bn.weight, bn.running_var], make, job)


def dgrad_packed_padded(cache, conv, bn, Op, Ip):
    """dgrad_packed of the dense ``conv`` at (Op, Ip): the data gradient of maps at a padded pitch arrives padded, its pad channels exact
    zeros (zero rows / columns, and a zero folded scale, in the pad).  bn None: no scale (a GroupNorm layer reading a padded map)."""
    w = conv.weight
    if (Op, Ip) == tuple(w.shape[:2]):
        return dgrad_packed(cache, conv, bn)
    assert conv.groups == 1
    if bn is None:
        return cache.get(('dgrad_pad_raw', id(conv), Op, Ip), [w], lambda: ops.dgrad_pack(_zero_embedded(w, Op, Ip), conv.stride[0], conv.padding[0]))
    return cache.get(('dgrad_pad', id(conv), Op, Ip), [w, bn.weight, bn.running_var],
                     lambda: ops.dgrad_pack(_zero_embedded(w, Op, Ip), conv.stride[0], conv.padding[0],
                                            scale=_zero_extended(folded_bn(cache, bn)[0], Op)))


class ConvModule(nn.Module):
    """conv -> norm -> act container with mmcv's attribute names (``conv``, ``gn``/``bn``), bias='auto'."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias='auto', conv_cfg=None,
                 norm_cfg=None, act_cfg=dict(type='ReLU'), inplace=True):
        super().__init__()
        assert conv_cfg is None or conv_cfg.get('type') in (None, 'Conv2d'), 'only plain Conv2d is on this path'
        self.with_norm = norm_cfg is not None
        self.with_activation = act_cfg is not None
        if bias == 'auto':
            bias = not self.with_norm
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, bias=bias)
        self.norm_name = None
        if self.with_norm:
            cfg = dict(norm_cfg)
            t = cfg.pop('type')
            rg = cfg.pop('requires_grad', True)
            if t == 'GN':
                self.norm_name = 'gn'
                norm = nn.GroupNorm(num_channels=out_channels, **cfg)
            elif t == 'BN':
                self.norm_name = 'bn'
                norm = nn.BatchNorm2d(out_channels, **cfg)
            else:
                raise KeyError(t)
            for p in norm.parameters():
                p.requires_grad = rg
            self.add_module(self.norm_name, norm)
        if self.with_activation:
            assert act_cfg.get('type', 'ReLU') == 'ReLU'

    @property
    def norm(self):
        return getattr(self, self.norm_name) if self.norm_name else None


def conv_gn(cache, m, x, in_ab=None, in_relu=False, materialize=True, up=None, save=None, consume_input=False,
            out_b8=False):
    """Run a ConvModule(conv, GN[, ReLU]) on an NHWC tensor (or a channel-blocked one, ops.is_b8: Winograd layers only).

    The GroupNorm statistics come out of the conv epilogue (no extra pass: always for the Winograd layers, for the
    direct kernel when the map is tile-aligned); with ``materialize=False`` the raw conv output and the per-(image,
    channel) affine (a, b) are returned so the CONSUMER conv applies normalisation + ReLU while loading its input (no
    apply pass either).
    ``save`` (dict): training mode -- records what the backward needs (conv input and its pending affine, raw output,
    GroupNorm affine and statistics) and keeps the raw output intact (the apply pass goes out of place).
    ``consume_input``: the caller owns ``x`` and nobody else reads it -- a pending producer-GroupNorm may be applied in place.
    ``out_b8``: the consumer is a Winograd layer -- hand it the raw output channel-blocked (forward only, materialize=False).

    Fused-on-load vs one streaming apply pass: the Winograd layers (3x3, stride 1) transform every input element once per
    cout tile on its way into the 4x4 patch transform -- 2 packed FMA/max per 8 bytes, invisible behind the MFMAs -- so they
    always fuse.  The direct kernel's KxK consumers re-transform every element K*K x (cout tiles) times (3x3 256->256 at
    160x160, B=16: 3.52 ms fused vs 3.30 ms plain) while gn_apply touches it once at HBM speed (0.14 ms): those take the
    materialised input in forward-only mode, 1x1 consumers fuse.
    """
    gn = m.norm
    blocked = ops.is_b8(x)
    if not blocked and x.shape[-1] != m.conv.in_channels:      # a backbone map at its padded pitch (the caller vouches for the zeros)
        assert x.dtype == torch.float32 and in_ab is None and x.shape[-1] == ops.pad32(m.conv.in_channels), (x.shape[-1], m.conv.in_channels)
        pc = packed_conv_padded(cache, m.conv, m.conv.out_channels, x.shape[-1])
    else:
        pc = packed_conv(cache, m.conv, x.dtype)
    if blocked:
        N, _, H, W, _ = x.shape
    else:
        N, H, W, _ = x.shape
    wino = x.dtype == torch.float32 and ops.wino_eligible(pc, H, W, x.dtype) and pc.Cin <= 512
    if blocked and not wino:       # a channel-blocked map reached a layer that cannot read it: back to NHWC (+ its pending affine)
        x = ops.gn_apply_b8(x, *(in_ab if in_ab is not None else (None, None)), relu=in_relu and in_ab is not None)
        in_ab, blocked = None, False
    OH, OW = pc.out_hw(H, W)
    fused_stats = wino or (OH * OW) % 128 == 0
    fuse_in = in_ab is not None and (wino or ((H * W) % 128 == 0 and pc.stride == 1 and (OH, OW) == (H, W)
                                              and x.dtype == torch.float32))   # the bf16 kernel does not fuse the producer GN
    if fuse_in and not wino and save is None and pc.KH * pc.KW > 1:
        fuse_in = False
    if in_ab is not None and not fuse_in:
        x = ops.gn_apply(x, in_ab[0], in_ab[1], relu=in_relu, out=x if (consume_input and save is None) else None)
        in_ab = None
    out_b8 = bool(out_b8) and wino and save is None and not materialize
    bias = m.conv.bias
    if fused_stats:
        raw, part = ops.conv2d(x, pc, bias=bias, in_ab=in_ab, in_relu=in_relu, gn_part=True, out_b8=out_b8)
    else:
        raw = ops.conv2d(x, pc, bias=bias, in_ab=in_ab, in_relu=in_relu)
        part = ops.gn_stats(raw)
    if save is not None:
        a, b, mean, rstd = ops.gn_finalize(part, gn.weight, gn.bias, N, OH * OW, gn.num_groups, gn.eps, want_stats=True)
        save.update(module=m, x=x, in_ab=in_ab, in_relu=in_relu, raw=raw, a=a, b=b, mean=mean, rstd=rstd)
    else:
        a, b = ops.gn_finalize(part, gn.weight, gn.bias, N, OH * OW, gn.num_groups, gn.eps)
    if not materialize:
        return raw, (a, b)
    return ops.gn_apply(raw, a, b, relu=m.with_activation, up=up, out=None if save is not None else raw)
