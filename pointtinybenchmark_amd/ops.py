"""Thin tensor -> C-ABI wrappers.  PyTorch here is plumbing only: it owns the device memory
(caller-allocated outputs and workspaces) and the stream; every op runs in a
hand-written HIP kernel from libcprhip.so on the current HIP stream.

Activations are NHWC fp32 (see csrc/conv_mfma.hip for why).  ``as_nchw`` / ``from_nchw`` expose them as
NCHW-shaped (channels_last-strided) tensors, which is what crosses the reference's module boundaries.
"""
import collections
import ctypes
import math

import torch

from . import _lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(t, dtype=torch.float32):
    """dtype may be a tuple of accepted dtypes (fp32 / bf16 activations)."""
    if not t.is_cuda:
        raise _lib.CprHipError('HIP op called with a CPU tensor: the product path has no CPU fallback')
    ok = t.dtype in dtype if isinstance(dtype, tuple) else t.dtype == dtype
    assert ok and t.is_contiguous(), (t.dtype, t.stride())
    return t


ACT = (torch.float32, torch.bfloat16)   # activation dtypes: fp32 (default, parity mode) or bf16 (configs[4] mode)


def as_nchw(x_nhwc):
    """(N,H,W,C) buffer -> NCHW-shaped view (channels_last strides, no copy)."""
    return x_nhwc.permute(0, 3, 1, 2)


def pad32(c):
    return (c + 31) // 32 * 32


def as_nchw_padded(buf, C):
    """A map kept at a channel pitch -- buf (N,H,W,Cp), Cp = pad32(C), channels [C, Cp) exact zeros as its producer wrote them -> the
    NCHW-shaped view (N,C,H,W) of its real channels (no copy).  The producer vouches for the pad: the view carries the buffer, and
    ``padded_buffer`` hands it to a consumer that reads the pitch in place (a 1x1 pack with zero columns in the pad)."""
    if buf.shape[-1] == C:
        return as_nchw(buf)
    view = buf[..., :C].permute(0, 3, 1, 2)
    view._cpr_padded = buf
    return view


def padded_buffer(x):
    """The (N,H,W,Cp) buffer behind a view made by as_nchw_padded, or None.  Only that very view qualifies: a tensor derived from it (a
    slice, a copy, a user's own view of a wider tensor) carries no voucher and takes the copying route (from_nchw)."""
    buf = getattr(x, '_cpr_padded', None)
    if buf is None:
        return None
    N, C, H, W = x.shape
    ok = buf.dim() == 4 and tuple(buf.shape[:3]) == (N, H, W) and buf.shape[3] == pad32(C) and buf.is_contiguous() and \
        x.data_ptr() == buf.data_ptr() and x.stride() == (H * W * buf.shape[3], 1, W * buf.shape[3], buf.shape[3])
    return buf if ok else None


def from_nchw(x):
    """NCHW-shaped tensor -> contiguous (N,H,W,C) buffer; free when x is already channels_last."""
    y = x.permute(0, 2, 3, 1)
    if y.is_contiguous():
        return y
    return nchw_to_nhwc(x)


NECK_INPUT_COPIES = [0]      # maps of a width that is no multiple of 32 that reached neck_input without a voucher and were copied


def neck_input(x):
    """What a neck reads of one backbone output (N,C,H,W): the NHWC buffer.  C % 32 == 0: from_nchw.  Else the dense kernels need the
    pitch roundup(C, 32) with zeros behind the real channels: a view the backbone made (as_nchw_padded) hands over its buffer as it is;
    any other tensor -- a user's slice of a wider tensor, whatever lies behind it -- is copied into a zeroed buffer of that pitch."""
    C = x.shape[1]
    if C % 32 == 0 or C <= 4:
        return from_nchw(x)
    buf = padded_buffer(x)
    if buf is None:
        N, _, H, W = x.shape
        buf = torch.zeros((N, H, W, pad32(C)), device=x.device, dtype=torch.float32)
        buf[..., :C].copy_(x.permute(0, 2, 3, 1))      # layout copy only (not on the benchmarked path: the counter shows a view that lost
        NECK_INPUT_COPIES[0] += 1                      # its voucher on the way -- .detach(), a hook that re-wraps the outputs)
    return buf


def nchw_to_nhwc(x):
    N, C, H, W = x.shape
    if C <= 4:  # network input: pad to 4 channels for the stem's float4 taps
        x = _check(x.contiguous())
        out = torch.empty((N, H, W, 4), device=x.device, dtype=torch.float32)
        _lib.call('cpr_nchw_to_nhwc4', _ptr(x), _ptr(out), N, C, H, W, _stream())
        return out
    return x.permute(0, 2, 3, 1).contiguous()  # layout copy only (not on the benchmarked path)


def nhwc_to_nchw_dense(x_nhwc):
    N, H, W, C = x_nhwc.shape
    out = torch.empty((N, C, H, W), device=x_nhwc.device, dtype=torch.float32)
    _lib.call('cpr_nhwc_to_nchw', _ptr(_check(x_nhwc)), _ptr(out), N, C, H, W, _stream())
    return out


class PackedConv:
    """Conv weight repacked for the implicit-GEMM kernel: [Cout][KH][KW][Cin'] fp32, rows padded to a
    multiple of 32 floats.  Cin' = 4 for the 3-channel stem (zero 4th channel)."""
    wfrag = None    # bf16: the weights in MFMA-fragment order (frag_image), built on first use for Cout % 256 == 0
    wino = None     # transformed weights of the Winograd path, built on first use (conv3x3_wino)
    wino32 = None   # the same for the two-workgroups-per-CU kernel (csrc/conv_wino32.hip: chunks of 4 input channels)
    ready = None    # record_ready() behind the last pack kernel (weights / Winograd image); see pack_ready()
    groups = 1      # > 1: a grouped 3x3 layer (ResNeXt conv2) in the layout of csrc/conv_group.hip, see _init_grouped
    cg = None       # ... its group width (channels per group)
    C = None        # ... its real channels; Cin = Cout = the pitch of the maps it reads and writes (>= C, RegNet)
    dilation = 1    # > 1: a dilated 3x3 / stride 1 / padding == dilation layer (fp32; cpr_conv2d_fwd_dil, cpr_conv_group_fwd_dil)

    def _packed(self):
        """A pack kernel was just enqueued on the current stream: consumers on OTHER streams (CPR_STREAMS > 1 sub-batches)
        must order themselves behind it."""
        self.ready = record_ready()

    def __init__(self, weight, stride=1, padding=0, dtype=torch.float32, groups=1, pitch=None, dilation=1):
        dilation = int(dilation)
        assert dilation >= 1, 'dilation must be >= 1, got %d' % dilation
        if dilation != 1 and dtype == torch.bfloat16:
            raise NotImplementedError('dilation=%d: a dilated convolution runs in the fp32 compute mode only (the bf16 kernels have no '
                                      'dilated form)' % dilation)
        if groups > 1:
            self._init_grouped(weight, stride, padding, dtype, groups, None, 0, pitch, dilation)
            return
        assert pitch is None, 'a channel pitch is the grouped kernels\' (dense layers pad their packs)'
        Cout, Cin, KH, KW = weight.shape
        if dilation != 1:      # the pack itself is the undilated one; the launch carries the tap step
            assert (KH, KW) == (3, 3) and stride == 1 and padding == dilation and Cin % 32 == 0, \
                'dilation=%d: 3x3 / stride 1 / padding == dilation with Cin %% 32 == 0, got weight %s stride %d padding %d' \
                % (dilation, tuple(weight.shape), stride, padding)
            self.dilation = dilation
        w = weight.detach().to(torch.float32).permute(0, 2, 3, 1)  # OHWI
        self.dtype = dtype
        if dtype == torch.bfloat16:
            # bf16 kernel: K chunks of 64 elements, no stem mode (the 3-channel stem stays on the fp32 kernel)
            assert Cin % 64 == 0, 'bf16 conv needs Cin % 64 == 0'
            self.Cout, self.Cin, self.KH, self.KW, self.Kpad = Cout, Cin, KH, KW, KH * KW * Cin
            self.stride, self.padding = stride, padding
            if weight.is_cuda:
                self._pack_bf16(weight, None, 0)      # one launch: the [Cout][K] image and, where it is used, the fragment image
                return
            self.w = w.reshape(Cout, KH * KW * Cin).to(torch.bfloat16).contiguous()
            return
        if Cin <= 4:
            cin_p = 4
        else:
            assert Cin % 32 == 0, 'input channels must be a multiple of 32 (or <= 4 for the stem)'
            cin_p = Cin
        K = KH * KW * cin_p
        Kpad = (K + 31) // 32 * 32
        self.Cout, self.Cin, self.KH, self.KW, self.Kpad = Cout, cin_p, KH, KW, Kpad
        self.stride, self.padding = stride, padding
        if weight.is_cuda:       # one HIP launch (the training step re-packs every conv after each optimizer update)
            src = weight.detach()
            if src.dtype != torch.float32 or not src.is_contiguous():
                src = src.float().contiguous()
            self.w = torch.empty((Cout, Kpad), device=weight.device, dtype=torch.float32)
            _lib.call('cpr_pack_weights', _ptr(src), None, _ptr(self.w), Cout, Cin, KH, KW, cin_p, Kpad, 0, _stream())
            self._packed()
            return
        wp = torch.zeros((Cout, KH, KW, cin_p), device=weight.device, dtype=torch.float32)
        wp[..., :Cin] = w
        packed = torch.zeros((Cout, Kpad), device=weight.device, dtype=torch.float32)
        packed[:, :K] = wp.reshape(Cout, K)
        self.w = packed.contiguous()

    def _init_grouped(self, weight, stride, padding, dtype, groups, scale, transpose, pitch=None, dilation=1):
        """A grouped 3x3 / padding 1 conv, weight (C, cg, 3, 3) with cg = C / groups in GROUP_WIDTHS (csrc/conv_group.hip): self.w is the
        kernel's own image, 9 * cg * C floats [tap][cg / 4][4][C / 4][4] (cpr_pack_weights_grouped), not the dense [Cout][Kpad] rows.
        transpose: the data-gradient pack -- per group in / out channels swapped, taps flipped, ``scale`` multiplied in.  fp32 only.
        pitch: floats between the pixels of the maps the layer reads and writes (>= C, a multiple of 4; None: C) -- the pack is the same."""
        C, cg, KH, KW = weight.shape
        pitch = C if pitch is None else int(pitch)
        assert pitch >= C and pitch % 4 == 0, 'grouped conv: the channel pitch %d must be a multiple of 4 and >= C = %d' % (pitch, C)
        if dtype != torch.float32:
            raise NotImplementedError('a grouped convolution (groups=%d) runs in the fp32 compute mode only, not in %s' % (groups, dtype))
        assert weight.is_cuda, 'the grouped pack is built on the device'
        assert cg * groups == C and cg in GROUP_WIDTHS and (KH, KW) == (3, 3) and padding == dilation and stride in (1, 2), \
            'grouped conv: 3x3 / padding == dilation / stride 1 or 2 with a group width in %s, got weight %s groups %d stride %d ' \
            'padding %d dilation %d' % (GROUP_WIDTHS, tuple(weight.shape), groups, stride, padding, dilation)
        assert dilation == 1 or (stride == 1 and pitch == C), \
            'grouped conv: dilation=%d needs stride 1 and unpitched maps, got stride %d pitch %d (C = %d)' % (dilation, stride, pitch, C)
        self.dtype, self.groups, self.cg, self.C = torch.float32, groups, cg, C
        self.Cout, self.Cin, self.KH, self.KW, self.Kpad = pitch, pitch, 3, 3, 9 * cg
        self.stride, self.padding = stride, dilation
        if dilation != 1:
            self.dilation = dilation
        src = weight.detach()
        if src.dtype != torch.float32 or not src.is_contiguous():
            src = src.float().contiguous()
        self.w = torch.empty((9 * cg * C,), device=weight.device, dtype=torch.float32)
        _lib.call('cpr_pack_weights_grouped', _ptr(src), _ptr(scale), _ptr(self.w), C, cg, int(transpose), _stream())
        self._packed()

    @staticmethod
    def dgrad_padding(k, padding, dilation=1):
        """Padding of the stride-1 conv over dy (flipped taps, the same dilation) that yields the data gradient of a k x k conv with
        ``padding`` and ``dilation``: the taps span d (k - 1) pixels, so d (k - 1) - p (k - 1 - p undilated; d for a 3x3 with p = d)."""
        return dilation * (k - 1) - padding

    @classmethod
    def for_dgrad_grouped(cls, weight, groups, scale=None, pitch=None, dilation=1):
        """The grouped pack of the stride-1 grouped conv over dy (zero-inserted first for a stride-2 layer, conv2d_dgrad) that yields
        the data gradient of a grouped 3x3 / padding == dilation conv: what for_dgrad is to the dense layers (padding 2 d - d = d)."""
        self = cls.__new__(cls)
        self._init_grouped(weight, 1, self.dgrad_padding(3, dilation, dilation), torch.float32, groups, scale, 1, pitch, dilation)
        return self

    def _pack_bf16(self, weight, scale, transpose):
        """csrc/pack.hip, cpr_pack_weights_bf16: OIHW fp32 master -> self.w (bf16 [rows][K]) and, for rows % 256 == 0, self.wfrag.
        transpose: the data-gradient pack (rows = input channels, taps flipped, ``scale`` of the forward conv folded in)."""
        src = weight.detach()
        if src.dtype != torch.float32 or not src.is_contiguous():
            src = src.float().contiguous()
        O, I, KH, KW = src.shape
        rows = self.Cout
        self.w = torch.empty((rows, self.Kpad), device=src.device, dtype=torch.bfloat16)
        want_frag = rows % 256 == 0 and self.Kpad % 64 == 0 and WFRAG[0]
        if want_frag:
            self.wfrag = torch.empty((rows // 64, self.Kpad // 16, 2, 2, 32, 8), device=src.device, dtype=torch.bfloat16)
        _lib.call('cpr_pack_weights_bf16', _ptr(src), _ptr(scale), _ptr(self.w), _ptr(self.wfrag if want_frag else None), O, I, KH, KW,
                  int(transpose), _stream())
        self._packed()

    @classmethod
    def for_dgrad_bf16(cls, weight, padding, scale=None, pad_override=None):
        """The bf16 pack of the stride-1 conv over dy that yields the data gradient of a stride-1 conv (mixed-precision step): in / out
        channels swapped, taps flipped, the forward conv's folded-BN ``scale`` multiplied in (fp32) before the rounding, padding
        K-1-p (``pad_override``: explicit padding, used by the per-parity sub-kernels of a strided conv, which need not be square).
        The same bits as PackedConv((w * scale).flip(2, 3).permute(1, 0, 2, 3), 1, K-1-p, bf16), one launch."""
        Cout, Cin, KH, KW = weight.shape
        assert (KH == KW or pad_override is not None) and weight.is_cuda and Cout % 64 == 0
        self = cls.__new__(cls)
        self.dtype = torch.bfloat16
        self.Cout, self.Cin, self.KH, self.KW, self.Kpad = Cin, Cout, KH, KW, KH * KW * Cout
        self.stride, self.padding = 1, (KH - 1 - padding if pad_override is None else pad_override)
        self._pack_bf16(weight, scale, 1)
        return self

    def frag_image(self):
        """bf16 weights in the fragment order of conv_bf16_dma_kernel<4, 2, 4, true> (include/cpr_hip.h, cpr_conv2d_fwd_bf16):
        [cout / 64][k / 16][j][lane = l + 32 h][8] = w[64 g + 2 l + j][16 ks + 8 h .. + 8] -- the 16 bytes lane (l, h) of cout block j
        feeds to one MFMA, so a wave's weight operand of a k-step is two coalesced 1 KB loads.  None when the layer cannot take
        the 256 x 256 tile (Cout % 256, K % 64)."""
        if self.dtype != torch.bfloat16 or self.Cout % 256 != 0 or self.Kpad % 64 != 0 or not WFRAG[0]:
            return None
        if self.wfrag is None:
            G, KS = self.Cout // 64, self.Kpad // 16
            self.wfrag = self.w.view(G, 32, 2, KS, 2, 8).permute(0, 3, 2, 4, 1, 5).contiguous()
            self._packed()      # built on the calling stream: the other sub-batch streams order themselves behind it (pack_ready)
        return self.wfrag

    @classmethod
    def for_dgrad(cls, weight, padding, scale=None, pad_override=None, dilation=1):
        """Weights of the stride-1 conv over dy that yields the data gradient: in/out channels swapped, taps flipped,
        optional per-output-channel scale of the FORWARD conv (folded BatchNorm) multiplied in, padding d (K-1) - p at the forward's
        dilation d (``pad_override``: explicit padding, used by the per-parity sub-kernels of a strided conv)."""
        Cout, Cin, KH, KW = weight.shape
        assert (KH == KW or pad_override is not None) and weight.is_cuda
        dilation = int(dilation)
        assert dilation == 1 or ((KH, KW) == (3, 3) and pad_override is None and padding == dilation and Cout % 32 == 0), \
            'dilation=%d: the data gradient of a 3x3 / padding == dilation layer, got weight %s padding %d' \
            % (dilation, tuple(weight.shape), padding)
        assert Cout % 32 == 0 or Cout <= 4, 'gradient channels must be a multiple of 32 (or <= 4)'
        self = cls.__new__(cls)
        self.dtype = torch.float32
        cols_p = 4 if Cout <= 4 else Cout
        K = KH * KW * cols_p
        Kpad = (K + 31) // 32 * 32
        self.Cout, self.Cin, self.KH, self.KW, self.Kpad = Cin, cols_p, KH, KW, Kpad
        self.stride, self.padding = 1, (self.dgrad_padding(KH, padding, dilation) if pad_override is None else pad_override)
        if dilation != 1:
            self.dilation = dilation
        src = weight.detach()
        if src.dtype != torch.float32 or not src.is_contiguous():
            src = src.float().contiguous()
        self.w = torch.empty((Cin, Kpad), device=weight.device, dtype=torch.float32)
        _lib.call('cpr_pack_weights', _ptr(src), _ptr(scale), _ptr(self.w), Cout, Cin, KH, KW, cols_p, Kpad, 1, _stream())
        self._packed()
        return self

    def out_hw(self, H, W):
        d = self.dilation
        return ((H + 2 * self.padding - d * (self.KH - 1) - 1) // self.stride + 1,
                (W + 2 * self.padding - d * (self.KW - 1) - 1) // self.stride + 1)


CONV_RELU, CONV_OUT_BF16, CONV_RES_MASK, CONV_COLSUM = 1, 2, 4, 8      # include/cpr_hip.h CPR_CONV_*
GROUP_WIDTHS = (4, 8, 16, 24, 32, 40, 48, 56)      # channels per group the grouped 3x3 kernels are built for (csrc/conv_group.hip)
# bf16 mode: hand the fragment-order weight image to the conv launcher (the 256 x 256 tile then loads its weight operand
# straight into registers, csrc/conv_bf16_dma.hip BD instance).  False keeps both operands on the LDS-DMA path (tests).
WFRAG = [True]
# profilers (bench.py) set [0] = True; the template instance of the last conv launch is then left in [1] as
# (kind, code).  Host-side, single-threaded bookkeeping of a value the C ABI returns through an out-parameter.
TRACE_CONV_VARIANT = [False, None]

# 3x3 / stride 1 / pad 1 fp32 layers run as fused Winograd F(2x2,3x3) (csrc/conv_wino.hip, 2.25x fewer multiplies) when the
# map fills its 16x16 output regions well enough; False keeps every layer on the direct implicit GEMM (tests).
WINOGRAD = [True]
WINO_MIN_FILL = 0.6      # useful share of the 16x16 regions (40x40 -> 0.69 runs Winograd, 20x20 -> 0.39 stays direct)


def record_ready():
    """(event, stream) recorded behind the work just enqueued on the current stream, for wait_ready; None without a device or
    while the stream is being captured."""
    if not torch.cuda.is_available() or torch.cuda.is_current_stream_capturing():
        return None
    ev = torch.cuda.Event()
    ev.record()
    return ev, torch.cuda.current_stream().cuda_stream


def wait_ready(ready):
    """Order the current stream behind ``ready`` (record_ready) unless it is the producer's own stream.  Returns what the holder
    keeps: None once the event has completed."""
    if ready is None or torch.cuda.is_current_stream_capturing():      # (a capture starts after a synchronised warm-up)
        return ready
    ev, stream = ready
    if ev.query():
        return None
    cur = torch.cuda.current_stream()
    if cur.cuda_stream != stream:
        cur.wait_event(ev)
    return ready


def pack_ready(pc):
    """Order the current stream behind the kernels that packed ``pc`` (they may have run on another stream: the first
    sub-batch of a multi-stream forward packs, the others only read)."""
    if pc.ready is not None:
        pc.ready = wait_ready(pc.ready)


def wino_eligible(pc, H, W, dtype=torch.float32):
    if pc.dilation != 1:      # the Winograd transforms are those of adjacent taps
        return False
    if not (pc.groups == 1 and WINOGRAD[0] and dtype == torch.float32 and pc.dtype == torch.float32 and pc.KH == 3 and pc.KW == 3 and
            pc.stride == 1 and pc.padding == 1 and pc.Cin % 16 == 0 and pc.Cin >= 32 and pc.Cout % 64 == 0):
        return False
    fill = (H * W) / float(((H + 15) // 16 * 16) * ((W + 15) // 16 * 16))
    return fill >= WINO_MIN_FILL


# Which fused Winograd kernel serves a 3x3 layer: '32' = the two-workgroups-per-CU form (csrc/conv_wino32.hip: 8 x 16 pixel
# regions, 4-wave workgroups), '64' = the one-workgroup-per-CU form (csrc/conv_wino.hip: 16 x 16 regions).  The choice is a function
# of the LAYER alone (never of the batch size: an image of a big batch must equal its single-image run bit for bit, and the two
# kernels differ in accumulation order).  '64' / '32' forces one of them everywhere it can run (tests).
WINO_TILE = ['auto']


def wino_instance(pc, H, W, fused_affine):
    """'32' or '64' for a Winograd-eligible layer."""
    can32 = pc.Cin % 8 == 0 and (not fused_affine or pc.Cin <= 256)
    if WINO_TILE[0] == '64' or not can32:
        return '64'
    if WINO_TILE[0] == '32':
        return '32'
    return WINO_AUTO(pc, H, W, fused_affine)


WINO32_MAX_PIXELS = 40 * 40


def WINO_AUTO(pc, H, W, fused_affine):
    """Keyed on the LAYER GEOMETRY alone (never on the batch size: an image of a big batch must equal its single-image run bit
    for bit, and the two kernels differ in accumulation order).  Measured per shape on MI355X (profiles/round4_wino32_ab.txt,
    DESIGN.md 4.1d): the two-workgroups-per-CU kernel loses on the large maps at every batch (160x160x256: 8.9 vs 7.0 ms at
    B = 64, 0.359 vs 0.319 at B = 2; 80x80x128: 0.63 vs 0.54; 160x160x64: 0.71 vs 0.59) and wins where one image brings fewer
    16 x 16 regions than a tenth of the chip: 40x40x256 at the reference's batch of 2 runs 0.061 vs 0.071 ms (B = 2: 18 regions of
    16 x 16 per image against 30 of 8 x 16), at B = 64 it costs 0.709 vs 0.672 ms.  Maps of at most 40 x 40 pixels (layer3 of
    a 640 x 640 input) therefore take the 8 x 16-region kernel at every batch: -14 % on those layers at B = 2, +5 % at B = 64
    (0.3 % of that step)."""
    return '32' if H * W <= WINO32_MAX_PIXELS else '64'


def wino_gn_slots(pc, H, W, fused_affine):
    """GroupNorm-statistics slots per image of the Winograd kernel that serves this layer."""
    if wino_instance(pc, H, W, fused_affine) == '32':
        return ((H + 7) // 8) * ((W + 15) // 16)
    return ((H + 15) // 16) * ((W + 15) // 16)


def is_b8(x):
    """Channel-blocked activation (N, C/8, H, W, 8): the layout Winograd layers hand to each other (csrc/conv_wino.hip)."""
    return x.dim() == 5 and x.shape[-1] == 8


def conv3x3_wino(x, pc, scale=None, bias=None, relu=False, gn_part=False, out=None, in_ab=None, in_relu=False,
                 out_b8=False):
    """Winograd F(2x2,3x3) path of conv2d for 3x3 / stride 1 / pad 1 fp32 layers.  x: NHWC (N,H,W,Cin) or channel-blocked
    (N,Cin/8,H,W,8); out_b8=True returns the blocked form (N,Cout/8,H,W,8).  in_ab=(a,b): input read as relu?(x*a+b).
    gn_part=True also returns one (sum, sumsq) slot per output region of the kernel that runs (16x16, or 8x16 for the
    two-workgroups-per-CU form): (N * wino_gn_slots(...), Cout, 2)."""
    _check(x, ACT)
    in_b8 = is_b8(x)
    if in_b8:
        N, _, H, W, _ = x.shape
        Cin = x.shape[1] * 8
    else:
        N, H, W, Cin = x.shape
    assert x.dtype == torch.float32 and Cin == pc.Cin and pc.KH == 3 and pc.stride == 1 and pc.padding == 1
    inst = wino_instance(pc, H, W, in_ab is not None)
    attr, pack_fn = ('wino32', 'cpr_wino32_pack_weights') if inst == '32' else ('wino', 'cpr_wino_pack_weights')
    if getattr(pc, attr) is None:     # G g G^T of the packed weights, once per PackedConv (= once per weight update)
        pack_ready(pc)
        wino = torch.empty((16 * pc.Cin * pc.Cout,), device=x.device, dtype=torch.float32)
        _lib.call(pack_fn, _ptr(pc.w), _ptr(wino), pc.Cin, pc.Cout, pc.Kpad, _stream())
        setattr(pc, attr, wino)
        pc._packed()
    pack_ready(pc)
    shape = (N, pc.Cout // 8, H, W, 8) if out_b8 else (N, H, W, pc.Cout)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    assert tuple(out.shape) == shape and out.is_contiguous()
    part = None
    if gn_part:
        part = torch.empty((N * wino_gn_slots(pc, H, W, in_ab is not None), pc.Cout, 2), device=x.device, dtype=torch.float32)
    a = b = None
    if in_ab is not None:
        a, b = in_ab
        assert Cin <= 512
    _lib.call('cpr_conv3x3_wino32_fwd' if inst == '32' else 'cpr_conv3x3_wino_fwd', _ptr(x), _ptr(getattr(pc, attr)), _ptr(out),
              _ptr(scale), _ptr(bias), _ptr(a), _ptr(b), _ptr(part), N, H, W, Cin, pc.Cout, CONV_RELU if relu else 0, int(in_relu),
              (1 if in_b8 else 0) | (2 if out_b8 else 0), _stream())
    if TRACE_CONV_VARIANT[0]:
        TRACE_CONV_VARIANT[1] = ('wino32' if inst == '32' else 'wino',
                                 (1 if in_b8 else 0) | (2 if out_b8 else 0) | (4 if in_ab is not None else 0))
    return (out, part) if gn_part else out


def gn_apply_b8(x, a=None, b=None, relu=False):
    """Channel-blocked (N,C/8,H,W,8) -> NHWC (N,H,W,C), optionally through y = relu?(x*a+b)."""
    assert is_b8(x)
    N, C8, H, W, _ = _check(x, ACT).shape
    y = torch.empty((N, H, W, C8 * 8), device=x.device, dtype=torch.float32)
    _lib.call('cpr_gn_apply_b8', _ptr(x), _ptr(a), _ptr(b), _ptr(y), N, H, W, C8 * 8, int(relu), _stream())
    return y


def conv2d(x, pc, scale=None, bias=None, residual=None, relu=False, in_ab=None, in_relu=False, gn_part=False,
           out=None, out_dtype=None, res_mask=False, colsum=False, out_b8=False):
    """x (N,H,W,Cin) -> (N,OH,OW,Cout).  Epilogue: *scale[c] + bias[c] (+residual) (ReLU).
    in_ab=(a,b) applies x*a[n,c]+b[n,c] (+ReLU) to the input on load (fused GroupNorm of the producer; fp32 only).
    gn_part=True also returns per-128-pixel-tile per-channel (sum, sumsq) partials of the output.
    bf16 inputs run the bf16 MFMA kernel (fp32 accumulate); out_dtype overrides the output type (the fp32 stem can
    emit bf16, the bf16 logit projection emits fp32).
    Backward helpers (fp32): res_mask=True turns ``residual`` into a ReLU mask source (out = residual > 0 ? v : 0);
    colsum=True also returns the per-channel sums of the output (C,), taken from the epilogue partials."""
    _check(x, ACT)
    pack_ready(pc)
    if is_b8(x):     # channel-blocked input: only the Winograd layers read it
        assert residual is None and not (res_mask or colsum) and out_dtype in (None, torch.float32) and \
            wino_eligible(pc, x.shape[2], x.shape[3], x.dtype), 'channel-blocked input needs a Winograd-eligible layer'
        return conv3x3_wino(x, pc, scale, bias, relu, gn_part, out, in_ab, in_relu, out_b8)
    N, H, W, Cin = x.shape
    assert Cin == pc.Cin, (Cin, pc.Cin)
    assert x.dtype == pc.dtype, 'weights were packed for %s, input is %s' % (pc.dtype, x.dtype)
    OH, OW = pc.out_hw(H, W)
    odt = out_dtype or x.dtype
    if pc.groups > 1:
        # grouped 3x3 (csrc/conv_group.hip): scale / bias / ReLU epilogue or the raw form, nothing else
        assert residual is None and in_ab is None and not (in_relu or gn_part or res_mask or colsum or out_b8) and \
            odt == torch.float32, 'the grouped conv has no residual, GroupNorm-statistics, fused-input-affine or bf16 form'
        if out is None:
            out = torch.empty((N, OH, OW, pc.Cout), device=x.device, dtype=torch.float32)
        assert tuple(out.shape) == (N, OH, OW, pc.Cout) and out.is_contiguous()
        if scale is not None or bias is not None:
            assert (scale is None or _check(scale).numel() >= pc.C) and (bias is None or _check(bias).numel() >= pc.C)
        if pc.dilation != 1:
            assert Cin == pc.C and pc.stride == 1
            _lib.call('cpr_conv_group_fwd_dil', _ptr(x), _ptr(pc.w), _ptr(out), _ptr(scale), _ptr(bias), N, H, W, Cin, pc.cg, pc.dilation,
                      CONV_RELU if relu else 0, _stream())
        elif Cin == pc.C:
            _lib.call('cpr_conv_group_fwd', _ptr(x), _ptr(pc.w), _ptr(out), _ptr(scale), _ptr(bias), N, H, W, Cin, pc.cg, pc.stride,
                      CONV_RELU if relu else 0, _stream())
        else:      # maps at a channel pitch: pad channels never read, written as +0.0
            _lib.call('cpr_conv_group_fwd_pitch', _ptr(x), _ptr(pc.w), _ptr(out), _ptr(scale), _ptr(bias), N, H, W, pc.C, Cin, pc.cg,
                      pc.stride, CONV_RELU if relu else 0, _stream())
        if TRACE_CONV_VARIANT[0]:
            TRACE_CONV_VARIANT[1] = ('group', pc.cg)
        return out
    if residual is None and not (res_mask or colsum) and odt == torch.float32 and wino_eligible(pc, H, W, x.dtype) and \
            (in_ab is None or Cin <= 512):
        return conv3x3_wino(x, pc, scale, bias, relu, gn_part, out, in_ab, in_relu, out_b8)
    assert not out_b8, 'channel-blocked output is produced by the Winograd layers only (check wino_eligible first)'
    if pc.dilation != 1:
        # dilated 3x3 (cpr_conv2d_fwd_dil): the direct fp32 kernel with scale / bias / residual / ReLU / mask / column sums, nothing else
        assert in_ab is None and not (in_relu or gn_part) and odt == torch.float32 and x.dtype == torch.float32, \
            'a dilated conv (dilation=%d) has no fused-input-affine, GroupNorm-statistics or bf16 form' % pc.dilation
        if out is None:
            out = torch.empty((N, OH, OW, pc.Cout), device=x.device, dtype=torch.float32)
        assert tuple(out.shape) == (N, OH, OW, pc.Cout) and out.is_contiguous()
        part = torch.empty(((N * OH * OW + 63) // 64, pc.Cout, 2), device=x.device, dtype=torch.float32) if colsum else None
        variant = ctypes.c_int(0) if (colsum or TRACE_CONV_VARIANT[0]) else None
        flags = (CONV_RELU if relu else 0) | (CONV_RES_MASK if res_mask else 0) | (CONV_COLSUM if colsum else 0)
        _lib.call('cpr_conv2d_fwd_dil', _ptr(x), _ptr(pc.w), _ptr(out), _ptr(scale), _ptr(bias), _ptr(residual), None, None, _ptr(part),
                  N, H, W, Cin, pc.Cout, pc.KH, pc.KW, pc.stride, pc.padding, pc.dilation, pc.Kpad, flags, 0,
                  ctypes.byref(variant) if variant is not None else None, _stream())
        if variant is not None:
            TRACE_CONV_VARIANT[1] = ('fp32_dil', variant.value)
        if colsum:
            bm = variant.value // 1000000
            return out, TilePartials(part, (N * OH * OW + bm - 1) // bm, pc.Cout)
        return out
    if out is None:
        out = torch.empty((N, OH, OW, pc.Cout), device=x.device, dtype=odt)
    part = None
    if gn_part:
        assert (OH * OW) % 128 == 0 and not colsum
        part = torch.empty((N * OH * OW // 128, pc.Cout, 2), device=x.device, dtype=torch.float32)
    if colsum and x.dtype != torch.bfloat16:
        part = torch.empty(((N * OH * OW + 63) // 64, pc.Cout, 2), device=x.device, dtype=torch.float32)
    variant = ctypes.c_int(0) if (colsum or TRACE_CONV_VARIANT[0]) else None   # [host] out-parameter of the launcher
    vref = ctypes.byref(variant) if variant is not None else None
    if x.dtype == torch.bfloat16:
        assert in_ab is None, 'the bf16 kernel does not fuse the producer GroupNorm (materialise with gn_apply)'
        if res_mask or colsum:
            # mask mode (round 6): data gradient + ReLU backward + column sums (+ the bf16 rounding: out_dtype) in one launch
            assert res_mask and colsum and residual is not None and residual.dtype == torch.bfloat16 and not relu and not gn_part
            slots = conv2d_bf16_mask_slots(x.shape, pc, odt)
            assert slots > 0, 'this shape has no mask-mode instance (ask conv2d_bf16_mask_slots first)'
            part = torch.empty((slots, pc.Cout, 2), device=x.device, dtype=torch.float32)
            _lib.call('cpr_conv2d_fwd_bf16', _ptr(x), _ptr(pc.w), _ptr(pc.frag_image()), _ptr(out), _ptr(scale), _ptr(bias), _ptr(residual),
                      _ptr(part), N, H, W, Cin, pc.Cout, pc.KH, pc.KW, pc.stride, pc.padding, pc.Kpad, 2,
                      int(odt == torch.float32), vref, _stream())
            if variant is not None:
                TRACE_CONV_VARIANT[1] = ('bf16', variant.value)
            return out, TilePartials(part, slots, pc.Cout)
        _lib.call('cpr_conv2d_fwd_bf16', _ptr(x), _ptr(pc.w), _ptr(pc.frag_image()), _ptr(out), _ptr(scale), _ptr(bias), _ptr(residual),
                  _ptr(part), N, H, W, Cin, pc.Cout, pc.KH, pc.KW, pc.stride, pc.padding, pc.Kpad, int(relu),
                  int(odt == torch.float32), vref, _stream())
        if variant is not None:
            TRACE_CONV_VARIANT[1] = ('bf16', variant.value)
        return (out, part) if gn_part else out
    a = b = None
    if in_ab is not None:
        a, b = in_ab
    flags = (CONV_RELU if relu else 0) | (CONV_OUT_BF16 if odt == torch.bfloat16 else 0) | \
        (CONV_RES_MASK if res_mask else 0) | (CONV_COLSUM if colsum else 0)
    _lib.call('cpr_conv2d_fwd', _ptr(x), _ptr(pc.w), _ptr(out), _ptr(scale), _ptr(bias),
              _ptr(residual), _ptr(a), _ptr(b), _ptr(part), N, H, W, Cin, pc.Cout, pc.KH, pc.KW, pc.stride,
              pc.padding, pc.Kpad, flags, int(in_relu), vref, _stream())
    if variant is not None:
        TRACE_CONV_VARIANT[1] = ('fp32', variant.value)
    if colsum:
        bm = variant.value // 1000000     # tile edge the launcher picked
        return out, TilePartials(part, (N * OH * OW + bm - 1) // bm, pc.Cout)
    return (out, part) if gn_part else out


def conv2d_bf16_mask_slots(x_shape, pc, out_dtype=torch.bfloat16, fused_add=False):
    """Column-sum slots a mask-mode launch (``conv2d(bf16 x, pc, residual=mask, res_mask=True, colsum=True)``) of this shape writes;
    0 = the shape's kernel does not know the mode (include/cpr_hip.h, cpr_conv2d_bf16_mask_slots).  fused_add: the form with the
    shortcut sum and two outputs (``conv2d_dgrad_bf16_fused``)."""
    N, H, W, Cin = x_shape
    if pc.groups > 1 or (fused_add and (not WFRAG[0] or pc.Cout % 256 != 0)):
        return 0
    return _lib.call('cpr_conv2d_bf16_mask_slots', N, H, W, Cin, pc.Cout, pc.KH, pc.KW, pc.stride, pc.padding,
                     2 if fused_add else int(out_dtype == torch.float32), positive=True)


def conv2d_dgrad_bf16_fused(g16, pc, mask, add):
    """The block-boundary data gradient of the mixed-precision backward in one launch (include/cpr_hip.h,
    cpr_conv2d_dgrad_bf16_fused): g = mask > 0 ? conv(g16, pc) + add : 0 -> (g fp32, g bf16, column-sum TilePartials).  g16 bf16
    (N,H,W,Cin), pc: the rotated, BN-scaled bf16 pack, mask: bf16 map of the output's shape, add: fp32 map of the output's shape."""
    _check(g16, ACT)
    pack_ready(pc)
    N, H, W, Cin = g16.shape
    OH, OW = pc.out_hw(H, W)
    shape = (N, OH, OW, pc.Cout)
    assert g16.dtype == torch.bfloat16 and pc.dtype == torch.bfloat16 and Cin == pc.Cin
    assert mask.dtype == torch.bfloat16 and add.dtype == torch.float32 and tuple(mask.shape) == shape and tuple(add.shape) == shape
    assert mask.is_contiguous() and add.is_contiguous()
    slots = conv2d_bf16_mask_slots(g16.shape, pc, fused_add=True)
    assert slots > 0, 'this shape has no fused instance (ask conv2d_bf16_mask_slots(..., fused_add=True) first)'
    out32 = torch.empty(shape, device=g16.device, dtype=torch.float32)
    out16 = torch.empty(shape, device=g16.device, dtype=torch.bfloat16)
    part = torch.empty((slots, pc.Cout, 2), device=g16.device, dtype=torch.float32)
    variant = ctypes.c_int(0) if TRACE_CONV_VARIANT[0] else None
    _lib.call('cpr_conv2d_dgrad_bf16_fused', _ptr(g16), _ptr(pc.w), _ptr(pc.frag_image()), _ptr(out32), _ptr(out16), _ptr(add), _ptr(mask),
              _ptr(part), N, H, W, Cin, pc.Cout, pc.KH, pc.KW, pc.stride, pc.padding, pc.Kpad,
              ctypes.byref(variant) if variant is not None else None, _stream())
    if variant is not None:
        TRACE_CONV_VARIANT[1] = ('bf16', variant.value)
    return out32, out16, TilePartials(part, slots, pc.Cout)


def conv1x1_stream(x, pc, scale=None, bias=None, residual=None, relu=False, res_mask=False):
    """The streamed 1x1 kernel (csrc/conv1x1_stream.hip) called explicitly -- ``conv2d`` takes it by itself for large launches;
    tests compare the two kernels bit for bit.  x (N, H, W, Cin) fp32, Cin in {64, 128, 256}."""
    N, H, W, Cin = x.shape
    assert pc.KH == 1 and pc.stride == 1 and pc.padding == 0 and pc.Kpad == Cin and x.dtype == torch.float32
    out = torch.empty((N, H, W, pc.Cout), device=x.device, dtype=torch.float32)
    flags = (CONV_RELU if relu else 0) | (CONV_RES_MASK if res_mask else 0)
    _lib.call('cpr_conv1x1_stream_fwd', _ptr(x), _ptr(pc.w), _ptr(out), _ptr(scale), _ptr(bias), _ptr(residual),
              N * H * W, Cin, pc.Cout, flags, _stream())
    return out


def conv2d_dual(x, pc, x2, pc2, scale=None, bias=None, scale2=None, bias2=None, relu=False, out=None):
    """relu?((conv(x, pc) * scale + bias) + (conv1x1(x2, pc2) * scale2 + bias2)) in one launch: conv3 + bn3 of a stage's first
    bottleneck together with its projection shortcut (resnet.py:262-302) -- the shortcut map never reaches HBM.  Bit-identical
    to ``conv2d(x, pc, scale, bias, residual=conv2d(x2, pc2, scale2, bias2), relu=relu)``.  fp32 NHWC; pc2 is 1x1, unpadded."""
    _check(x, ACT)
    _check(x2, ACT)
    pack_ready(pc)
    pack_ready(pc2)
    N, H, W, Cin = x.shape
    N2, H2, W2, Cin2 = x2.shape
    assert x.dtype == torch.float32 and x2.dtype == torch.float32 and pc.dtype == torch.float32 and pc2.dtype == torch.float32
    assert N == N2 and Cin == pc.Cin and Cin2 == pc2.Cin and pc.Cout == pc2.Cout and pc2.KH == 1 and pc2.KW == 1 and pc2.padding == 0
    OH, OW = pc.out_hw(H, W)
    assert (OH, OW) == pc2.out_hw(H2, W2), 'the two sources must produce the same output grid'
    if out is None:
        out = torch.empty((N, OH, OW, pc.Cout), device=x.device, dtype=torch.float32)
    variant = ctypes.c_int(0) if TRACE_CONV_VARIANT[0] else None
    _lib.call('cpr_conv2d_dual_fwd', _ptr(x), _ptr(pc.w), _ptr(x2), _ptr(pc2.w), _ptr(out), _ptr(scale), _ptr(bias),
              _ptr(scale2), _ptr(bias2), N, H, W, Cin, pc.Cout, pc.KH, pc.KW, pc.stride, pc.padding, pc.Kpad, H2, W2, Cin2,
              pc2.stride, pc2.Kpad, CONV_RELU if relu else 0, ctypes.byref(variant) if variant is not None else None, _stream())
    if variant is not None:
        TRACE_CONV_VARIANT[1] = ('fp32', variant.value)
    return out


class TilePartials:
    """Per-tile per-channel sums left by a conv epilogue; ``reduce()`` -> (C,) column sums on the CURRENT stream (the
    training step does it on its side stream, next to the only consumer, so the main chain never waits for it)."""

    def __init__(self, part, tiles, C):
        self.part, self.tiles, self.C = part, tiles, C

    def record_stream(self, stream):
        self.part.record_stream(stream)

    def reduce(self):
        cs = torch.empty((self.C,), device=self.part.device, dtype=torch.float32)
        ws = torch.empty((64 * self.C,), device=self.part.device, dtype=torch.float32)
        _lib.call('cpr_part_colsum', _ptr(self.part), _ptr(cs), _ptr(ws), self.tiles, self.C, _stream())
        return cs


def _sfx(x):
    return '_bf16' if x.dtype == torch.bfloat16 else ''


def bn_fold(gamma, beta, mean, var, eps, want_inv_sigma=False):
    """Eval-mode BatchNorm as a per-channel affine: (scale, shift[, inv_sigma])."""
    C = gamma.numel()
    dev = gamma.device
    scale = torch.empty((C,), device=dev, dtype=torch.float32)
    shift = torch.empty((C,), device=dev, dtype=torch.float32)
    inv = torch.empty((C,), device=dev, dtype=torch.float32) if want_inv_sigma else None
    _lib.call('cpr_bn_fold', _ptr(_check(gamma.detach())), _ptr(_check(beta.detach())), _ptr(_check(mean)), _ptr(_check(var)),
              float(eps), _ptr(scale), _ptr(shift), _ptr(inv), C, _stream())
    return scale, shift, inv


# ---- training-mode BatchNorm (batch statistics; ResNet norm_eval=False) -- csrc/bn_train.hip
def _bn_rows(y):
    C = y.shape[-1]
    M = y.numel() // C
    if M <= 1:
        # torch.nn.functional.batch_norm's refusal (_verify_batch_size)
        raise ValueError('Expected more than 1 value per channel when training, got input size %s' % (tuple(y.shape),))
    assert C % 64 == 0, 'training-mode BatchNorm needs C % 64 == 0, got %d' % C
    return M, C


def _bn_vec(t, C):
    """A per-channel (C,) operand of the bn_train.hip kernels (read with 16-byte loads): fp32, contiguous, exactly C long; None passes."""
    if t is None:
        return None
    t = _check(t.detach())
    assert t.numel() == C, 'per-channel vector of %d elements, want %d' % (t.numel(), C)
    return t


BnStats = collections.namedtuple('BnStats', 'mean rstd scale shift center cmean cshift')


def bn_batch_stats(y, gamma, beta, running_mean=None, running_var=None, num_batches_tracked=None, momentum=0.1, eps=1e-5, group=None):
    """Batch statistics of an NHWC fp32 map y (..., C) -> BnStats of (C,) vectors: mean, rstd = 1/sqrt(biased var + eps),
    scale = gamma*rstd, shift = beta - mean*scale, and the centred form the product path applies and differentiates with --
    center = the map's first row, cmean = mean - center, cshift = beta - cmean*scale: (y - center)*scale + cshift has an exact first
    difference, so a map whose mean is far above its spread normalises to the precision of its spread.  running_mean / running_var are updated in place as torch's training-mode
    BatchNorm does (unbiased variance; momentum None: 1 / num_batches_tracked), num_batches_tracked incremented -- on the device.
    The kernel writes the buffers through raw pointers: their version counters are bumped here so that anything keyed on them
    (layers._PackCache: the folded eval-mode BatchNorm) sees the change.
    group (SyncBN): a torch.distributed process group of more than one rank -> the statistics of the rows of ALL its ranks
    (bn_sync_local_stats -> all_gather_into_tensor of the fp64 record on the current stream -> bn_sync_merge_stats; a BnSyncStats).
    None, torch.distributed not initialised or a one-rank group: the single-rank launch below, untouched (torch's ``need_sync`` rule)."""
    if sync_world_size(group) > 1:
        rec, _ = bn_sync_local_stats(y)
        return bn_sync_merge_stats(_sync_gather(rec, group), y, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps)
    M, C = _bn_rows(_check(y))
    dev = y.device
    st = torch.empty((7, C), device=dev, dtype=torch.float32)
    ws = torch.empty((_lib.call('cpr_bn_train_ws', M, C, positive=True),), device=dev, dtype=torch.float32)
    if momentum is None:
        assert num_batches_tracked is not None, 'momentum None averages over num_batches_tracked'
    assert (running_mean is None) == (running_var is None), 'running_mean and running_var go together'
    bufs = [t for t in (running_mean, running_var) if t is not None]
    for t in bufs:
        _bn_vec(t, C)
    if num_batches_tracked is not None:
        assert _check(num_batches_tracked, torch.int64).numel() == 1
    _lib.call('cpr_bn_batch_stats', _ptr(y), _ptr(_bn_vec(gamma, C)), _ptr(_bn_vec(beta, C)), _ptr(running_mean),
              _ptr(running_var), _ptr(num_batches_tracked), -1.0 if momentum is None else float(momentum), float(eps),
              _ptr(st[0]), _ptr(st[1]), _ptr(st[2]), _ptr(st[3]), _ptr(st[4]), _ptr(st[5]), _ptr(st[6]), _ptr(ws), M, C, _stream())
    from torch.autograd.graph import increment_version
    for t in bufs + ([num_batches_tracked] if num_batches_tracked is not None else []):
        increment_version(t)
    return BnStats(*st.unbind(0))


def bn_apply(y, scale, shift, residual=None, relu=False, center=None, y2=None, scale2=None, shift2=None, center2=None, out=None):
    """out = [ReLU]((y - center)*scale + shift [+ residual]) (center None = 0), or the two-input form of a bottleneck with a projection
    shortcut: out = [ReLU]((y - center)*scale + shift + (y2 - center2)*scale2 + shift2) -- the shortcut is never materialised."""
    M, C = y.numel() // _check(y).shape[-1], y.shape[-1]
    for t in (residual, y2):
        if t is not None:
            assert _check(t).shape == y.shape, (t.shape, y.shape)
    assert residual is None or y2 is None
    assert y2 is not None or (scale2 is None and shift2 is None and center2 is None), 'scale2 / shift2 / center2 belong to y2'
    assert y2 is None or (scale2 is not None and shift2 is not None), 'the two-input form needs scale2 and shift2'
    if out is None:
        out = torch.empty_like(y)
    assert _check(out).shape == y.shape
    _lib.call('cpr_bn_apply', _ptr(y), _ptr(_bn_vec(center, C)), _ptr(_bn_vec(scale, C)), _ptr(_bn_vec(shift, C)), _ptr(residual),
              _ptr(y2), _ptr(_bn_vec(center2, C)), _ptr(_bn_vec(scale2, C)), _ptr(_bn_vec(shift2, C)), _ptr(out), M, C, int(relu),
              _stream())
    return out


def bn_train_bwd(dout, y, mean, rstd, gamma, mask=None, out_dgamma=None, out_dbeta=None, center=None, group=None, count=None):
    """Backward of training-mode BatchNorm (xhat = ((y - center) - mean)*rstd: pass BnStats' center and cmean for the centred form) (+ the ReLU whose output is ``mask``, when given: g = dout*(mask > 0), applied on the fly,
    never written) -> (dy, dgamma, dbeta): dbeta = sum g, dgamma = sum g*xhat, dy = gamma*rstd*(g - dbeta/M - xhat*dgamma/M).
    out_dgamma / out_dbeta: where the parameter gradients go (e.g. the trainer's gradient views); default fresh tensors.
    group (SyncBN, a group of more than one rank; ``count``: the forward's BnSyncStats.count): the sums behind dy run over the rows of
    all ranks (bn_sync_local_bwd -> all_gather_into_tensor -> bn_sync_merge_bwd); dgamma / dbeta stay THIS rank's local sums."""
    if sync_world_size(group) > 1:
        assert count is not None, 'the synchronised backward divides by the global row count of the forward (BnSyncStats.count)'
        rec, ws, dg, db = bn_sync_local_bwd(dout, y, mean, rstd, mask=mask, out_dgamma=out_dgamma, out_dbeta=out_dbeta, center=center)
        return bn_sync_merge_bwd(_sync_gather(rec, group), ws, count, dout, y, mean, rstd, gamma, mask=mask, center=center), dg, db
    M, C = _bn_rows(_check(y))
    assert _check(dout).shape == y.shape and (mask is None or _check(mask).shape == y.shape)
    dev = y.device
    dg = out_dgamma if out_dgamma is not None else torch.empty((C,), device=dev, dtype=torch.float32)
    db = out_dbeta if out_dbeta is not None else torch.empty((C,), device=dev, dtype=torch.float32)
    dy = torch.empty_like(y)
    ws = torch.empty((_lib.call('cpr_bn_train_ws', M, C, positive=True),), device=dev, dtype=torch.float32)
    _lib.call('cpr_bn_train_bwd', _ptr(dout), _ptr(mask), _ptr(y), _ptr(_bn_vec(center, C)), _ptr(_bn_vec(mean, C)), _ptr(_bn_vec(rstd, C)),
              _ptr(_bn_vec(gamma, C)), _ptr(dy), _ptr(_bn_vec(dg, C)), _ptr(_bn_vec(db, C)), _ptr(ws), M, C, _stream())
    return dy, dg, db


# ---- SyncBN: batch statistics over the rows of every rank of a process group (torch.nn.SyncBatchNorm).  The local / merge halves are
# public: one process can play R ranks by calling the local half on R chunks and stacking the records (tests/test_gpu_syncbn.py).
class BnSyncStats(BnStats):
    """BnStats of a synchronised BatchNorm.  mean, rstd, scale, shift are the same bits on every rank; center, cmean, cshift are
    rank-local (center = this rank's first row).  ``count``: (1,) fp64 device tensor, the global row count (the backward divides by it)."""
    count = None


def sync_world_size(group=None):
    """Ranks a BatchNorm synchronises over: 1 without a group or without an initialised torch.distributed (no synchronisation)."""
    if group is None:
        return 1
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 1
    return dist.get_world_size(group)


def _sync_gather(record, group):
    """(n,) fp64 record -> (R, n): every rank's record in rank order; issued in program order on the current stream."""
    import torch.distributed as dist
    R = dist.get_world_size(group)
    out = torch.empty((R * record.numel(),), device=record.device, dtype=record.dtype)
    dist.all_gather_into_tensor(out, record, group=group)
    return out.view(R, record.numel())


def _bn_sync_rows(y):
    C = y.shape[-1]
    M = y.numel() // C if C else 0
    if M < 1:
        raise ValueError('SyncBN: this rank holds no rows (input size %s): every rank of the group brings at least one value per channel'
                         % (tuple(y.shape),))
    assert C % 64 == 0, 'training-mode BatchNorm needs C % 64 == 0, got %d' % C
    return M, C


def _bn_sync_records(records, n, y):
    assert _check(records, torch.float64).dim() == 2 and records.shape[1] == n, (tuple(records.shape), n)
    assert records.device == y.device
    return int(records.shape[0])


def bn_sync_local_stats(y):
    """This rank's half of the synchronised statistics: NHWC fp32 map y (..., C), one row or more -> (record, workspace).  record:
    (2C + 1,) fp64 = [absolute per-channel mean | M2 | row count], what the ranks exchange; workspace: the row-block partials."""
    M, C = _bn_sync_rows(_check(y))
    rec = torch.empty((2 * C + 1,), device=y.device, dtype=torch.float64)
    ws = torch.empty((_lib.call('cpr_bn_sync_ws', M, C, positive=True),), device=y.device, dtype=torch.float32)
    _lib.call('cpr_bn_sync_stats_local', _ptr(y), _ptr(rec), _ptr(ws), M, C, _stream())
    return rec, ws


def bn_sync_merge_stats(records, y, gamma, beta, running_mean=None, running_var=None, num_batches_tracked=None, momentum=0.1, eps=1e-5):
    """records (R, 2C + 1): the gathered bn_sync_local_stats records, rank order; y: THIS rank's map -> BnSyncStats over the rows of all
    ranks, running buffers / num_batches_tracked updated as bn_batch_stats does (unbiased variance over the global count - 1).  More than
    one value per channel is needed over the whole group (torch's refusal), not per rank."""
    M, C = _bn_sync_rows(_check(y))
    R = _bn_sync_records(records, 2 * C + 1, y)
    if R == 1 and M <= 1:      # every rank brings >= 1 row (bn_sync_local_stats), so only a lone one-row rank can fall short
        raise ValueError('Expected more than 1 value per channel when training, got input size %s' % (tuple(y.shape),))
    dev = y.device
    st = torch.empty((7, C), device=dev, dtype=torch.float32)
    count = torch.empty((1,), device=dev, dtype=torch.float64)
    if momentum is None:
        assert num_batches_tracked is not None, 'momentum None averages over num_batches_tracked'
    assert (running_mean is None) == (running_var is None), 'running_mean and running_var go together'
    bufs = [t for t in (running_mean, running_var) if t is not None]
    for t in bufs:
        _bn_vec(t, C)
    if num_batches_tracked is not None:
        assert _check(num_batches_tracked, torch.int64).numel() == 1
    _lib.call('cpr_bn_sync_stats_merge', _ptr(records), R, _ptr(y), _ptr(_bn_vec(gamma, C)), _ptr(_bn_vec(beta, C)), _ptr(running_mean),
              _ptr(running_var), _ptr(num_batches_tracked), -1.0 if momentum is None else float(momentum), float(eps),
              _ptr(st[0]), _ptr(st[1]), _ptr(st[2]), _ptr(st[3]), _ptr(st[4]), _ptr(st[5]), _ptr(st[6]), _ptr(count), C, _stream())
    from torch.autograd.graph import increment_version
    for t in bufs + ([num_batches_tracked] if num_batches_tracked is not None else []):
        increment_version(t)
    out = BnSyncStats(*st.unbind(0))
    out.count = count
    return out


def bn_sync_local_bwd(dout, y, mean, rstd, mask=None, out_dgamma=None, out_dbeta=None, center=None):
    """This rank's half of the synchronised backward (mean / center as bn_train_bwd: BnSyncStats' cmean and center) ->
    (record, workspace, dgamma, dbeta): record (2C,) fp64 = [sum g | sum g*(y - mean)] over this rank's rows; dgamma / dbeta are this
    rank's LOCAL sums, as torch's SyncBatchNorm gives them (the gradient reducer averages them over the ranks)."""
    M, C = _bn_sync_rows(_check(y))
    assert _check(dout).shape == y.shape and (mask is None or _check(mask).shape == y.shape)
    dev = y.device
    dg = out_dgamma if out_dgamma is not None else torch.empty((C,), device=dev, dtype=torch.float32)
    db = out_dbeta if out_dbeta is not None else torch.empty((C,), device=dev, dtype=torch.float32)
    rec = torch.empty((2 * C,), device=dev, dtype=torch.float64)
    ws = torch.empty((_lib.call('cpr_bn_sync_ws', M, C, positive=True),), device=dev, dtype=torch.float32)
    _lib.call('cpr_bn_sync_bwd_local', _ptr(dout), _ptr(mask), _ptr(y), _ptr(_bn_vec(center, C)), _ptr(_bn_vec(mean, C)),
              _ptr(_bn_vec(rstd, C)), _ptr(_bn_vec(dg, C)), _ptr(_bn_vec(db, C)), _ptr(rec), _ptr(ws), M, C, _stream())
    return rec, ws, dg, db


def bn_sync_merge_bwd(records, workspace, count, dout, y, mean, rstd, gamma, mask=None, center=None):
    """records (R, 2C): the gathered bn_sync_local_bwd records, rank order; workspace: this rank's, from bn_sync_local_bwd; count: the
    forward's BnSyncStats.count -> dy of THIS rank's rows, dy = gamma*rstd*(g - sum g / count - xhat * sum g*xhat / count) with the
    sums over all ranks."""
    M, C = _bn_sync_rows(_check(y))
    R = _bn_sync_records(records, 2 * C, y)
    assert _check(dout).shape == y.shape and (mask is None or _check(mask).shape == y.shape)
    assert _check(count, torch.float64).numel() == 1
    assert _check(workspace).numel() == _lib.call('cpr_bn_sync_ws', M, C, positive=True), 'the workspace of bn_sync_local_bwd on this map'
    dy = torch.empty_like(y)
    _lib.call('cpr_bn_sync_bwd_merge', _ptr(records), R, _ptr(count), _ptr(dout), _ptr(mask), _ptr(y), _ptr(_bn_vec(center, C)),
              _ptr(_bn_vec(mean, C)), _ptr(_bn_vec(rstd, C)), _ptr(_bn_vec(gamma, C)), _ptr(dy), _ptr(workspace), M, C, _stream())
    return dy


def stem_weight_f32(weight):
    """(64, 3, 7, 7) conv1 weight -> the (64, 154) fp32 image of csrc/stem_f32.hip: [cout][kh][kw * 3 + c], slot 21 of every
    kernel row zero."""
    assert tuple(weight.shape) == (64, 3, 7, 7), tuple(weight.shape)
    w = torch.zeros((64, 7, 22), device=weight.device, dtype=torch.float32)
    w[:, :, :21] = weight.detach().float().permute(0, 2, 3, 1).reshape(64, 7, 21)
    return w.reshape(64, 154).contiguous()


def stem7x7s2_pool_f32(x, wpack, scale=None, bias=None, planar=None, record=False):
    """The whole ResNet stem in one kernel, exact fp32: x (N,H,W,4) NHWC4 or the (N,3,H,W) network input -> (N,PH,PW,64) =
    maxpool3x3s2(ReLU(conv7x7/2(x) * scale + bias)).  record: the recording instance -> (out, arg), arg (N,PH,PW,64) uint8 = the
    window position 0..8 of each maximum (first of ties), 255 where the pooled value is 0 (stem_pool_bwd's input)."""
    N, H, W, layout = _stem_input(_check(x), planar)
    assert wpack.dtype == torch.float32 and tuple(wpack.shape) == (64, 154)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((N, (OH - 1) // 2 + 1, (OW - 1) // 2 + 1, 64), device=x.device, dtype=torch.float32)
    if record:
        arg = torch.empty(tuple(out.shape), device=x.device, dtype=torch.uint8)
        _lib.call('cpr_stem7x7s2_pool_f32_rec', _ptr(x), _ptr(wpack), _ptr(scale), _ptr(bias), _ptr(out), _ptr(arg), N, H, W, layout,
                  _stream())
        return out, arg
    _lib.call('cpr_stem7x7s2_pool_f32', _ptr(x), _ptr(wpack), _ptr(scale), _ptr(bias), _ptr(out), N, H, W, layout, _stream())
    return out


def stem_weight_bf16(weight):
    """(64, 3, 7, 7) conv1 weight -> the (64, 224) bf16 image of csrc/stem_bf16.hip: k = (kh * 8 + kw) * 4 + c, zero at kw = 7
    and c = 3."""
    assert tuple(weight.shape) == (64, 3, 7, 7), tuple(weight.shape)
    w = torch.zeros((64, 7, 8, 4), device=weight.device, dtype=torch.float32)
    w[:, :, :7, :3] = weight.detach().float().permute(0, 2, 3, 1)
    return w.reshape(64, 224).to(torch.bfloat16).contiguous()


def _stem_input(x, planar=None):
    """(N, H, W, layout) of a stem input: NHWC4 (N,H,W,4) -> layout 0, the NCHW network input (N,3,H,W) -> layout 1.
    planar: say which one it is (a (N,3,W,4) tensor reads both ways); None = by shape, NHWC4 first."""
    assert x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous()
    if planar is None:
        planar = x.shape[-1] != 4
    if not planar:
        assert x.shape[-1] == 4, tuple(x.shape)
        return x.shape[0], x.shape[1], x.shape[2], 0
    assert x.shape[1] == 3, tuple(x.shape)
    return x.shape[0], x.shape[2], x.shape[3], 1


def stem_bf16_fits(x, planar=None):
    N, H, W, _ = _stem_input(x, planar)
    return N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * 64 * 2 < (1 << 31)


def stem7x7s2_bf16(x, wpack, scale=None, bias=None, relu=True, planar=None):
    """ResNet stem of the bf16 compute mode: x (N,H,W,4) fp32 NHWC4 or (N,3,H,W) fp32 -> (N,OH,OW,64) bf16 =
    ReLU(conv7x7/2(x) * scale + bias)."""
    N, H, W, layout = _stem_input(_check(x), planar)
    assert wpack.dtype == torch.bfloat16 and tuple(wpack.shape) == (64, 224)
    out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64), device=x.device, dtype=torch.bfloat16)
    _lib.call('cpr_stem7x7s2_bf16', _ptr(x), _ptr(wpack), _ptr(scale), _ptr(bias), _ptr(out), N, H, W, int(relu), layout, _stream())
    return out


def stem7x7s2_pool_bf16(x, wpack, scale=None, bias=None, planar=None, record=False):
    """stem7x7s2_bf16 (with ReLU) + maxpool3x3s2 in one kernel: x (N,H,W,4) or (N,3,H,W) fp32 -> (N,PH,PW,64) bf16; same bits as
    the pair.  record: -> (out, arg), the argmax byte map of the bf16 values (see stem7x7s2_pool_f32)."""
    N, H, W, layout = _stem_input(_check(x), planar)
    assert wpack.dtype == torch.bfloat16 and tuple(wpack.shape) == (64, 224)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((N, (OH - 1) // 2 + 1, (OW - 1) // 2 + 1, 64), device=x.device, dtype=torch.bfloat16)
    if record:
        arg = torch.empty(tuple(out.shape), device=x.device, dtype=torch.uint8)
        _lib.call('cpr_stem7x7s2_pool_bf16_rec', _ptr(x), _ptr(wpack), _ptr(scale), _ptr(bias), _ptr(out), _ptr(arg), N, H, W, layout,
                  _stream())
        return out, arg
    _lib.call('cpr_stem7x7s2_pool_bf16', _ptr(x), _ptr(wpack), _ptr(scale), _ptr(bias), _ptr(out), N, H, W, layout, _stream())
    return out


def maxpool3x3s2(x, record=False):
    """record: -> (out, arg), arg (N,PH,PW,C) uint8 = the window position 0..8 of each maximum (first of ties, out-of-map positions
    never win), 255 where the maximum is 0 -- x is a ReLU output there (the stem)."""
    N, H, W, C = _check(x, ACT).shape
    out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), device=x.device, dtype=x.dtype)
    if record:
        arg = torch.empty(tuple(out.shape), device=x.device, dtype=torch.uint8)
        _lib.call('cpr_maxpool3x3s2' + _sfx(x) + '_rec', _ptr(x), _ptr(out), _ptr(arg), N, H, W, C, _stream())
        return out, arg
    _lib.call('cpr_maxpool3x3s2' + _sfx(x), _ptr(x), _ptr(out), N, H, W, C, _stream())
    return out


def stem_deep(x, packs, folds, planar=None, out_dtype=torch.float32):
    """The deep stem (ResNetV1d) in exact fp32 on the matrix cores (csrc/stem_deep.hip): x (N,H,W,4) NHWC4 or the (N,3,H,W) network
    input -> (N,PH,PW,64) = maxpool3x3s2(the three conv3x3 + folded BN + ReLU layers).  packs: the fp32 PackedConv of the 3 -> 32 / 2,
    32 -> 32 and 32 -> 64 convs; folds: their (scale, shift).  out_dtype bf16 (the bf16 compute mode): the same fp32 chain, the pooled
    map rounded once.  Both input forms give the same bits."""
    N, H, W, layout = _stem_input(_check(x), planar)
    p1, p2, p3 = packs
    for pc, shape in zip(packs, ((32, 4, 64, 2), (32, 32, 288, 1), (64, 32, 288, 1))):
        assert pc.dtype == torch.float32 and (pc.Cout, pc.Cin, pc.Kpad, pc.stride) == shape and (pc.KH, pc.KW, pc.padding) == (3, 3, 1), \
            'deep stem: conv3x3 3 -> 32 / 2, 32 -> 32, 32 -> 64, padding 1'
        pack_ready(pc)
    assert out_dtype in ACT
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    mid1 = torch.empty((N, OH, OW, 32), device=x.device, dtype=torch.float32)
    mid2 = torch.empty_like(mid1)
    out = torch.empty((N, (OH - 1) // 2 + 1, (OW - 1) // 2 + 1, 64), device=x.device, dtype=out_dtype)
    (s1, b1), (s2, b2), (s3, b3) = folds
    _lib.call('cpr_stem_deep_fwd', _ptr(x), _ptr(p1.w), _ptr(_check(s1)), _ptr(_check(b1)), _ptr(p2.w), _ptr(_check(s2)), _ptr(_check(b2)),
              _ptr(p3.w), _ptr(_check(s3)), _ptr(_check(b3)), _ptr(mid1), _ptr(mid2), _ptr(out), N, H, W, layout,
              int(out_dtype == torch.bfloat16), _stream())
    return out


def stem3x3s2(x, pc, scale, bias, planar=None):
    """The RegNet stem (conv 3x3 / 2 / pad 1, 3 -> 32, + folded BatchNorm + ReLU, no max-pool): the deep stem's first launch alone
    (csrc/stem_deep.hip), exact fp32 on the matrix cores.  x (N,H,W,4) NHWC4 or the (N,3,H,W) network input -> (N,OH,OW,32) fp32; both
    input forms give the same bits.  pc: the conv's fp32 PackedConv."""
    N, H, W, layout = _stem_input(_check(x), planar)
    assert pc.dtype == torch.float32 and (pc.Cout, pc.Cin, pc.Kpad, pc.stride) == (32, 4, 64, 2) and (pc.KH, pc.KW, pc.padding) == (3, 3, 1), \
        'stem3x3s2: conv3x3 3 -> 32 / stride 2 / padding 1'
    pack_ready(pc)
    out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 32), device=x.device, dtype=torch.float32)
    _lib.call('cpr_stem3x3s2_fwd', _ptr(x), _ptr(pc.w), _ptr(_check(scale)), _ptr(_check(bias)), _ptr(out), N, H, W, layout, _stream())
    return out


def stem3x3s2_wgrad(dy, x, planar=None, out=None):
    """Weight gradient of that conv: dy (N,OH,OW,32) fp32 and the stem's input as the forward read it -> (32,3,3,3) fp32 (written into
    ``out`` when given); the split over pixels is added up in a fixed order (csrc/stem3x3_bwd.hip)."""
    N, H, W, layout = _stem_input(_check(x), planar)
    assert _check(dy).shape == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 32), (tuple(dy.shape), tuple(x.shape))
    if out is None:
        out = torch.empty((32, 3, 3, 3), device=x.device, dtype=torch.float32)
    assert _check(out).shape == (32, 3, 3, 3), tuple(out.shape)
    ws = torch.empty((_lib.call('cpr_stem3x3s2_wgrad_workspace', N, H, W, positive=True),), device=x.device, dtype=torch.float32)
    _lib.call('cpr_stem3x3s2_wgrad', _ptr(dy), _ptr(x), _ptr(out), _ptr(ws), N, H, W, layout, _stream())
    return out


def avgpool(x, s):
    """nn.AvgPool2d(s, s, ceil_mode=True, count_include_pad=False) on an NHWC fp32 / bf16 map (the avg_down shortcut): a last window
    of an odd map divides by its in-map elements; fp32 accumulation in a fixed order."""
    N, H, W, C = _check(x, ACT).shape
    assert s >= 2 and C % (8 if x.dtype == torch.bfloat16 else 4) == 0, (s, C)
    out = torch.empty((N, -(-H // s), -(-W // s), C), device=x.device, dtype=x.dtype)
    _lib.call('cpr_avgpool_fwd', _ptr(x), _ptr(out), N, H, W, C, s, int(x.dtype == torch.bfloat16), _stream())
    return out


def avgpool_bwd(g, in_hw, s, add=None):
    """Backward of avgpool in gather form: g (N,ceil(H/s),ceil(W/s),C) -> dx (N,H,W,C) = g[h/s, w/s] / count (+ add: another gradient
    of the pooled map's input, summed in the same pass -- the same bits as avgpool_bwd followed by axpby)."""
    N, OH, OW, C = _check(g, ACT).shape
    H, W = in_hw
    assert s >= 2 and (OH, OW) == (-(-H // s), -(-W // s)) and C % (8 if g.dtype == torch.bfloat16 else 4) == 0, (tuple(g.shape), in_hw, s)
    dx = torch.empty((N, H, W, C), device=g.device, dtype=g.dtype)
    if add is not None:
        assert _check(add, g.dtype).shape == dx.shape, (tuple(add.shape), tuple(dx.shape))
    _lib.call('cpr_avgpool_bwd', _ptr(g), _ptr(add), _ptr(dx), N, H, W, C, s, int(g.dtype == torch.bfloat16), _stream())
    return dx


def stem_pool_bwd(dp, arg, conv_hw):
    """Backward of the stem's max-pool 3x3/2/1 and the ReLU before it: dp (N,PH,PW,64) fp32 (the pooled map's gradient) and the
    recorded arg map (uint8, same shape) -> (dy (N,OH,OW,64) fp32 = the gradient at the BatchNorm output, TilePartials of its column
    sums).  conv_hw = (OH, OW), the conv map's size.  Each conv pixel sums the windows that chose it in a fixed order (pooled row,
    then pooled column, ascending); exact zeros where none did."""
    N, PH, PW, C = _check(dp).shape
    OH, OW = conv_hw
    assert C == 64 and (PH, PW) == ((OH - 1) // 2 + 1, (OW - 1) // 2 + 1), (tuple(dp.shape), conv_hw)
    assert _check(arg, torch.uint8).shape == dp.shape, (tuple(arg.shape), tuple(dp.shape))
    M = N * OH * OW
    tiles = _lib.call('cpr_stem_pool_bwd_blocks', M, positive=True)
    dy = torch.empty((N, OH, OW, 64), device=dp.device, dtype=torch.float32)
    part = torch.empty((tiles, 64, 2), device=dp.device, dtype=torch.float32)
    _lib.call('cpr_stem_pool_bwd', _ptr(dp), _ptr(arg), _ptr(dy), _ptr(part), N, OH, OW, _stream())
    return dy, TilePartials(part, tiles, 64)


def stem_wgrad_f32(dy, x, planar=None, out=None):
    """Weight gradient of the stem conv (7x7, stride 2, pad 3, 3 -> 64): dy (N,OH,OW,64) fp32 and the stem's input as the forward
    read it -- NHWC4 (N,H,W,4) or the (N,3,H,W) planes -> (64,3,7,7) fp32 (written into ``out`` when given), exact fp32 on the matrix
    pipe, the split-K partials summed in a fixed order."""
    N, H, W, layout = _stem_input(_check(x), planar)
    assert _check(dy).shape == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64), (tuple(dy.shape), tuple(x.shape))
    if out is None:
        out = torch.empty((64, 3, 7, 7), device=x.device, dtype=torch.float32)
    assert _check(out).shape == (64, 3, 7, 7), tuple(out.shape)
    ws = torch.empty((_lib.call('cpr_stem_wgrad_f32_workspace', N, H, W, positive=True),), device=x.device, dtype=torch.float32)
    _lib.call('cpr_stem_wgrad_f32', _ptr(dy), _ptr(x), _ptr(out), _ptr(ws), N, H, W, layout, _stream())
    return out


def gn_stats(x, slots=None):
    """Per (image, slot, channel) (sum, sumsq) partials of an NHWC tensor."""
    N, H, W, C = _check(x, ACT).shape
    HW = H * W
    if slots is None:
        slots = max(1, min(256, HW // 256))
    part = torch.empty((N * slots, C, 2), device=x.device, dtype=torch.float32)
    _lib.call('cpr_gn_stats' + _sfx(x), _ptr(x), _ptr(part), N, HW, C, slots, _stream())
    return part


def gn_finalize(part, gamma, beta, N, HW, groups=32, eps=1e-5, want_stats=False):
    """partials -> per (image, channel) affine (a, b) with y = x*a + b == GroupNorm(x)."""
    C = part.shape[1]
    P = part.shape[0] // N
    a = torch.empty((N, C), device=part.device, dtype=torch.float32)
    b = torch.empty((N, C), device=part.device, dtype=torch.float32)
    mean = rstd = None
    if want_stats:
        mean = torch.empty((N, groups), device=part.device, dtype=torch.float32)
        rstd = torch.empty((N, groups), device=part.device, dtype=torch.float32)
    _lib.call('cpr_gn_finalize', _ptr(part), _ptr(_check(gamma)), _ptr(_check(beta)), _ptr(a), _ptr(b), _ptr(mean),
              _ptr(rstd), N, P, C, groups, HW, float(eps), _stream())
    return (a, b, mean, rstd) if want_stats else (a, b)


def gn_apply(x, a, b, relu=False, up=None, out=None):
    """y = x*a[n,c] + b[n,c] (ReLU) (+ nearest-upsampled ``up``).  In place when out is x."""
    N, H, W, C = _check(x, ACT).shape
    if out is None:
        out = torch.empty_like(x)
    UH = UW = 0
    if up is not None:
        assert up.dtype == x.dtype
        UH, UW = up.shape[1], up.shape[2]
    _lib.call('cpr_gn_apply' + _sfx(x), _ptr(x), _ptr(a), _ptr(b), _ptr(up), _ptr(out), N, H, W, C, UH, UW, int(relu),
              _stream())
    return out


def gn_apply2(x1, a1, b1, x2, a2, b2, out=None):
    """y = (x1*a1[n,c] + b1[n,c]) + (x2*a2[n,c] + b2[n,c]): two raw conv outputs under their pending GroupNorm affines, summed in one
    pass (the PAFPN bottom-up path).  In place when out is x1 (or x2)."""
    N, H, W, C = _check(x1, ACT).shape
    assert _check(x2, ACT).shape == x1.shape and x2.dtype == x1.dtype, (x1.shape, x2.shape, x1.dtype, x2.dtype)
    assert tuple(a1.shape) == tuple(b1.shape) == tuple(a2.shape) == tuple(b2.shape) == (N, C)
    if out is None:
        out = torch.empty_like(x1)
    _lib.call('cpr_gn_apply2' + _sfx(x1), _ptr(x1), _ptr(_check(a1)), _ptr(_check(b1)), _ptr(x2), _ptr(_check(a2)), _ptr(_check(b2)),
              _ptr(out), N, H, W, C, _stream())
    return out


# ------------------------------------------------------------------------------------------------ BFP neck (csrc/bfp.hip)
class _BfpLevel(ctypes.Structure):      # include/cpr_hip.h: cpr_bfp_level
    _fields_ = [('x', ctypes.c_void_p), ('a', ctypes.c_void_p), ('b', ctypes.c_void_p), ('y', ctypes.c_void_p), ('arg', ctypes.c_void_p),
                ('H', ctypes.c_int), ('W', ctypes.c_int), ('sy', ctypes.c_float), ('sx', ctypes.c_float)]


BFP_MAX_LEVELS = 8


def nearest_scale(n_in, n_out):
    """The scale of torch's nearest resize of an axis from n_in to n_out cells: ONE fp32 division, formed here on the host.
    src = min(int(floorf(float(dst) * scale)), n_in - 1) -- ``nearest_index`` -- is torch's index for every dtype."""
    import numpy as np
    return float(np.float32(n_in) / np.float32(n_out))


def nearest_index(n_in, n_out):
    """The source index of every destination cell of a nearest resize, as the kernels compute it (numpy float32)."""
    import numpy as np
    src = np.floor(np.arange(n_out, dtype=np.float32) * np.float32(nearest_scale(n_in, n_out))).astype(np.int64)
    return np.minimum(src, n_in - 1)


def adaptive_windows(n_in, n_out):
    """[(start, end)] of the n_out windows of adaptive pooling over an axis of n_in cells: [floor(i*in/out), ceil((i+1)*in/out))."""
    return [((i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)) for i in range(n_out)]


def _bfp_arg_dtype(pairs):
    """The code width of the recorded argmax for the pooled axes ``pairs`` = [(n_in, n_out)]: uint8 while no window side exceeds 16."""
    widest = max([e - s for n_in, n_out in pairs for s, e in adaptive_windows(n_in, n_out)] + [1])
    if widest > 256:
        raise _lib.CprHipError('BFP: an adaptive-pooling window of %d cells cannot be recorded (256 at most)' % widest)
    return torch.uint8 if widest <= 16 else torch.int16


def _bfp_split(levels):
    """levels: per level a materialised NHWC map, or (raw map, (a, b)) -> maps, [(a, b) | (None, None)]."""
    maps, abs_ = [], []
    for lv in levels:
        x, ab = (lv, (None, None)) if torch.is_tensor(lv) else (lv[0], tuple(lv[1]))
        maps.append(x), abs_.append(ab)
    N, _, _, C = _check(maps[0], ACT).shape
    for x, (a, b) in zip(maps, abs_):
        assert _check(x, ACT).dtype == maps[0].dtype and x.shape[0] == N and x.shape[3] == C, (x.shape, maps[0].shape)
        assert (a is None) == (b is None) and (a is None or tuple(_check(a).shape) == tuple(_check(b).shape) == (N, C))
    assert 1 <= len(maps) <= BFP_MAX_LEVELS, 'BFP takes 1 .. %d levels' % BFP_MAX_LEVELS
    return maps, abs_


def _bfp_table(rows):
    t = (_BfpLevel * len(rows))()
    for e, (x, a, b, y, arg, H, W, sy, sx) in zip(t, rows):
        e.x, e.a, e.b = x.data_ptr(), (a.data_ptr() if a is not None else None), (b.data_ptr() if b is not None else None)
        e.y, e.arg = (y.data_ptr() if y is not None else None), (arg.data_ptr() if arg is not None else None)
        e.H, e.W, e.sy, e.sx = H, W, sy, sx
    return t


def bfp_gather(levels, refine_level, record=False):
    """BFP step 1 (bfp.py:73-85): bsf (N, h, w, C) = mean over the levels of adaptive_max_pool2d (levels finer than refine_level) /
    nearest (the others) to level refine_level's size, one launch.  levels: materialised NHWC maps or (raw, (a, b)) pairs.
    record: also the argmax of every window -> (bsf, [arg | None per level])."""
    maps, abs_ = _bfp_split(levels)
    r = int(refine_level)
    N, h, w, C = maps[r].shape
    dt = _bfp_arg_dtype([p for x in maps[:r] for p in ((x.shape[1], h), (x.shape[2], w))]) if record else torch.uint8
    args = [torch.empty((N, h, w, C), device=maps[0].device, dtype=dt) if record and i < r else None for i in range(len(maps))]
    bsf = torch.empty((N, h, w, C), device=maps[0].device, dtype=maps[0].dtype)
    rows = [(x, a, b, None, g, x.shape[1], x.shape[2], nearest_scale(x.shape[1], h), nearest_scale(x.shape[2], w))
            for x, (a, b), g in zip(maps, abs_, args)]
    _lib.call('cpr_bfp_gather' + _sfx(bsf), _bfp_table(rows), len(maps), r, _ptr(bsf), N, C, int(dt != torch.uint8), _stream())
    return (bsf, args) if record else bsf


def bfp_scatter(levels, refine_level, ref, ref_ab=None, record=False):
    """BFP step 3 (bfp.py:91-99): out_i = residual_i + level_i for every level, one launch; residual_i = nearest(ref) for the levels finer
    than refine_level, adaptive_max_pool2d(ref) for the others.  ref (N, h, w, C): the refined map, materialised, or with ref_ab = (a, b)
    the refine conv's raw output under its GroupNorm affine AND ReLU, applied on load.  -> outs [, args with record]."""
    maps, abs_ = _bfp_split(levels)
    r = int(refine_level)
    N, h, w, C = maps[r].shape
    assert tuple(_check(ref, ACT).shape) == (N, h, w, C) and ref.dtype == maps[0].dtype, (ref.shape, ref.dtype)
    ra, rb = (None, None) if ref_ab is None else ref_ab
    assert ra is None or tuple(_check(ra).shape) == tuple(_check(rb).shape) == (N, C)
    dt = _bfp_arg_dtype([p for x in maps[r + 1:] for p in ((h, x.shape[1]), (w, x.shape[2]))]) if record else torch.uint8
    args = [torch.empty(x.shape, device=x.device, dtype=dt) if record and i > r else None for i, x in enumerate(maps)]
    outs = [torch.empty_like(x) for x in maps]
    rows = [(x, a, b, y, g, x.shape[1], x.shape[2], nearest_scale(h, x.shape[1]), nearest_scale(w, x.shape[2]))
            for x, (a, b), y, g in zip(maps, abs_, outs, args)]
    _lib.call('cpr_bfp_scatter' + _sfx(ref), _bfp_table(rows), len(maps), r, _ptr(ref), _ptr(ra), _ptr(rb), N, C,
              int(dt != torch.uint8), _stream())
    return (outs, args) if record else outs


def bfp_scatter_bwd(gs, refine_level, args):
    """d(refined map) = the sum over the levels, ascending, of g_i through nearest / max-pool backward (gather form, no atomics).
    gs: fp32 gradients of the scatter's outputs; args: its record."""
    r = int(refine_level)
    N, h, w, C = _check(gs[r]).shape
    wide = [a.dtype != torch.uint8 for a in args if a is not None]
    rows = [(_check(g), None, None, None, a, g.shape[1], g.shape[2], nearest_scale(h, g.shape[1]), nearest_scale(w, g.shape[2]))
            for g, a in zip(gs, args)]
    d_ref = torch.empty((N, h, w, C), device=gs[r].device, dtype=torch.float32)
    _lib.call('cpr_bfp_scatter_bwd', _bfp_table(rows), len(gs), r, _ptr(d_ref), N, C, int(any(wide)), _stream())
    return d_ref


def bfp_gather_bwd(gs, refine_level, d_bsf, args):
    """d_level_i = g_i + (d_bsf / L through max-pool / nearest backward) for every level, one launch.  gs: what reaches the levels
    directly (the scatter's residual connection); args: the gather's record."""
    r = int(refine_level)
    N, h, w, C = _check(d_bsf).shape
    assert tuple(gs[r].shape) == (N, h, w, C)
    wide = [a.dtype != torch.uint8 for a in args if a is not None]
    outs = [torch.empty_like(_check(g)) for g in gs]
    rows = [(g, None, None, y, a, g.shape[1], g.shape[2], nearest_scale(g.shape[1], h), nearest_scale(g.shape[2], w))
            for g, y, a in zip(gs, outs, args)]
    _lib.call('cpr_bfp_gather_bwd', _bfp_table(rows), len(gs), r, _ptr(d_bsf), N, C, int(any(wide)), _stream())
    return outs


# ------------------------------------------------------------------------------------------------ HRFPN neck (csrc/hrfpn.hip)
class _HrfpnLevel(ctypes.Structure):    # include/cpr_hip.h: cpr_hrfpn_level
    _fields_ = [('p', ctypes.c_void_p), ('H', ctypes.c_int), ('W', ctypes.c_int)]


HRFPN_MAX_LEVELS, HRFPN_MAX_OUTS = 4, 5


def _hrfpn_table(maps):
    t = (_HrfpnLevel * max(1, len(maps)))()
    for e, m in zip(t, maps):
        e.p, e.H, e.W = m.data_ptr(), m.shape[1], m.shape[2]
    return t


def _hrfpn_maps(maps, dtype):
    """The common checks of a level table: NHWC, one dtype, one batch, one channel count.  Sizes are the kernels' own argument check."""
    N, _, _, C = _check(maps[0], dtype).shape
    for m in maps:
        assert _check(m, dtype).dtype == maps[0].dtype and m.dim() == 4 and m.shape[0] == N and m.shape[3] == C, (m.shape, maps[0].shape)
    return N, C


def hrfpn_fuse(ys, bias=None):
    """out = bias + ys[0] + sum_{i>=1} bilinear_i(ys[i]): the HRFPN reduction conv behind its per-level 1x1 convs (csrc/hrfpn.hip).
    ys: 1..4 NHWC maps, fp32 or bf16, level i at (H0 >> i, W0 >> i) with H_i * 2^i == H0 (anything else is refused by the kernel's
    argument check); bilinear_i: F.interpolate(scale_factor=2**i, mode='bilinear', align_corners=False).  bias (C,) fp32 or None."""
    N, C = _hrfpn_maps(ys, ACT)
    if bias is not None:
        assert _check(bias.detach()).numel() == C, (bias.shape, C)
    out = torch.empty_like(ys[0])
    _lib.call('cpr_hrfpn_fuse' + _sfx(out), _hrfpn_table(ys), len(ys), _ptr(bias), _ptr(out), N, C, _stream())
    return out


def hrfpn_pool(out, num_outs):
    """-> [F.avg_pool2d(out, 2**k, 2**k) for k in 1 .. num_outs - 1] of an NHWC fp32 / bf16 map in one launch: floor mode (H0 // 2**k,
    trailing rows and columns dropped), every level from ``out`` itself.  An empty level is refused by the kernel's argument check."""
    N, H0, W0, C = _check(out, ACT).shape
    if num_outs <= 1:
        return []
    levels = [torch.empty((N, H0 >> k, W0 >> k, C), device=out.device, dtype=out.dtype) for k in range(1, num_outs)]
    _lib.call('cpr_hrfpn_pool' + _sfx(out), _ptr(out), H0, W0, _hrfpn_table(levels), len(levels), N, C, _stream())
    return levels


def hrfpn_pool_bwd(gs):
    """gs: the fp32 gradients g_0 .. g_{K-1} of hrfpn_pool's input and outputs (g_k at (H0 >> k, W0 >> k)) ->
    (d_out = g_0 + sum_k g_k[y >> k, x >> k] / 4**k inside level k's floor region, TilePartials of d_out's column sums)."""
    N, C = _hrfpn_maps(gs, torch.float32)
    _, H0, W0, _ = gs[0].shape
    d_out = torch.empty_like(gs[0])
    tiles = _lib.call('cpr_hrfpn_pool_bwd_blocks', N, H0, W0, positive=True)
    part = torch.empty((tiles, C, 2), device=d_out.device, dtype=torch.float32)
    _lib.call('cpr_hrfpn_pool_bwd', _hrfpn_table(gs), len(gs), _ptr(d_out), _ptr(part), N, C, _stream())
    return d_out, TilePartials(part, tiles, C)


def hrfpn_fuse_bwd(d_out, sizes):
    """The adjoint of hrfpn_fuse's bilinear part: d_out (N, H0, W0, C) fp32 -> [dy_1, ..] with dy_i (N,) + sizes[i - 1] + (C,) (dy_0 is
    d_out itself).  sizes: the (H_i, W_i) of levels 1 ..; H_i * 2^i != H0 is refused by the kernel's argument check."""
    N, H0, W0, C = _check(d_out).shape
    if not sizes:
        return []
    dys = [torch.empty((N, int(h), int(w), C), device=d_out.device, dtype=torch.float32) for h, w in sizes]
    _lib.call('cpr_hrfpn_fuse_bwd', _ptr(d_out), H0, W0, _hrfpn_table(dys), len(dys), N, C, _stream())
    return dys


# ------------------------------------------------------------------------------------------------ HRNet branch exchange (csrc/hrnet.hip)
class _HrnetTerm(ctypes.Structure):    # include/cpr_hip.h: cpr_hrnet_term
    _fields_ = [('p', ctypes.c_void_p), ('k', ctypes.c_int)]


HRNET_MAX_TERMS, HRNET_MAX_K = 4, 3


def hrnet_fuse(terms, size, out=None):
    """out (N, H, W, C) = ReLU(t_0 + t_1 + ..): the exchange step of HRModule.forward for one output branch (csrc/hrnet.hip).
    terms: [(map, k)], map an NHWC fp32 tensor (N, H >> k, W >> k, C) read at [y >> k, x >> k] (nearest upsampling by 2**k; k = 0: a
    map at the output's size), in the reference's order -- source branch ascending; the fp32 sum runs left to right.  size: (H, W).
    The term count and the divisibility of (H, W) by 2**k are the kernel's own argument check.  out: written when given."""
    H, W = int(size[0]), int(size[1])
    N, C = terms[0][0].shape[0], terms[0][0].shape[3]
    for m, k in terms:
        assert _check(m).dim() == 4 and 0 <= int(k) <= HRNET_MAX_K and tuple(m.shape) == (N, H >> int(k), W >> int(k), C), \
            (tuple(m.shape), k, (N, H, W, C))
    t = (_HrnetTerm * max(1, len(terms)))()
    for e, (m, k) in zip(t, terms):
        e.p, e.k = m.data_ptr(), int(k)
    if out is None:
        out = torch.empty((N, H, W, C), device=terms[0][0].device, dtype=torch.float32)
    assert tuple(_check(out).shape) == (N, H, W, C)
    _lib.call('cpr_hrnet_fuse', t, len(terms), _ptr(out), N, H, W, C, _stream())
    return out


def hrnet_fuse_bwd(dy, y, K, out=None):
    """The adjoint of hrnet_fuse at its output: dy, y (N, H, W, C) fp32, y the recorded output -> (g, pools, TilePartials) with
    g = y <= 0 ? +0.0 : dy, pools[k - 1] (N, H >> k, W >> k, C) = the sum of g over 2**k x 2**k blocks for k = 1..K (the gradient of
    a term that was upsampled by 2**k; 2x2 blocks in row-major order, then 2x2 of those), and the per-block column sums of g -- the
    bias gradient of every folded BN that fed this branch.  out: (g, pools, partials tensor (blocks, C, 2)) written when given."""
    N, H, W, C = _check(dy).shape
    assert tuple(_check(y).shape) == (N, H, W, C) and dy.dim() == 4
    K = int(K)
    tiles = _lib.call('cpr_hrnet_fuse_bwd_blocks', N, H, W, C, K, positive=True)
    if out is None:
        g = torch.empty_like(dy)
        pools = [torch.empty((N, H >> k, W >> k, C), device=dy.device, dtype=torch.float32) for k in range(1, K + 1)]
        part = torch.empty((tiles, C, 2), device=dy.device, dtype=torch.float32)
    else:
        g, pools, part = out
        assert tuple(_check(g).shape) == (N, H, W, C) and tuple(_check(part).shape) == (tiles, C, 2) and len(pools) == K and \
            all(tuple(_check(p).shape) == (N, H >> k, W >> k, C) for k, p in enumerate(pools, 1))
    table = (ctypes.c_void_p * max(1, K))(*[p.data_ptr() for p in pools])
    _lib.call('cpr_hrnet_fuse_bwd', _ptr(dy), _ptr(y), _ptr(g), table, K, _ptr(part), N, H, W, C, _stream())
    return g, pools, TilePartials(part, tiles, C)


# ------------------------------------------------------------------------------------------------ CPR points
def box_centers(boxes):
    n = boxes.shape[0]
    out = torch.empty((n, 2), device=boxes.device, dtype=torch.float32)
    _lib.call('cpr_box_centers', _ptr(_check(boxes)), _ptr(out), n, _stream())
    return out


def logit_project(x, w, bias, in_ab=None, in_relu=True):
    """x (N,H,W,Cin) fp32, w (J,Cin), bias (J) -> (N,H,W,J): the streaming projection kernel (J <= 8, Cin in {64, 128,
    192, 256}); returns None when the shape is outside what it covers (the caller uses the MFMA conv)."""
    N, H, W, Cin = _check(x).shape
    J = w.shape[0]
    if J > 8 or Cin > 256 or Cin % 64:
        return None
    out = torch.empty((N, H, W, J), device=x.device, dtype=torch.float32)
    a, b = in_ab if in_ab is not None else (None, None)
    _lib.call('cpr_logit_project', _ptr(x), _ptr(_check(w)), _ptr(_check(bias)), _ptr(a), _ptr(b), _ptr(out), N, H * W, Cin, J,
              int(in_relu), _stream())
    return out


def p2p_out_bf16_supported(x_shape, J):
    """Whether the bf16 output-conv kernels (csrc/p2p_out_bf16.hip) cover a map of this shape with J output channels."""
    return len(x_shape) == 4 and 1 <= J <= 8 and x_shape[3] in (64, 128, 192, 256)


def _p2p_out_args(x, ab, w):
    _check(x, torch.bfloat16)
    N, H, W, Cin = x.shape
    J = w.shape[0]
    assert tuple(w.shape) == (J, Cin, 3, 3), (tuple(w.shape), Cin)
    a, b = ab
    assert tuple(_check(a).shape) == (N, Cin) and tuple(_check(b).shape) == (N, Cin), (a.shape, b.shape)
    return N, H, W, Cin, J


def p2p_out_bf16(x, ab, w, bias):
    """P2PHead output conv on the bf16 map: x (N,H,W,Cin) RAW bf16 last tower layer, ab = its GroupNorm affine (a, b) (N,Cin), read as
    relu(a*x + b); w (J,Cin,3,3), bias (J) fp32 -> (N,H,W,J) fp32.  None when the shape is outside the kernel (p2p_out_bf16_supported)."""
    if not p2p_out_bf16_supported(x.shape, w.shape[0]):
        return None
    N, H, W, Cin, J = _p2p_out_args(x, ab, w)
    assert tuple(_check(bias).shape) == (J,)
    taps = torch.empty((N, H, W, 9 * J), device=x.device, dtype=torch.float32)
    out = torch.empty((N, H, W, J), device=x.device, dtype=torch.float32)
    _lib.call('cpr_p2p_out_bf16_fwd', _ptr(x), _ptr(ab[0]), _ptr(ab[1]), _ptr(_check(w)), _ptr(bias), _ptr(taps), _ptr(out),
              N, H, W, Cin, J, _stream())
    return out


def _dout_rows(dout, N, H, W, J):
    """dout (N,H,W,Jd >= J) fp32: the first J channels are read (a channel-padded gradient map as it is)."""
    assert dout.dtype == torch.float32 and dout.is_cuda and dout.is_contiguous() and tuple(dout.shape[:3]) == (N, H, W) \
        and dout.shape[3] >= J, (tuple(dout.shape), (N, H, W, J))
    return dout.shape[3]


def p2p_out_bf16_dgrad(dout, w, x_shape, out_dtype=torch.float32):
    """Data gradient of the output conv wrt its ACTIVATED input: dout (N,H,W,Jd) fp32 (first J = w.shape[0] channels live), w
    (J,Cin,3,3) -> (N,H,W,Cin) fp32, or bf16 (each element the round-to-nearest-even of the fp32 result).  None when unsupported."""
    J = w.shape[0]
    if not p2p_out_bf16_supported(x_shape, J):
        return None
    N, H, W, Cin = x_shape
    assert tuple(_check(w).shape) == (J, Cin, 3, 3) and out_dtype in ACT
    ldd = _dout_rows(dout, N, H, W, J)
    dx = torch.empty((N, H, W, Cin), device=dout.device, dtype=out_dtype)
    _lib.call('cpr_p2p_out_bf16_dgrad', _ptr(dout), ldd, _ptr(w), _ptr(dx), int(out_dtype == torch.bfloat16), N, H, W, Cin, J,
              _stream())
    return dx


def p2p_out_bf16_wgrad(dout, x, ab, weight_shape, out_w=None, out_b=None):
    """Weight and bias gradients of the output conv: dout (N,H,W,Jd) fp32 (first J live), x / ab as in p2p_out_bf16 -> (gw (J,Cin,3,3),
    gb (J)), written into out_w / out_b when given (e.g. a trainer's gradient views).  Fixed-order reduction: bit-repeatable.
    None when unsupported."""
    J = weight_shape[0]
    if not p2p_out_bf16_supported(x.shape, J):
        return None
    N, H, W, Cin, _ = _p2p_out_args(x, ab, torch.empty(tuple(weight_shape), device='meta'))
    ldd = _dout_rows(dout, N, H, W, J)
    gw = out_w if out_w is not None else torch.empty(tuple(weight_shape), device=x.device, dtype=torch.float32)
    gb = out_b if out_b is not None else torch.empty((J,), device=x.device, dtype=torch.float32)
    assert tuple(_check(gw).shape) == (J, Cin, 3, 3) and tuple(_check(gb).shape) == (J,)
    ws = torch.empty((_lib.call('cpr_p2p_out_bf16_wgrad_ws', N, H, W, Cin, J, positive=True),), device=x.device,
                     dtype=torch.float32)
    _lib.call('cpr_p2p_out_bf16_wgrad', _ptr(x), _ptr(ab[0]), _ptr(ab[1]), _ptr(dout), ldd, _ptr(gw), _ptr(gb), _ptr(ws), N, H, W,
              Cin, J, _stream())
    return gw, gb


PROB_TYPES = {'sigmoid': 0, 'softmax': 1, 'normed_sigmoid': 2, 'identity': 3}


def neg_mask_loss(logit_map, centers, labels, gt_start, pad_hw, num_classes, stride, d2_thr, eps=1e-6,
                  class_wise=True, prob_type='sigmoid', norm_p=1.0, mask_classes=None):
    """logit_map (N,H,W,J) -> mask (N*H*W, C) uint8, partial sums (double).  centers/labels/gt_start: the annotated
    points in CSR form (with num_refine > 1: every refine point, carrying its gt's label).  mask_classes=1 with
    num_classes=2: out_bg_cls, the single class's validity covers the [class, background] outputs."""
    N, H, W, J = _check(logit_map).shape
    C = num_classes
    mask = torch.empty((N * H * W, C), device=logit_map.device, dtype=torch.uint8)
    nblk = (H * W * C + 255) // 256
    partial = torch.empty((N * nblk,), device=logit_map.device, dtype=torch.float64)
    _lib.call('cpr_neg_mask_loss', _ptr(logit_map), J, _ptr(centers), _ptr(labels), _ptr(gt_start), _ptr(pad_hw),
              _ptr(mask), _ptr(partial), N, H, W, C, float(stride), float(d2_thr), float(eps), int(class_wise),
              PROB_TYPES[prob_type], float(norm_p), C if mask_classes is None else int(mask_classes), None, _stream())
    return mask, partial


def bag_sample(fmap, centers, gt_img, pad_hw, offsets, stride, align_corners=False, pad_value=None):
    """fmap (N,H,W,J); one bag per row of centers; returns pts (G,K,2), valid (G,K) uint8, sampled (G,K,J).
    align_corners: the generators' align_corners=True sampling (zeros padding); pad_value (J,): contribution of a dropped tap per
    unit of weight (the projection's bias when fmap is the logit map)."""
    N, H, W, J = _check(fmap).shape
    G = centers.shape[0]
    K = (offsets.shape[0] if offsets is not None else 0) + 1
    pts = torch.empty((G, K, 2), device=fmap.device, dtype=torch.float32)
    valid = torch.empty((G, K), device=fmap.device, dtype=torch.uint8)
    out = torch.empty((G, K, J), device=fmap.device, dtype=torch.float32)
    _lib.call('cpr_bag_sample', _ptr(fmap), J, _ptr(centers), _ptr(gt_img), _ptr(pad_hw), _ptr(offsets), _ptr(pts),
              _ptr(valid), _ptr(out), G, K, H, W, float(stride), int(align_corners), _ptr(pad_value), _stream())
    return pts, valid, out


def grid_bag(fmap, points, gt_img, num_refine, max_pos_num, radius_px, stride, pad_value=None, align_corners=False,
             want_cell=False):
    """GridCirclesPtFeatGenerator bags: fmap (N,H,W,J), points (G*R,2), gt_img (G) -> pts (G,Kmax+R,2),
    valid (G,Kmax+R) uint8, sampled (G,Kmax+R,J), count (G) int32 (grid points found per gt).  pad_value (J,): what the
    padding slots hold (default zeros).  want_cell: also the entry codes (G,Kmax+R) int32 -- cell index | -1 padding slot |
    <= -2 refine point (bilinear sample) -- which ``bag_points_gather_bwd`` walks."""
    N, H, W, J = _check(fmap).shape
    R = int(num_refine)
    G = points.shape[0] // R
    Kt = int(max_pos_num) + R
    dev = fmap.device
    pts = torch.empty((G, Kt, 2), device=dev, dtype=torch.float32)
    valid = torch.empty((G, Kt), device=dev, dtype=torch.uint8)
    cell = torch.empty((G, Kt), device=dev, dtype=torch.int32)
    count = torch.empty((G,), device=dev, dtype=torch.int32)
    out = torch.empty((G, Kt, J), device=dev, dtype=torch.float32)
    assert pad_value is None or pad_value.numel() == J
    _lib.call('cpr_grid_bag', _ptr(fmap), J, _ptr(_check(points)), _ptr(gt_img), R, int(max_pos_num), float(radius_px),
              _ptr(pad_value), _ptr(pts), _ptr(valid), _ptr(cell), _ptr(count), _ptr(out), G, H, W, float(stride),
              int(align_corners), _stream())
    return (pts, valid, out, count, cell) if want_cell else (pts, valid, out, count)


def mil_loss(logits, ins_off, valid, labels, num_classes, neg_partial, w_mil, w_gt, w_neg, gt_weight=None, eps=1e-6,
             bags=None, centres=None, prob_type='sigmoid', norm_p=1.0, binary_ins=False, allpos=False,
             neg_from_gt=False):
    """logits (G,K,J) [entries = G*K rows], valid (G,K).  bags = (num_bags, stride, off, len) in entries (default: one bag
    per row of the (G,K) layout); centres = (off, stride, count, mod): the annotated-point loss entries of a bag (default:
    the last entry of every bag).  labels / gt_weight are per bag.
    -> (5,) tensor {gt_loss, pos_loss, bag_acc, neg_loss, num_sample} and the per-bag workspace (num_bags,5)."""
    G, K, J = _check(logits).shape
    nb, bstride, boff, blen = bags if bags is not None else (G, K, 0, K)
    coff, cstride, ccount, cmod = centres if centres is not None else (K - 1, K, 1, 1)
    assert labels.numel() == nb and (gt_weight is None or gt_weight.numel() == nb)
    assert (nb - 1) * bstride + boff + blen <= G * K
    bag = torch.empty((nb, 5), device=logits.device, dtype=torch.float32)
    out = torch.empty((5,), device=logits.device, dtype=torch.float32)
    npart = 0 if neg_partial is None else neg_partial.numel()
    _lib.call('cpr_mil_loss', _ptr(logits), J, ins_off, _ptr(valid), _ptr(labels), _ptr(gt_weight), _ptr(bag),
              _ptr(neg_partial), npart, nb, bstride, boff, blen, coff, cstride, ccount, cmod, num_classes, float(eps),
              PROB_TYPES[prob_type], float(norm_p), int(binary_ins), int(allpos), float(w_mil), float(w_gt),
              float(w_neg), int(neg_from_gt), _ptr(out), _stream())
    return out, bag


def refine(logits, pts, valid, centers, labels, gt_img, gt_start, img_hw, num_classes, gt_alpha, merge_th, refine_th,
           use_nearest=True, use_classify=False, not_refine_in=None, sub_bags=1, ctr_stride=None, prob_type='sigmoid',
           norm_p=1.0, score_max=False):
    """logits (G,Kt,J): a gt owns Kt = sub_bags*Kv entries; centers holds ctr_stride points per gt (default sub_bags)."""
    G, Kt, J = _check(logits).shape
    Rv = int(sub_bags)
    assert Kt % Rv == 0
    ctr_stride = Rv if ctr_stride is None else int(ctr_stride)
    assert centers.shape[0] == G * ctr_stride
    dev = logits.device
    rp = torch.empty((G, 2), device=dev, dtype=torch.float32)
    sc = torch.empty((G,), device=dev, dtype=torch.float32)
    nr = torch.empty((G,), device=dev, dtype=torch.uint8)
    chosen = torch.empty((G, Kt), device=dev, dtype=torch.uint8)
    _lib.call('cpr_refine', _ptr(logits), J, _ptr(pts), _ptr(valid), _ptr(centers), Rv, ctr_stride, _ptr(labels),
              _ptr(gt_img), _ptr(gt_start), _ptr(img_hw), _ptr(not_refine_in), _ptr(rp), _ptr(sc), _ptr(nr),
              _ptr(chosen), G, Kt, Kt // Rv, num_classes, PROB_TYPES[prob_type], float(norm_p), float(gt_alpha),
              float(merge_th), float(refine_th), int(use_nearest), int(use_classify), int(score_max), _stream())
    return rp, sc, nr, chosen


# ------------------------------------------------------------------------------------------------ assigners
def point_assign(points, gt_bboxes, scale=4, pos_num=3):
    n, k = points.shape[0], gt_bboxes.shape[0]
    dev = points.device
    inds = torch.zeros((n,), device=dev, dtype=torch.int64)
    if n == 0 or k == 0:
        return inds
    best = torch.empty((n,), device=dev, dtype=torch.float32)
    lvl = torch.empty((n,), device=dev, dtype=torch.int32)
    _lib.call('cpr_point_assign', _ptr(_check(points)), _ptr(_check(gt_bboxes)), n, k, float(scale), pos_num,
              _ptr(inds), _ptr(best), _ptr(lvl), _stream())
    return inds


def hungarian_cost(pred, logits, gt, labels, w_cls=2.0, alpha=0.25, gamma=2.0, eps=1e-12, w_dis=0.1, fx=1.0,
                   fy=1.0, p=1):
    """-> cost^T (G, M) fp32 (column-major view of the reference's (M, G) cost)."""
    M, G = pred.shape[0], gt.shape[0]
    costT = torch.empty((G, M), device=pred.device, dtype=torch.float32)
    _lib.call('cpr_hungarian_cost', _ptr(_check(pred)), pred.shape[1], _ptr(_check(logits)), logits.shape[1],
              _ptr(_check(gt)), _ptr(labels), _ptr(costT), M, G, float(w_cls), float(alpha), float(gamma),
              float(eps), float(w_dis), float(fx), float(fy), int(p), _stream())
    return costT


LSA_REGISTER_KERNEL = [True]     # test hook: False keeps the memory-resident kernel (the two must agree bit for bit)


def lsa_topk(costT_list, topk):
    """Solve a batch of independent assignment problems (one workgroup each).  costT_list: list of (G_b, M_b)
    fp32 tensors with M_b >= G_b.  Returns list of gt_inds (M_b,) int64 (0 = background, j+1 = gt j)."""
    dev = costT_list[0].device
    Ms = [c.shape[1] for c in costT_list]
    Gs = [c.shape[0] for c in costT_list]
    nb = len(costT_list)
    flat = torch.cat([c.reshape(-1) for c in costT_list]) if nb > 1 else costT_list[0].reshape(-1)
    cost_off, col_off, row_off = [0], [0], [0]
    for m, g in zip(Ms, Gs):
        cost_off.append(cost_off[-1] + m * g)
        col_off.append(col_off[-1] + m)
        row_off.append(row_off[-1] + g)
    # index tables: keep them alive in locals until after the launch (a temporary would be freed -- and its block
    # recycled by the caching allocator -- before the kernel reads it)
    t_m = torch.tensor(Ms, dtype=torch.int32, device=dev)
    t_g = torch.tensor(Gs, dtype=torch.int32, device=dev)
    t_off = torch.tensor([cost_off[:-1], col_off[:-1], row_off[:-1]], dtype=torch.int64, device=dev)
    tm, tg = col_off[-1], max(row_off[-1], 1)
    gt_inds = torch.zeros((tm,), device=dev, dtype=torch.int64)
    ws_v = torch.empty((tm,), device=dev, dtype=torch.float64)
    ws_spc = torch.empty((tm,), device=dev, dtype=torch.float64)
    ws_path = torch.empty((tm,), device=dev, dtype=torch.int32)
    ws_r4c = torch.empty((tm,), device=dev, dtype=torch.int32)
    ws_sc = torch.empty((tm,), device=dev, dtype=torch.uint8)
    ws_act = torch.empty((tm,), device=dev, dtype=torch.uint8)
    ws_cols = torch.empty((3, tm), device=dev, dtype=torch.int32)   # cols / remaining / pos
    ws_u = torch.empty((tg,), device=dev, dtype=torch.float64)
    ws_c4r = torch.empty((tg,), device=dev, dtype=torch.int32)
    ws_sr = torch.empty((tg,), device=dev, dtype=torch.uint8)
    status = torch.zeros((nb,), device=dev, dtype=torch.int32)
    _lib.call('cpr_lsa_topk', _ptr(flat), _ptr(t_m), _ptr(t_g), _ptr(t_off[0]), _ptr(t_off[1]), _ptr(t_off[2]), nb,
              int(topk), _ptr(gt_inds), _ptr(ws_v), _ptr(ws_spc),
              _ptr(ws_path), _ptr(ws_r4c), _ptr(ws_sc), _ptr(ws_act), _ptr(ws_cols[0]), _ptr(ws_cols[1]),
              _ptr(ws_cols[2]), _ptr(ws_u), _ptr(ws_c4r), _ptr(ws_sr), _ptr(status),
              max(Ms) if LSA_REGISTER_KERNEL[0] else 0, max(Gs), _stream())
    return [gt_inds[col_off[i]:col_off[i + 1]] for i in range(nb)], status


# ------------------------------------------------------------------------------------------------ P2P inference
def topk_desc(scores, k):
    """k largest of a 1-D fp32 tensor, sorted descending, ties by lower index (+0.0 and -0.0 are a tie; the values keep their
    input bits).  -> (values, indices int64)"""
    n = _check(scores).numel()
    vals = torch.empty((k,), device=scores.device, dtype=torch.float32)
    idx = torch.empty((k,), device=scores.device, dtype=torch.int64)
    _lib.call('cpr_topk_desc', _ptr(scores), n, int(k), _ptr(vals), _ptr(idx), _stream())
    return vals, idx


def nms_candidates(boxes, scores, score_thr, factors=None):
    """(proposal, class) pairs above score_thr in row-major order.  boxes (n,4) or (n,4C), scores (n,C+1) (last column =
    background).  -> cand_boxes (k,4), cand_scores (k), cand_labels (k) int32, cand_inds (k) int64.
    One host read of k (the list is variable-length in the reference too)."""
    n, C = scores.shape[0], scores.shape[1] - 1
    dev = scores.device
    cap = max(n * C, 1)
    cb = torch.empty((cap, 4), device=dev, dtype=torch.float32)
    cs = torch.empty((cap,), device=dev, dtype=torch.float32)
    cl = torch.empty((cap,), device=dev, dtype=torch.int32)
    ci = torch.empty((cap,), device=dev, dtype=torch.int64)
    cnt = torch.zeros((1,), device=dev, dtype=torch.int32)
    _lib.call('cpr_nms_candidates', _ptr(_check(boxes)), boxes.shape[1], _ptr(_check(scores)), _ptr(factors), n, C,
              float(score_thr), _ptr(cb), _ptr(cs), _ptr(cl), _ptr(ci), _ptr(cnt), _stream())
    k = int(cnt.item())
    return cb[:k], cs[:k], cl[:k], ci[:k]


def nms(boxes, scores, labels, iou_thr):
    """Class-aware greedy NMS (batched_nms semantics).  -> keep indices (int64, descending score).
    One host read of the keep count (the reference's NMS output is variable-length too)."""
    n = boxes.shape[0]
    dev = boxes.device
    if n == 0:
        return torch.zeros((0,), device=dev, dtype=torch.int64)
    keep = torch.empty((n,), device=dev, dtype=torch.int64)
    num = torch.zeros((1,), device=dev, dtype=torch.int32)
    order = torch.empty((n,), device=dev, dtype=torch.int32)
    sboxes = torch.empty((n, 4), device=dev, dtype=torch.float32)
    # (sort workspace, then the pair mask -- whole for n <= 8192, else one band of 8192 rows + the carried removed bits)
    mask = torch.empty((_lib.call('cpr_nms_workspace', n, positive=True),), device=dev, dtype=torch.int64)
    _lib.call('cpr_nms', _ptr(_check(boxes)), _ptr(_check(scores)), _ptr(_check(labels, torch.int32)), n,
              float(iou_thr), _ptr(keep), _ptr(num), _ptr(order), _ptr(sboxes), _ptr(mask), _stream())
    return keep[:int(num.item())]


def topk_desc_batched(scores, k):
    """scores (B, n) fp32 -> (values (B, k), indices (B, k) int64): the k largest of every row, sorted descending, ties by
    lower index -- one launch for the batch."""
    B, n = _check(scores).shape
    vals = torch.empty((B, k), device=scores.device, dtype=torch.float32)
    idx = torch.empty((B, k), device=scores.device, dtype=torch.int64)
    _lib.call('cpr_topk_desc_batched', _ptr(scores), B, n, int(k), _ptr(vals), _ptr(idx), _stream())
    return vals, idx


def nms_candidates_batched(boxes, scores, score_thr, factors=None):
    """boxes (B, n, 4) or (B, n, 4C), scores (B, n, C+1) -> per-image slabs of capacity n * C: cand_boxes (B, cap, 4),
    cand_scores (B, cap), cand_labels (B, cap) int32, cand_inds (B, cap) int64 and count (B) int32 ON THE DEVICE (no host read)."""
    B, n, C = scores.shape[0], scores.shape[1], scores.shape[2] - 1
    dev = scores.device
    cap = max(n * C, 1)
    cb = torch.empty((B, cap, 4), device=dev, dtype=torch.float32)
    cs = torch.empty((B, cap), device=dev, dtype=torch.float32)
    cl = torch.empty((B, cap), device=dev, dtype=torch.int32)
    ci = torch.empty((B, cap), device=dev, dtype=torch.int64)
    cnt = torch.zeros((B,), device=dev, dtype=torch.int32)
    if n * C > 0:
        _lib.call('cpr_nms_candidates_batched', _ptr(_check(boxes)), boxes.shape[2], _ptr(_check(scores)), _ptr(factors), B, n, C,
                  float(score_thr), _ptr(cb), _ptr(cs), _ptr(cl), _ptr(ci), _ptr(cnt), _stream())
    return cb, cs, cl, ci, cnt


def nms_batched(boxes, scores, labels, counts, iou_thr):
    """Class-aware greedy NMS of B candidate slabs (nms_candidates_batched outputs): the candidate counts are read on the device.
    -> keep (B, cap) int64 slab-relative indices in descending score order, num_keep (B) int32 on the device."""
    B, cap = scores.shape
    dev = scores.device
    keep = torch.empty((B, cap), device=dev, dtype=torch.int64)
    num = torch.zeros((B,), device=dev, dtype=torch.int32)
    nblk = (cap + 63) // 64
    P = 1
    while P < cap:
        P <<= 1
    stride = max(cap * nblk, P)
    order = torch.empty((B, cap), device=dev, dtype=torch.int32)
    sboxes = torch.empty((B, cap, 4), device=dev, dtype=torch.float32)
    mask = torch.empty((B * stride,), device=dev, dtype=torch.int64)
    _lib.call('cpr_nms_batched', _ptr(_check(boxes)), _ptr(_check(scores)), _ptr(_check(labels, torch.int32)),
              _ptr(_check(counts, torch.int32)), B, cap, float(iou_thr), _ptr(keep), _ptr(num), _ptr(order), _ptr(sboxes),
              _ptr(mask), stride, _stream())
    return keep, num


def tap_sum3x3(R, bias, J):
    """R (N,H,W,9J) tap responses -> (N,H,W,J) = bias + the nine shifted responses (see csrc/postproc.hip tap_sum3x3_kernel)."""
    N, H, W, J9 = _check(R).shape
    assert J9 == 9 * J
    out = torch.empty((N, H, W, J), device=R.device, dtype=torch.float32)
    _lib.call('cpr_tap_sum3x3', _ptr(R), _ptr(bias), _ptr(out), N, H, W, J, _stream())
    return out


def p2p_decode(reg_nhwc, point_anchor, stride, gamma, want_anchor=False):
    """reg (N,H,W,2k) -> pred (N, H*W*k, 3) = (x, y, stride) [, anchor pts]."""
    N, H, W, C2 = _check(reg_nhwc).shape
    k = C2 // 2
    pred = torch.empty((N, H * W * k, 3), device=reg_nhwc.device, dtype=torch.float32)
    anchor = torch.empty_like(pred) if want_anchor else None
    _lib.call('cpr_p2p_decode', _ptr(reg_nhwc), _ptr(_check(point_anchor)), _ptr(pred), _ptr(anchor), N, H, W, k,
              float(stride), float(gamma), _stream())
    return (pred, anchor) if want_anchor else pred


def sigmoid_exact(x):
    """Elementwise sigmoid with torch's CPU bits (the scores that order top-k / NMS candidates)."""
    x = _check(x.contiguous())
    y = torch.empty_like(x)
    _lib.call('cpr_sigmoid', _ptr(x), _ptr(y), x.numel(), _stream())
    return y


def rowmax_sigmoid(logits):
    M, C = _check(logits).shape
    out = torch.empty((M,), device=logits.device, dtype=torch.float32)
    _lib.call('cpr_rowmax_sigmoid', _ptr(logits), _ptr(out), M, C, _stream())
    return out


P2P_CLS_MODES = {'FocalLoss': 0, 'CrossEntropyLoss_sigmoid': 1, 'CrossEntropyLoss': 2}
P2P_REG_MODES = {'SmoothL1Loss': 0, 'MSELoss': 1, 'L1Loss': 2}


def p2p_loss(logits, pred, gt_inds, gt_pts, gt_labels, gt_start, alpha, gamma, beta, pos_w, neg_w, reg_norm, w_cls,
             w_reg, cls_mode=0, reg_mode=0):
    """logits (B,M,C), pred (B,M,3), gt_inds (B,M) int64 -> (B,2) {loss_cls, loss_pts} per image.  cls_mode / reg_mode:
    P2P_CLS_MODES / P2P_REG_MODES (include/cpr_hip.h, cpr_p2p_loss)."""
    B, M, C = _check(logits).shape
    nblk = (M + 255) // 256
    ws = torch.empty((B * nblk * 3,), device=logits.device, dtype=torch.float64)
    out = torch.empty((B, 2), device=logits.device, dtype=torch.float32)
    _lib.call('cpr_p2p_loss', _ptr(logits), _ptr(_check(pred)), _ptr(_check(gt_inds, torch.int64)), _ptr(_check(gt_pts)),
              _ptr(_check(gt_labels, torch.int32)), _ptr(_check(gt_start, torch.int32)), _ptr(ws), _ptr(out), B, M, C,
              float(alpha), float(gamma), float(beta), float(pos_w), float(neg_w), float(reg_norm), float(w_cls),
              float(w_reg), int(cls_mode), int(reg_mode), _stream())
    return out


def match_cost(pred, logits, gt, labels, cls_terms, reg_terms):
    """The general cost matrix of the Hungarian assigners (csrc/assign.hip, match_cost_kernel) -> cost^T (G, M).  pred (M, 2) points or
    (M, 4) xyxy boxes, gt alike; cls_terms / reg_terms: lists of (type, weight, a, b, c, d) (include/cpr_hip.h, cpr_match_cost)."""
    import ctypes
    M, G = pred.shape[0], gt.shape[0]
    assert pred.shape[1] == gt.shape[1] and pred.shape[1] in (2, 4) and len(cls_terms) <= 4 and len(reg_terms) <= 4
    costT = torch.empty((G, M), device=pred.device, dtype=torch.float32)
    flat = [float(v) for t in list(cls_terms) + list(reg_terms) for v in (tuple(t) + (0.,) * 6)[:6]]
    terms = (ctypes.c_float * max(len(flat), 1))(*flat)
    _lib.call('cpr_match_cost', _ptr(_check(pred)), pred.shape[1], _ptr(_check(logits)), logits.shape[1], _ptr(_check(gt)),
              _ptr(_check(labels, torch.int32)), _ptr(costT), M, G, terms, len(cls_terms), len(reg_terms), _stream())
    return costT


# ------------------------------------------------------------------------------------------------ backward / optimizer
def dgrad_pack(weight, stride, padding, scale=None, dtype=torch.float32, groups=1, pitch=None, dilation=1):
    """PackedConv that computes the data gradient of ``conv2d(x, weight, stride, padding)`` as a stride-1 forward conv
    over dy (zero-inserted first when stride > 1): channels swapped, taps flipped, padding K-1-p; ``scale`` (Cout,) is
    the forward conv's folded-BatchNorm scale, multiplied into the weights.  Stride-2 convs with k in {1, 3} and
    padding k//2 (every strided conv of the ResNet body) get the phase-decomposed form (PhasedDgrad).  groups > 1 (a grouped 3x3 layer):
    the grouped data-gradient pack at either stride -- conv2d_dgrad zero-inserts a strided layer's gradient; ``pitch``: the channel pitch
    of its gradient maps (PackedConv).  dilation > 1 (stride 1, 3x3, padding == dilation; fp32): the same dilated conv over dy with the
    flipped pack and padding 2 d - d = d -- never the Winograd route (wino_eligible)."""
    dilation = int(dilation)
    if dilation != 1:
        assert stride == 1 and padding == dilation, \
            'dilation=%d: the data gradient is built for stride 1 and padding == dilation, got stride %d padding %d' % (dilation, stride, padding)
        if dtype != torch.float32:
            raise NotImplementedError('dilation=%d: a dilated convolution runs in the fp32 compute mode only, not in %s' % (dilation, dtype))
    if groups > 1:
        if dtype != torch.float32:
            raise NotImplementedError('a grouped convolution (groups=%d) runs in the fp32 compute mode only, not in %s' % (groups, dtype))
        assert padding == dilation and stride in (1, 2)
        return PackedConv.for_dgrad_grouped(weight, groups, scale, pitch, dilation)
    assert pitch is None
    if dilation != 1:
        return PackedConv.for_dgrad(weight, padding, scale, dilation=dilation)
    if stride == 2 and weight.shape[2] == weight.shape[3] and weight.shape[2] in (1, 3) and padding == weight.shape[2] // 2 \
            and _PHASED[0]:
        return PhasedDgrad(weight, stride, padding, scale, dtype)
    assert dtype == torch.float32, 'bf16: PackedConv.for_dgrad_bf16 (stride 1) or the phase-decomposed form (stride 2)'
    return PackedConv.for_dgrad(weight, padding, scale)


_PHASED = [True]     # test hook: False forces the zero-insertion form for strided convs


class PhasedDgrad:
    """Data gradient of a stride-2 conv (k in {1, 3}, padding k//2) without zero insertion: one stride-1 sub-convolution
    over dy per output-parity class (py, px) using only the taps that can reach that class (1+2+2+4 = 9 of the 9 taps
    instead of 4 x 9 over a dilated gradient), scattered to the strided positions."""

    def __init__(self, weight, stride, padding, scale=None, dtype=torch.float32):
        Cout, Cin, KH, KW = weight.shape
        assert stride == 2 and KH == KW and KH in (1, 3) and padding == KH // 2 and weight.is_cuda
        self.Cin, self.stride, self.classes, self.dtype = Cin, stride, [], dtype      # bf16 (round 6): the sub-convolutions on the bf16 pipe, fp32 out
        for py in range(2):
            khs = [kh for kh in range(KH) if (py + padding - kh) % 2 == 0]
            for px in range(2):
                kws = [kw for kw in range(KW) if (px + padding - kw) % 2 == 0]
                if not khs or not kws:
                    continue                       # no tap reaches this class (1x1: only (0, 0))
                # dy offsets (py+p-kh)/2 form a contiguous range [dmin, dmax]; a symmetric-pad conv has offsets t-P
                dh = [(py + padding - kh) // 2 for kh in khs]
                dw = [(px + padding - kw) // 2 for kw in kws]
                P = max(0, max(dh), max(dw), -min(dh), -min(dw))
                sub = weight.detach()[:, :, khs][:, :, :, kws].contiguous()    # ascending kh/kw; for_dgrad flips the taps
                pc = PackedConv.for_dgrad(sub, 0, scale, pad_override=P) if dtype == torch.float32 else \
                    PackedConv.for_dgrad_bf16(sub, 0, scale, pad_override=P)
                # flipped tap t <-> descending kh <-> offset dmin + t, conv offset t - P  =>  out row i' = i + dmin + P
                self.classes.append((py, px, pc, min(dh) + P, min(dw) + P))

    def __call__(self, dy, in_hw, add=None):
        N = dy.shape[0]
        H, W = in_hw
        dx = add.clone() if add is not None else torch.zeros((N, H, W, self.Cin), device=dy.device, dtype=torch.float32)
        assert dy.dtype == self.dtype
        for py, px, pc, sh, sw in self.classes:
            o = conv2d(dy, pc, out_dtype=torch.float32)
            _lib.call('cpr_phase_scatter_add', _ptr(o), _ptr(dx), N, o.shape[1], o.shape[2], self.Cin, H, W, py, px, sh, sw,
                      self.stride, _stream())
        return dx


def conv2d_dgrad(dy, pc_t, in_hw, stride=1, mask=None, add=None, colsum=False):
    """dx (N,H,W,Cin) of a conv whose transposed/flipped weights are ``pc_t`` (dgrad_pack).
    mask: the forward's post-ReLU input -- the result is the gradient BEFORE that ReLU (dx * (mask > 0)), fused into
    the epilogue; add: another gradient of the same tensor summed in the epilogue (before the mask when both are given); colsum: also return the
    per-channel sums of the result as TilePartials (-> (dx, partials); ``partials.reduce()`` gives the (C,) vector)."""
    N, OH, OW, Cout = _check(dy).shape
    H, W = in_hw
    assert isinstance(pc_t, PhasedDgrad) or pc_t.dilation == 1 or stride == 1, 'the data gradient of a dilated conv is built for stride 1'
    if not isinstance(pc_t, PhasedDgrad) and pc_t.groups > 1:
        # grouped layer: the grouped kernel over dy (its epilogue has no extra operand), then sum / mask / column sums as ONE streaming
        # pass over the result.  Stride 2: zero insertion -- the map is the block's narrow one and three layers of the net are strided
        if stride > 1:
            z = torch.empty((N, H, W, Cout), device=dy.device, dtype=torch.float32)
            _lib.call('cpr_zero_insert', _ptr(dy), _ptr(z), N, OH, OW, Cout, H, W, stride, _stream())
            dy = z
        dx = conv2d(dy, pc_t)
        assert dx.shape[1] == H and dx.shape[2] == W, (dx.shape, in_hw)
        if mask is None and not colsum:
            return dx if add is None else axpby(dx, add, 1.0, 1.0)
        keep = mask is not None or add is not None
        g, cs = relu_bwd_colsum(dx, mask, want_g=keep, add=add)
        dx = g if keep else dx
        return (dx, cs) if colsum else dx
    if mask is not None and add is not None:
        # the conv epilogue has one extra operand (the sum OR the mask source): the sum rides in the epilogue, mask and column sums
        # are one streaming pass over the result
        g, cs = relu_bwd_colsum(conv2d_dgrad(dy, pc_t, in_hw, stride, add=add), mask)
        return (g, cs) if colsum else g
    if isinstance(pc_t, PhasedDgrad):
        dx = pc_t(dy, in_hw, add=add)
        if mask is not None or colsum:
            g, cs = relu_bwd_colsum(dx, mask, want_g=mask is not None)
            dx = g if mask is not None else dx
            return (dx, cs) if colsum else dx
        return dx
    if stride > 1:
        # dilated gradient of extent (H + 2p - K + 1): rows/cols past (O-1)*s are the zeros the forward never read
        He, We = H + 2 * (pc_t.KH - 1 - pc_t.padding) - pc_t.KH + 1, W + 2 * (pc_t.KW - 1 - pc_t.padding) - pc_t.KW + 1
        z = torch.empty((N, He, We, Cout), device=dy.device, dtype=torch.float32)
        _lib.call('cpr_zero_insert', _ptr(dy), _ptr(z), N, OH, OW, Cout, He, We, stride, _stream())
        dy = z
    res = mask if mask is not None else add
    out = conv2d(dy, pc_t, residual=res, res_mask=mask is not None, colsum=colsum)
    o = out[0] if colsum else out
    assert o.shape[1] == H and o.shape[2] == W, (o.shape, in_hw)
    return out


def conv_wgrad_bf16_supported(x_shape, weight_shape, stride, padding, maps_bf16=False):
    """Whether conv_wgrad_bf16 takes this layer (1x1 or 3x3 / padding 1): maps_bf16 (both maps are bf16) -- the pixel-major kernel
    (csrc/conv_wgrad_bf16_tn.hip) or the rewriting path; else the rewriting path alone (csrc/conv_wgrad_bf16.hip), and not for a 1x1
    layer below 256 couts.  The shape rule itself is the C query's (cpr_conv_wgrad_bf16_workspace_s: negative = unsupported, called
    directly -- here that is an answer, not an error)."""
    Cout, Cin, KH, KW = weight_shape
    if Cin != x_shape[3]:          # a grouped layer: fp32 only
        return False
    if KH == 1 and Cout < 256 and not maps_bf16:      # measured (tools/wgrad_bf16_bench.py): the two rewrites cost what the bf16 GEMM saves
        return False
    if KH != KW or padding != KH // 2:                 # (the query sees one kernel size and no padding)
        return False
    return _lib.load().cpr_conv_wgrad_bf16_workspace_s(x_shape[0], x_shape[1], x_shape[2], Cin, Cout, KH, stride, int(maps_bf16),
                                                       int(maps_bf16)) > 0


def conv_wgrad_bf16(dy, x, weight_shape, out=None, accumulate=False, stride=1):
    """Weight gradient of a conv (1x1 or 3x3 / padding 1) on the bf16 matrix cores (mixed-precision training step): dy (N,OH,OW,Cout)
    and x (N,H,W,Cin) bf16 or fp32 (rounded to bf16 on the way in) -> [Cout][Cin][k][k] fp32.  stride 2 needs both maps in bf16."""
    N, H, W, Cin = x.shape
    Cout, Cin_w, KH, KW = weight_shape
    OH, OW = (H + 2 * (KH // 2) - KH) // stride + 1, (W + 2 * (KH // 2) - KH) // stride + 1
    assert Cin_w == Cin and tuple(dy.shape) == (N, OH, OW, Cout) and KH == KW, (tuple(dy.shape), (N, OH, OW, Cout))
    assert x.dtype in (torch.float32, torch.bfloat16) and dy.dtype in (torch.float32, torch.bfloat16)
    assert x.is_contiguous() and dy.is_contiguous()
    dy16, x16 = int(dy.dtype == torch.bfloat16), int(x.dtype == torch.bfloat16)
    units = _lib.call('cpr_conv_wgrad_bf16_workspace_s', N, H, W, Cin, Cout, KH, stride, dy16, x16, positive=True)
    ws = torch.empty((units * 256,), device=x.device, dtype=torch.uint8)
    if out is None:
        assert not accumulate
        out = torch.empty(tuple(weight_shape), device=x.device, dtype=torch.float32)
    assert tuple(out.shape) == tuple(weight_shape) and out.is_contiguous() and out.dtype == torch.float32
    _lib.call('cpr_conv_wgrad_bf16_s', _ptr(dy), dy16, _ptr(x), x16, _ptr(out), _ptr(ws), N, H, W, Cin, Cout, KH, stride, int(accumulate),
              _stream())
    return out


def conv3x3_wino_wgrad(dy, x, weight_shape, in_ab=None, in_relu=False, grad=None, out=None):
    """Weight gradient of a 3x3 / stride 1 / pad 1 conv as fused Winograd F(2x2,3x3) (csrc/conv_wino_wgrad.hip: 16 GEMMs over
    the tiles, 2.25x fewer multiplies).  Same arguments as conv2d_wgrad; Cin % 64 == 0, Cout % 64 == 0."""
    N, H, W, Cin = _check(x).shape
    Cout = _check(dy).shape[-1]
    assert tuple(weight_shape) == (Cout, Cin, 3, 3) and tuple(dy.shape[:3]) == (N, H, W)
    n = _lib.call('cpr_conv3x3_wino_wgrad_workspace', N, H, W, Cin, Cout, positive=True)
    ws = torch.empty((n,), device=x.device, dtype=torch.float32)
    acc = grad is not None
    if grad is None:
        grad = out if out is not None else torch.empty(tuple(weight_shape), device=x.device, dtype=torch.float32)
    assert tuple(grad.shape) == tuple(weight_shape) and grad.is_contiguous()
    a, b = in_ab if in_ab is not None else (None, None)
    _lib.call('cpr_conv3x3_wino_wgrad', _ptr(dy), _ptr(x), _ptr(a), _ptr(b), _ptr(grad), _ptr(ws), N, H, W, Cin, Cout,
              int(in_relu), int(acc), _stream())
    return grad


def conv2d_wgrad(dy, x, weight_shape, stride, padding, in_ab=None, in_relu=False, grad=None, out=None, groups=1, dilation=1):
    """grad_w [Cout][Cin][KH][KW]: accumulated into ``grad`` when given, written into ``out`` when given, else a new
    tensor.  in_ab: fused GroupNorm affine (+ReLU) of the input.  groups > 1: a grouped 3x3 / padding 1 layer, grad_w (C, C / groups, 3, 3)
    (csrc/conv_group.hip; the split over pixels is added up in a fixed order); dy and x may sit at a channel pitch >= C (their last
    dimension), whose pad channels are not read.  dilation > 1: the dilated kernels (cpr_conv2d_wgrad_dil, cpr_conv_group_wgrad_dil; no
    fused input affine), never the Winograd route."""
    N, H, W, Cin = _check(x).shape
    _, OH, OW, Cout = _check(dy).shape
    KH, KW = weight_shape[2], weight_shape[3]
    dilation = int(dilation)
    assert dilation >= 1
    if groups > 1:
        cg, C = weight_shape[1], weight_shape[0]
        assert Cout == Cin >= C == cg * groups and Cin % 4 == 0 and cg in GROUP_WIDTHS and (KH, KW) == (3, 3) and padding == dilation and \
            in_ab is None and not in_relu and x.dtype == torch.float32 and dy.dtype == torch.float32, (weight_shape, groups, Cin, Cout)
        assert (OH, OW) == ((H - 1) // stride + 1, (W - 1) // stride + 1), (dy.shape, x.shape, stride)
        n = _lib.call('cpr_conv_group_wgrad_workspace', N, OH, OW, C, cg, positive=True)
        ws = torch.empty((n,), device=x.device, dtype=torch.float32)
        acc = grad is not None
        if grad is None:
            grad = out if out is not None else torch.empty(tuple(weight_shape), device=x.device, dtype=torch.float32)
        assert tuple(grad.shape) == tuple(weight_shape) and grad.is_contiguous()
        if dilation != 1:
            assert stride == 1 and Cin == C, 'grouped conv: dilation=%d needs stride 1 and unpitched maps' % dilation
            _lib.call('cpr_conv_group_wgrad_dil', _ptr(dy), _ptr(x), _ptr(grad), _ptr(ws), N, H, W, Cin, cg, dilation, int(acc), _stream())
        elif Cin == C:
            _lib.call('cpr_conv_group_wgrad', _ptr(dy), _ptr(x), _ptr(grad), _ptr(ws), N, H, W, Cin, cg, stride, int(acc), _stream())
        else:
            _lib.call('cpr_conv_group_wgrad_pitch', _ptr(dy), _ptr(x), _ptr(grad), _ptr(ws), N, H, W, C, Cin, cg, stride, int(acc),
                      _stream())
        return grad
    assert weight_shape[0] == Cout and weight_shape[1] == Cin, (weight_shape, Cout, Cin)
    if dilation == 1 and WINOGRAD[0] and KH == 3 and KW == 3 and stride == 1 and padding == 1 and Cin % 64 == 0 and Cout % 64 == 0 and \
            x.dtype == torch.float32 and W / float((W + 15) // 16 * 16) >= WINO_MIN_FILL and H * W >= 1024 and \
            (in_ab is None or Cin <= 512):     # (20x20 maps: too few tiles per K slice against 16 frequencies of partials)
        return conv3x3_wino_wgrad(dy, x, weight_shape, in_ab, in_relu, grad, out)
    n = _lib.call('cpr_conv2d_wgrad_workspace', N, OH, OW, Cin, Cout, KH, KW, positive=True)
    ws = torch.empty((n,), device=x.device, dtype=torch.float32)
    acc = grad is not None
    if grad is None:
        grad = out if out is not None else torch.empty(tuple(weight_shape), device=x.device, dtype=torch.float32)
    assert tuple(grad.shape) == tuple(weight_shape) and grad.is_contiguous()
    if dilation != 1:
        assert in_ab is None and not in_relu and x.dtype == torch.float32 and dy.dtype == torch.float32, \
            'a dilated conv (dilation=%d) has no fused-input-affine or bf16 weight gradient' % dilation
        assert (OH, OW) == ((H + 2 * padding - dilation * (KH - 1) - 1) // stride + 1,
                            (W + 2 * padding - dilation * (KW - 1) - 1) // stride + 1), (dy.shape, x.shape, stride, padding, dilation)
        _lib.call('cpr_conv2d_wgrad_dil', _ptr(dy), _ptr(x), _ptr(grad), _ptr(ws), N, H, W, Cin, Cout, KH, KW, stride, padding, dilation,
                  int(acc), _stream())
        return grad
    a = b = None
    if in_ab is not None:
        a, b = in_ab
    _lib.call('cpr_conv2d_wgrad', _ptr(dy), _ptr(x), _ptr(a), _ptr(b), _ptr(grad), _ptr(ws), N, H, W, Cin, Cout, KH, KW,
              stride, padding, int(in_relu), int(acc), _stream())
    return grad


def gn_bwd(x, dz, a, b, mean, rstd, gamma, relu, dgamma=None, dbeta=None, slots=None, out_dgamma=None, out_dbeta=None,
           want16=False, want32=True):
    """GroupNorm(+ReLU) backward -> (dx, dgamma, dbeta); accumulates into dgamma/dbeta when given, writes into
    out_dgamma/out_dbeta when given.  x bf16 (the map the mixed-precision forward recorded): read as it is, and with want16 the
    bf16 rounding of dx is written by the same pass -> (dx | None, dgamma, dbeta, dx16)."""
    N, H, W, C = _check(x, ACT).shape
    HW, G = H * W, mean.shape[1]
    if slots is None:
        slots = max(1, min(256, HW // 256))
    acc = dgamma is not None
    if not acc:
        dgamma = out_dgamma if out_dgamma is not None else torch.empty((C,), device=x.device, dtype=torch.float32)
        dbeta = out_dbeta if out_dbeta is not None else torch.empty((C,), device=x.device, dtype=torch.float32)
    ws_part = torch.empty((N * slots * C * 2,), device=x.device, dtype=torch.float32)
    ws_k = torch.empty((2 * N * G + 2 * N * C,), device=x.device, dtype=torch.float32)
    if x.dtype == torch.bfloat16:
        assert want16 or want32
        dx = torch.empty(tuple(x.shape), device=x.device, dtype=torch.float32) if want32 else None
        dx16 = torch.empty_like(x) if want16 else None
        assert dz.dtype in (torch.float32, torch.bfloat16) and dz.is_contiguous()
        _lib.call('cpr_gn_bwd_bf16_dz16' if dz.dtype == torch.bfloat16 else 'cpr_gn_bwd_bf16', _ptr(x), _ptr(dz), _ptr(a), _ptr(b), _ptr(mean), _ptr(rstd), _ptr(_check(gamma)),
                  _ptr(dx), _ptr(dx16), _ptr(dgamma), _ptr(dbeta), _ptr(ws_part), _ptr(ws_k), N, HW, C, G, slots, int(relu),
                  int(acc), _stream())
        return dx, dgamma, dbeta, dx16
    assert want32 and not want16
    dx = torch.empty_like(x)
    _lib.call('cpr_gn_bwd', _ptr(x), _ptr(_check(dz)), _ptr(a), _ptr(b), _ptr(mean), _ptr(rstd), _ptr(_check(gamma)),
              _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(ws_part), _ptr(ws_k), N, HW, C, G, slots, int(relu), int(acc),
              _stream())
    return dx, dgamma, dbeta


def upsample_add_bwd(dfine, dcoarse_or_shape, accumulate=True):
    N, H, W, C = _check(dfine).shape
    if isinstance(dcoarse_or_shape, torch.Tensor):
        dc = dcoarse_or_shape
    else:
        dc, accumulate = torch.empty(dcoarse_or_shape, device=dfine.device, dtype=torch.float32), False
    _lib.call('cpr_upsample_add_bwd', _ptr(dfine), _ptr(dc), N, H, W, dc.shape[1], dc.shape[2], C, int(accumulate),
              _stream())
    return dc


def subsample2(x, a=None, b=None):
    """F.max_pool2d(y, 1, stride=2) of an NHWC map (fp32 or bf16): y = x, or x*a[n,c] + b[n,c] -- a pending GroupNorm affine
    applied on load, so a lazy FPN output is never materialised just to be subsampled (csrc/fpn_extra.hip)."""
    N, H, W, C = _check(x, ACT).shape
    assert (a is None) == (b is None)
    out = torch.empty((N, (H + 1) // 2, (W + 1) // 2, C), device=x.device, dtype=x.dtype)
    _lib.call('cpr_subsample2', _ptr(x), int(x.dtype == torch.bfloat16), _ptr(a), _ptr(b), _ptr(out), N, H, W, C, _stream())
    return out


def subsample2_bwd_add(dfine, dcoarse):
    """dfine + zero_insert(dcoarse): the gradient of a max-pool extra level joins the finer output's own, one pass."""
    N, H, W, C = _check(dfine).shape
    assert tuple(_check(dcoarse).shape) == (N, (H + 1) // 2, (W + 1) // 2, C), (dfine.shape, dcoarse.shape)
    out = torch.empty_like(dfine)
    _lib.call('cpr_subsample2_bwd_add', _ptr(dfine), _ptr(dcoarse), _ptr(out), N, H, W, C, _stream())
    return out


def relu_mask_add(dz, d, y):
    """dz + (y > 0 ? d : 0) (relu_before_extra_convs: y is the map the next extra conv read, fp32 or bf16)."""
    assert dz.shape == d.shape == y.shape and _check(y, ACT).is_contiguous()
    out = torch.empty_like(_check(dz))
    _lib.call('cpr_relu_mask_add', _ptr(dz), _ptr(_check(d)), _ptr(y), int(y.dtype == torch.bfloat16), _ptr(out), dz.numel(),
              _stream())
    return out


def relu_bwd_colsum(dy, y=None, want_g=True, colsum=None, want16=False, add=None):
    """g = dy*(y>0) (y None: g = dy) and per-channel column sums of g -> (g|None, colsum (C)[, g16]).  y fp32 or the bf16 map the
    mixed-precision forward recorded (read as it is); want16: also the bf16 rounding of g, written by the same pass; add (fp32, same
    shape): g = (dy + add)*(y>0) -- a shortcut gradient joining in the same pass."""
    C = dy.shape[-1]
    M = dy.numel() // C
    acc = colsum is not None
    if not acc:
        colsum = torch.empty((C,), device=dy.device, dtype=torch.float32)
    g = torch.empty_like(dy) if want_g else None
    g16 = torch.empty(tuple(dy.shape), device=dy.device, dtype=torch.bfloat16) if want16 else None
    ws = torch.empty((_lib.call('cpr_relu_bwd_colsum_ws', M, C, positive=True),), device=dy.device, dtype=torch.float32)
    if y is not None:
        assert y.dtype in (torch.float32, torch.bfloat16) and y.is_contiguous() and y.numel() == dy.numel()
    if add is not None:
        assert add.dtype == torch.float32 and add.is_contiguous() and add.numel() == dy.numel() and want_g
    _lib.call('cpr_relu_bwd_colsum', _ptr(_check(dy)), _ptr(add), _ptr(y), int(y is not None and y.dtype == torch.bfloat16), _ptr(g), _ptr(g16),
              _ptr(colsum), _ptr(ws), M, C, int(acc), _stream())
    return (g, colsum, g16) if want16 else (g, colsum)


def bn_fold_bwd(Gw, weight, scale, mean, inv_sigma, colsum_g, want_affine=True, out_dgamma=None, out_dbeta=None):
    """In place dW = scale*Gw; returns (dgamma, dbeta) of the folded eval BatchNorm (or (None, None)).  colsum_g: the (Cout,) column
    sums of the output gradient, or the TilePartials a conv epilogue left (summed inside the kernel)."""
    Cout = Gw.shape[0]
    K = Gw.numel() // Cout
    dg, db = out_dgamma, out_dbeta
    if want_affine and dg is None:
        dg = torch.empty((Cout,), device=Gw.device, dtype=torch.float32)
        db = torch.empty((Cout,), device=Gw.device, dtype=torch.float32)
    if isinstance(colsum_g, TilePartials):     # the conv epilogue's partials as they are: the kernel adds its channel's column up
        assert colsum_g.C == Cout
        _lib.call('cpr_bn_fold_bwd_part', _ptr(Gw), _ptr(_check(weight)), _ptr(scale), _ptr(mean), _ptr(inv_sigma),
                  _ptr(colsum_g.part), colsum_g.tiles, _ptr(dg), _ptr(db), Cout, K, _stream())
        return dg, db
    _lib.call('cpr_bn_fold_bwd', _ptr(Gw), _ptr(_check(weight)), _ptr(scale), _ptr(mean), _ptr(inv_sigma),
              _ptr(colsum_g), _ptr(dg), _ptr(db), Cout, K, _stream())
    return dg, db


def concurrent_stream(device, tries=8, spin_us=150.0):
    """A new torch stream that runs CONCURRENTLY with the current one, i.e. sits on another hardware queue.  The HIP runtime
    multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues, so a fresh stream shares the current stream's queue
    with probability 1 / queues (and always, once RCCL has taken the queues: pointtinybenchmark_amd/__init__.py) -- work on it
    then simply runs after the current stream's.  Probe: one idle wave of ``spin_us`` on each of the two streams (csrc/pack.hip,
    cpr_spin); together they take ~spin_us on two queues and ~2 spin_us on one.  -> (stream, concurrent: bool); after ``tries``
    shared candidates the last one is returned with concurrent = False."""
    ticks = int(spin_us * 100)                                    # 100 MHz wall clock
    s, ok = None, False
    with torch.cuda.device(device):                                # the probe's launches belong to ``device`` whatever the caller's current device is
        cur = torch.cuda.current_stream(device)
        for _ in range(tries):
            s = torch.cuda.Stream(device=device)
            _lib.call('cpr_spin', 1, s.cuda_stream)                # first use of a stream creates its queue: keep that out of the timing
            _lib.call('cpr_spin', 1, cur.cuda_stream)
            torch.cuda.synchronize(device)
            best = float('inf')
            for _rep in range(3):                                  # a shared GPU can stretch one measurement: the minimum of three decides
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(cur)
                s.wait_stream(cur)                                 # both spins start after e0
                _lib.call('cpr_spin', ticks, cur.cuda_stream)
                _lib.call('cpr_spin', ticks, s.cuda_stream)
                cur.wait_stream(s)
                e1.record(cur)
                e1.synchronize()
                best = min(best, e0.elapsed_time(e1) * 1e3)
                if best < 1.6 * spin_us:
                    break
            if best < 1.6 * spin_us:
                ok = True
                break
    return s, ok


def axpby(y, x, alpha=1.0, beta=1.0):
    assert y.numel() == x.numel()
    _lib.call('cpr_axpby', _ptr(_check(y)), _ptr(_check(x)), float(alpha), float(beta), y.numel(), _stream())
    return y


def cpr_loss_bwd(lmap, neg_mask, out5, bag_logits, valid, labels, bag_ws, centers, gt_img, offsets, ins_off, num_classes,
                 stride, w_mil, w_gt, w_neg, Jd, gt_weight=None, eps=1e-6, upstream=None, radius_cells=None, gather=True):
    """-> dmap (N,H,W,Jd): gradient of gt_loss + pos_loss + neg_loss wrt the logit map (channels >= J are zero).
    radius_cells: the bag radius in grid cells (every offset lies within radius_cells * stride of its centre): the taps of a
    bag are gathered in a (2 * radius_cells + 3)^2 window -- deterministic, no float atomics.  gt_img must ascend.
    upstream (5,) fp32 device tensor: gradient of the caller's total wrt the forward's (gt_loss, pos_loss, bag_acc, neg_loss,
    num_sample) vector -- the autograd bridge passes what torch hands it; None = unit weights."""
    assert upstream is None or (upstream.numel() == 5 and upstream.dtype == torch.float32 and upstream.is_contiguous())
    N, H, W, J = _check(lmap).shape
    G, K, _ = bag_logits.shape
    dmap = torch.empty((N, H, W, Jd), device=lmap.device, dtype=torch.float32)
    dbag = torch.empty((G, K, J), device=lmap.device, dtype=torch.float32)
    if gather:
        assert radius_cells is not None and radius_cells >= 0, 'the bag radius (in cells) sizes the gather window'
        win = 2 * int(math.ceil(radius_cells)) + 3      # taps of a bag span floor(c - r) .. floor(c + r) + 1
        win_ws = torch.empty((G, win, win, J), device=lmap.device, dtype=torch.float32)
        win_org = torch.empty((G, 2), device=lmap.device, dtype=torch.int32)
    else:     # the bag logits were not sampled from ``lmap`` (num_cls_fcs > 0): dmap = the negative-grid term, dbag is returned as is
        win, win_ws, win_org = 0, None, None
    _lib.call('cpr_loss_bwd', _ptr(lmap), _ptr(neg_mask), _ptr(out5), _ptr(bag_logits), _ptr(valid), _ptr(labels),
              _ptr(gt_weight), _ptr(bag_ws), _ptr(centers), _ptr(gt_img), _ptr(offsets), _ptr(dbag), _ptr(dmap), _ptr(win_ws),
              _ptr(win_org), win, N, H, W, J, Jd, ins_off, G, K, num_classes, float(stride), float(eps), float(w_mil),
              float(w_gt), float(w_neg), _ptr(upstream), _stream())
    return dmap, dbag


def cpr_loss_bwd_general(lmap, neg_mask, out5, bag_logits, valid, labels, bag_ws, bags, centres, ins_off, num_cls_out, Jd,
                         w_mil, w_gt, w_neg, gt_weight=None, eps=1e-6, upstream=None, prob_type='sigmoid', norm_p=1.0,
                         binary_ins=False, allpos=False, neg_from_gt=False):
    """The loss gradients for any CPRHead loss option (csrc/backward.hip, general form): bags / centres are ops.mil_loss's
    geometry tuples.  -> (dmap (N,H,W,Jd): the negative-grid term alone, dbag: the gradient wrt every bag entry's logits in the
    layout of ``bag_logits`` -- not gathered onto the map)."""
    assert upstream is None or (upstream.numel() == 5 and upstream.dtype == torch.float32 and upstream.is_contiguous())
    N, H, W, J = _check(lmap).shape
    E = bag_logits.numel() // J
    nb, bstride, boff, blen = bags
    coff, cstride, ccount, cmod = centres
    assert nb * bstride == E and labels.numel() == nb, (nb, bstride, E)
    dmap = torch.empty((N, H, W, Jd), device=lmap.device, dtype=torch.float32)
    dbag = torch.empty(tuple(bag_logits.shape), device=lmap.device, dtype=torch.float32)
    _lib.call('cpr_loss_bwd_general', _ptr(lmap), _ptr(neg_mask), _ptr(out5), _ptr(_check(bag_logits)), _ptr(valid), _ptr(labels),
              _ptr(gt_weight), _ptr(bag_ws), _ptr(dbag), _ptr(dmap), N, H, W, J, Jd, int(ins_off), nb, bstride, boff, blen, coff,
              max(int(cstride), 1), ccount, cmod, int(num_cls_out), float(eps), PROB_TYPES[prob_type], float(norm_p), int(binary_ins),
              int(allpos), float(w_mil), float(w_gt), float(w_neg), int(neg_from_gt), _ptr(upstream), _stream())
    return dmap, dbag


def bag_gather_bwd(dsample, centers, gt_img, offsets, dmap, stride, radius_cells):
    """dsample (G,K,J): gradient wrt the bilinear samples ``bag_sample`` took from a (N,H,W,J') map, J <= J'; ADDED onto dmap
    (N,H,W,J') through the same taps (deterministic: per-bag windows, per-image gt order).  gt_img must ascend."""
    G, K, J = _check(dsample).shape
    N, H, W, Jd = _check(dmap).shape
    win = 2 * int(math.ceil(radius_cells)) + 3
    win_ws = torch.empty((G, win, win, J), device=dmap.device, dtype=torch.float32)
    win_org = torch.empty((G, 2), device=dmap.device, dtype=torch.int32)
    _lib.call('cpr_bag_gather_bwd', _ptr(dsample), J, _ptr(centers), _ptr(gt_img), _ptr(offsets), _ptr(win_ws), _ptr(win_org), win,
              _ptr(dmap), N, H, W, Jd, G, K, float(stride), _stream())
    return dmap


def bag_points_gather_bwd(dsample, pts, code, gt_img, dmap, stride, align_corners=False, want_bias=False):
    """The gather stage from the forward's point list (grid generators, align_corners=True): dsample (G,Kt,J) ADDED onto dmap
    (N,H,W,J'), J <= J'; pts (G,Kt,2); code (G,Kt) int32 from ``grid_bag(want_cell=True)`` or None (every entry a bilinear sample).
    want_bias: also return (J,) = what the projection's bias receives through padding slots / dropped taps."""
    G, Kt, J = _check(dsample).shape
    N, H, W, Jd = _check(dmap).shape
    assert pts.numel() == G * Kt * 2 and (code is None or (code.numel() == G * Kt and code.dtype == torch.int32))
    wout = torch.empty((G * Kt,), device=dmap.device, dtype=torch.float32) if want_bias else None
    dbias = torch.empty((J,), device=dmap.device, dtype=torch.float32) if want_bias else None
    _lib.call('cpr_bag_points_gather_bwd', _ptr(dsample), J, _ptr(_check(pts)), _ptr(code), _ptr(gt_img), _ptr(dmap), _ptr(wout),
              _ptr(dbias), N, H, W, Jd, G, Kt, float(stride), int(align_corners), _stream())
    return dbias


def p2p_loss_bwd(logits, pred, gt_inds, gt_pts, gt_labels, gt_start, alpha, gamma, beta, pos_w, neg_w, reg_norm, w_cls,
                 w_reg, gamma_p, Cp, Rp, upstream=None, cls_mode=0, reg_mode=0):
    """-> (dcls (B,M,Cp), dreg (B,M,Rp)): gradient of the summed P2P losses wrt class logits / regression output.
    upstream (B,2): gradient of the caller's total wrt each image's (loss_cls, loss_pts); None = unit weights."""
    B, M, C = _check(logits).shape
    assert upstream is None or (tuple(upstream.shape) == (B, 2) and upstream.dtype == torch.float32 and upstream.is_contiguous())
    _check(pred), _check(gt_inds, torch.int64), _check(gt_pts), _check(gt_labels, torch.int32), _check(gt_start, torch.int32)
    assert tuple(pred.shape) == (B, M, 3) and tuple(gt_inds.shape) == (B, M) and gt_start.numel() >= B, \
        (tuple(pred.shape), tuple(gt_inds.shape), gt_start.numel())
    npos = (gt_inds > 0).sum().to(torch.float32).reshape(1)          # device scalar, no host sync
    dcls = torch.empty((B, M, Cp), device=logits.device, dtype=torch.float32)
    dreg = torch.empty((B, M, Rp), device=logits.device, dtype=torch.float32)
    _lib.call('cpr_p2p_loss_bwd', _ptr(logits), _ptr(pred), _ptr(gt_inds), _ptr(gt_pts), _ptr(gt_labels),
              _ptr(gt_start), _ptr(npos), _ptr(dcls), _ptr(dreg), B, M, C, Cp, Rp, float(alpha), float(gamma), float(beta),
              float(pos_w), float(neg_w), float(reg_norm), float(w_cls), float(w_reg), float(gamma_p), _ptr(upstream),
              int(cls_mode), int(reg_mode), _stream())
    return dcls, dreg


P2P_LOSS_BWD_MAX_LEVELS = 8       # csrc/backward.hip: the level table of p2p_loss_bwd_kernel


def p2p_grad_pad(n):
    """Channel count of an output-conv gradient map with n live channels, as the conv gradient kernels take it."""
    return 4 if n <= 4 else (n + 31) // 32 * 32


def p2p_loss_bwd_levels(logits, pred, gt_inds, gt_pts, gt_labels, gt_start, shapes, num_points, alpha, gamma, beta, pos_w, neg_w,
                        reg_norm, w_cls, w_reg, gamma_p, upstream=None, cls_mode=0, reg_mode=0, cps=None, rps=None, offsets=None,
                        out=None):
    """``p2p_loss_bwd`` for several FPN levels and ``num_points`` points per cell.  logits (B, M, C) / pred (B, M, 3): the levels'
    proposals concatenated (P2PHead.get_pred_points); shapes: [(H_l, W_l)] per level.  -> (dcls list of (B, H_l, W_l, cp_l),
    dreg list of (B, H_l, W_l, rp_l)): the gradient maps of every level's cls_out / reg_out, point p's channels at p*C .. and
    p*2 .., padding zero.  cps / rps / offsets default to p2p_grad_pad(P*C) / p2p_grad_pad(2P) / the running row offsets.
    out: (dcls, dreg) lists of maps to write into instead of fresh ones."""
    B, M, C = _check(logits).shape
    P, L = int(num_points), len(shapes)
    assert upstream is None or (tuple(upstream.shape) == (B, 2) and upstream.dtype == torch.float32 and upstream.is_contiguous())
    _check(pred), _check(gt_inds, torch.int64), _check(gt_pts), _check(gt_labels, torch.int32), _check(gt_start, torch.int32)
    assert tuple(pred.shape) == (B, M, 3) and tuple(gt_inds.shape) == (B, M) and gt_start.numel() >= B, \
        (tuple(pred.shape), tuple(gt_inds.shape), gt_start.numel())
    cps = [p2p_grad_pad(P * C)] * L if cps is None else [int(c) for c in cps]
    rps = [p2p_grad_pad(2 * P)] * L if rps is None else [int(r) for r in rps]
    if offsets is None:
        offsets = [0]
        for h, w in shapes[:-1]:
            offsets.append(offsets[-1] + h * w * P)
    npos = (gt_inds > 0).sum().to(torch.float32).reshape(1)          # device scalar, no host sync
    if out is None:
        dcls = [torch.empty((B, h, w, c), device=logits.device, dtype=torch.float32) for (h, w), c in zip(shapes, cps)]
        dreg = [torch.empty((B, h, w, r), device=logits.device, dtype=torch.float32) for (h, w), r in zip(shapes, rps)]
    else:
        dcls, dreg = list(out[0]), list(out[1])
        for t, (h, w), c in list(zip(dcls, shapes, cps)) + list(zip(dreg, shapes, rps)):
            assert tuple(_check(t).shape) == (B, h, w, c), (tuple(t.shape), (B, h, w, c))
    n = max(L, 1)
    ints = lambda v: (ctypes.c_int * n)(*[int(x) for x in v])                          # noqa: E731  (host tables)
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])               # noqa: E731
    _lib.call('cpr_p2p_loss_bwd_levels', _ptr(logits), _ptr(pred), _ptr(gt_inds), _ptr(gt_pts), _ptr(gt_labels), _ptr(gt_start),
              _ptr(npos), B, M, C, P, L, ints([h * w for h, w in shapes]), ints(offsets), ints(cps), ints(rps), ptrs(dcls),
              ptrs(dreg), float(alpha), float(gamma), float(beta), float(pos_w), float(neg_w), float(reg_norm), float(w_cls),
              float(w_reg), float(gamma_p), _ptr(upstream), int(cls_mode), int(reg_mode), _stream())
    return dcls, dreg


def grad_sumsq(g, out, ws, accumulate):
    _lib.call('cpr_grad_sumsq', _ptr(_check(g)), g.numel(), _ptr(ws), _ptr(out), int(accumulate), _stream())


def sgd_step(p, grad, buf, norm2, lr, momentum, weight_decay, max_norm, grad_scale, first):
    _lib.call('cpr_sgd_step', _ptr(p), _ptr(grad), _ptr(buf), _ptr(norm2), p.numel(), float(lr), float(momentum),
              float(weight_decay), float(max_norm), float(grad_scale), int(first), _stream())


def adam_step(p, grad, exp_avg, exp_avg_sq, norm2, lr, betas, eps, weight_decay, step, max_norm, grad_scale,
              decoupled=False):
    """torch.optim.Adam (AdamW: decoupled=True) step number ``step`` (1 at the first) on flat fp32 buffers, clipped with
    the coefficient of ``sgd_step`` (norm2: the device sum of squares of grad_sumsq; max_norm <= 0: no clip).  The bias
    corrections are formed here in double, as torch forms them in Python."""
    beta1, beta2 = float(betas[0]), float(betas[1])
    if step < 1:
        raise ValueError('adam_step: step counts from 1, got %r' % (step,))
    for t in (p, grad, exp_avg, exp_avg_sq):
        _check(t)
        if t.numel() != p.numel():
            raise _lib.CprHipError('adam_step: p, grad, exp_avg and exp_avg_sq must have one size')
    step_size = float(lr) / (1 - beta1 ** step)
    bc2_sqrt = (1 - beta2 ** step) ** 0.5
    _lib.call('cpr_adam_step', _ptr(p), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(norm2), p.numel(), float(lr),
              beta1, beta2, float(eps), float(weight_decay), step_size, bc2_sqrt, float(max_norm), float(grad_scale),
              int(bool(decoupled)), _stream())


# ---- data side: the job table of cpr_preprocess_jobs_u8 (include/cpr_hip.h: cpr_preprocess_job, 80 bytes) ----
PREPROCESS_JOB = [('src', '<u8'), ('out_off', '<i8'), ('scale_x', '<f8'), ('scale_y', '<f8')] + \
    [(k, '<i4') for k in ('pitch', 'src_w', 'src_h', 'x0', 'y0', 'cw', 'ch', 'dw', 'dh', 'flip', 'Hp', 'Wp')]


def preprocess_job_table(jobs, total_out_pixels):
    """Host copy of a job table, checked and completed: scale_x / scale_y = 1. / (dw / cw) in double (OpenCV's own expression).
    The library only ever sees the table as device memory, so its geometry is checked here: a job that would read outside its image
    or write outside the ``total_out_pixels`` of the output is an argument error."""
    import numpy as np
    jobs = np.ascontiguousarray(jobs, dtype=np.dtype(PREPROCESS_JOB)).copy()
    if len(jobs):
        j = {k: jobs[k].astype(np.int64) for k, _ in PREPROCESS_JOB if k not in ('scale_x', 'scale_y')}
        ok = (jobs['src'] != 0) & (j['src_w'] > 0) & (j['src_h'] > 0) & (j['pitch'] >= 3 * j['src_w']) & (j['x0'] >= 0) & \
            (j['y0'] >= 0) & (j['cw'] > 0) & (j['ch'] > 0) & (j['x0'] + j['cw'] <= j['src_w']) & (j['y0'] + j['ch'] <= j['src_h']) & \
            (j['dw'] > 0) & (j['dh'] > 0) & (j['Hp'] >= j['dh']) & (j['Wp'] >= j['dw']) & (j['out_off'] >= 0) & \
            (j['out_off'] + j['Hp'] * j['Wp'] <= total_out_pixels)
        if not ok.all():
            raise _lib.CprHipError('cpr_preprocess_jobs_u8: invalid argument (job %d)' % int(np.argmin(ok)))
        jobs['scale_x'] = 1.0 / (jobs['dw'].astype(np.float64) / jobs['cw'].astype(np.float64))
        jobs['scale_y'] = 1.0 / (jobs['dh'].astype(np.float64) / jobs['ch'].astype(np.float64))
    return jobs


def preprocess_jobs(jobs, mean3, stdinv3, to_rgb, out):
    """crop -> cv2 fixed-point bilinear resize -> flip -> Normalize -> Pad for a table of jobs in ONE launch.  ``jobs``: host numpy
    records of PREPROCESS_JOB (preprocess_job_table checks them and fills in the scales); ``out``: a contiguous fp32 device tensor
    of 4-float pixels."""
    import numpy as np
    if _check(out).numel() % 4:
        raise _lib.CprHipError('cpr_preprocess_jobs_u8: invalid argument (out holds 4-float pixels)')
    total = out.numel() // 4
    jobs = preprocess_job_table(jobs, total)
    n = len(jobs)
    table = torch.from_numpy(jobs.view(np.uint8).reshape(-1)).to(out.device) if n else None
    m = (ctypes.c_float * 3)(*[float(v) for v in mean3])
    s = (ctypes.c_float * 3)(*[float(v) for v in stdinv3])
    _lib.call('cpr_preprocess_jobs_u8', _ptr(table), n, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p),
              int(bool(to_rgb)), _ptr(out), total, _stream())
    return out


def scale_clip_flip_boxes(boxes, img_of, flips, img_hw, scale4, clip=True):
    """In place: boxes (n,4) * scale4[img] -> clip to the resized img_hw[img] -> mirror when flips[img] (Resize then RandomFlip)."""
    n = boxes.shape[0]
    if n:
        _check(boxes), _check(img_of, torch.int32), _check(flips, torch.int32), _check(img_hw, torch.int32), _check(scale4)
        k = flips.numel()
        if boxes.shape[1] != 4 or img_of.numel() != n or img_hw.numel() != 2 * k or scale4.numel() != 4 * k:
            raise _lib.CprHipError('scale_clip_flip_boxes: boxes (n,4), img_of (n), flips (N), img_hw (N,2), scale4 (N,4)')
    _lib.call('cpr_scale_clip_flip_boxes', _ptr(boxes), _ptr(img_of), _ptr(flips), _ptr(img_hw), _ptr(scale4), n, int(bool(clip)),
              _stream())
    return boxes


# ---- Res2Net slice kernels (csrc/res2net.hip): the Bottle2neck 3x3 chain on channel slices of the block's two internal maps.
# A slice is the channels [off, off + width) of a contiguous NHWC fp32 map; the C entry points check widths, offsets, pitches and strides
# (include/cpr_hip.h) and raise CprHipError('... invalid argument') before any launch.
RES2_MAX_WIDTH = 512       # widths the slice kernels take: even, 2 .. 512
RES2_MAX_SCALES = 8


def res2_width_ok(width):
    return 2 <= width <= RES2_MAX_WIDTH and width % 2 == 0


class Res2Pack:
    """A (width, width, 3, 3) parameter in the slice conv's own image (cpr_res2_pack_weights): 9 * width * width floats
    [tap][width / 2][2][width / 2][2].  transpose: the data-gradient pack -- in / out channels swapped, taps flipped, ``scale`` (the forward
    conv's folded BatchNorm) multiplied in."""

    def __init__(self, weight, scale=None, transpose=False):
        O, I, KH, KW = weight.shape
        assert weight.is_cuda, 'the slice-conv pack is built on the device'
        assert O == I and (KH, KW) == (3, 3), 'slice conv: a (width, width, 3, 3) weight, got %s' % (tuple(weight.shape),)
        src = weight.detach()
        if src.dtype != torch.float32 or not src.is_contiguous():
            src = src.float().contiguous()
        self.width, self.transpose = O, bool(transpose)
        self.w = torch.empty((9 * O * O,), device=weight.device, dtype=torch.float32)
        _lib.call('cpr_res2_pack_weights', _ptr(src), _ptr(scale), _ptr(self.w), O, int(self.transpose), _stream())
        self.ready = record_ready()


def _res2_map(t):
    N, H, W, pitch = _check(t).shape
    return N, H, W, pitch


def res2_conv(x, x_off, pack, out, out_off, stride=1, add=None, add_off=0, scale=None, bias=None, relu=False, transposed=False):
    """out[..., out_off : out_off + width] = relu?(conv3x3(x[..., x_off : x_off + width] (+ add[..., add_off : ...]), pack) * scale + bias),
    padding 1, stride 1 or 2; nothing else of ``out`` is written.  transposed: the data gradient of such a layer -- ``x`` is the gradient
    map, ``pack`` the data-gradient Res2Pack, and ``out`` has the layer's input size (a stride-2 layer in gather form)."""
    pack_ready(pack)
    N, IH, IW, xp = _res2_map(x)
    No, OH, OW, op = _res2_map(out)
    assert No == N, (x.shape, out.shape)
    ap = 0
    if add is not None:
        assert tuple(add.shape[:3]) == (N, IH, IW), (x.shape, add.shape)
        ap = _res2_map(add)[3]
    _lib.call('cpr_res2_conv_fwd', _ptr(x), xp, x_off, _ptr(add), ap, add_off, _ptr(pack.w), _ptr(out), op, out_off, _ptr(scale),
              _ptr(bias), N, IH, IW, OH, OW, pack.width, stride, int(bool(transposed)), CONV_RELU if relu else 0, _stream())
    if TRACE_CONV_VARIANT[0]:
        TRACE_CONV_VARIANT[1] = ('res2', pack.width)
    return out


def res2_wgrad(dy, dy_off, x, x_off, width, stride=1, add=None, add_off=0, grad=None, out=None):
    """grad_w (width, width, 3, 3) of the slice conv: the dy slice against the x slice (+ add slice).  Accumulated into ``grad`` when
    given, written into ``out`` when given, else a new tensor.  The split over pixels is added up in a fixed order."""
    N, H, W, xp = _res2_map(x)
    Nd, OH, OW, dp = _res2_map(dy)
    assert Nd == N and (OH, OW) == ((H - 1) // max(stride, 1) + 1, (W - 1) // max(stride, 1) + 1), (dy.shape, x.shape, stride)
    ap = 0
    if add is not None:
        assert tuple(add.shape[:3]) == (N, H, W), (x.shape, add.shape)
        ap = _res2_map(add)[3]
    n = _lib.call('cpr_res2_conv_wgrad_workspace', N, OH, OW, width, positive=True)
    ws = torch.empty((n,), device=x.device, dtype=torch.float32)
    acc = grad is not None
    if grad is None:
        grad = out if out is not None else torch.empty((width, width, 3, 3), device=x.device, dtype=torch.float32)
    assert tuple(grad.shape) == (width, width, 3, 3) and grad.is_contiguous() and grad.dtype == torch.float32
    _lib.call('cpr_res2_conv_wgrad', _ptr(dy), dp, dy_off, _ptr(x), xp, x_off, _ptr(add), ap, add_off, _ptr(grad), _ptr(ws), N, H, W,
              width, stride, int(acc), _stream())
    return grad


def res2_pool(x, x_off, out, out_off, width, stride):
    """The last slice of a Bottle2neck: stride 2 -- AvgPool2d(3, 2, padding 1), divisor always 9 -- or stride 1 -- the copy -- of
    x[..., x_off : x_off + width] into out[..., out_off : out_off + width]."""
    N, H, W, xp = _res2_map(x)
    No, OH, OW, op = _res2_map(out)
    assert No == N and (OH, OW) == ((H - 1) // max(stride, 1) + 1, (W - 1) // max(stride, 1) + 1), (x.shape, out.shape, stride)
    _lib.call('cpr_res2_pool_fwd', _ptr(x), xp, x_off, _ptr(out), op, out_off, N, H, W, width, stride, _stream())
    return out


def res2_pool_bwd(dy, dy_off, dx, dx_off, width, stride):
    """Its adjoint: dx[..., dx_off : dx_off + width] (the layer's input size) from dy[..., dy_off : dy_off + width]."""
    N, H, W, xp = _res2_map(dx)
    Nd, OH, OW, dp = _res2_map(dy)
    assert Nd == N and (OH, OW) == ((H - 1) // max(stride, 1) + 1, (W - 1) // max(stride, 1) + 1), (dy.shape, dx.shape, stride)
    _lib.call('cpr_res2_pool_bwd', _ptr(dy), dp, dy_off, _ptr(dx), xp, dx_off, N, H, W, width, stride, _stream())
    return dx


def res2_relu_bwd(g, g_off, y, y_off, width, carry=None, carry_off=0):
    """In place g[..., g_off : g_off + width] = (that slice (+ carry[..., carry_off : ...])) * (y[..., y_off : ...] > 0): the backward of a
    slice conv's ReLU with the gradient of the next conv's summed operand joining; returns the (width,) column sums of the result."""
    N, H, W, gp = _res2_map(g)
    assert tuple(y.shape[:3]) == (N, H, W) and (carry is None or tuple(carry.shape[:3]) == (N, H, W)), (g.shape, y.shape)
    yp = _res2_map(y)[3]
    cp = _res2_map(carry)[3] if carry is not None else 0
    M = N * H * W
    cs = torch.empty((width,), device=g.device, dtype=torch.float32)
    ws = torch.empty((_lib.call('cpr_res2_relu_bwd_colsum_ws', M, width, positive=True),), device=g.device, dtype=torch.float32)
    _lib.call('cpr_res2_relu_bwd_colsum', _ptr(g), gp, g_off, _ptr(carry), cp, carry_off, _ptr(y), yp, y_off, _ptr(cs), _ptr(ws), M, width,
              _stream())
    return cs


# ---- ResNeSt split attention, radix 2 (csrc/splat.hip).  u (N,H,W,2w) fp32: the block's 3x3 conv + bn0 + ReLU output, channel r*w + c =
# split r of channel c.  The C entry points check w % 4 == 0 and the ranges (include/cpr_hip.h) and raise CprHipError('... invalid
# argument') before any launch; the shapes of the operands against each other are checked here.
SPLAT_RADIX = 2


def _splat_map(u):
    assert u.dim() == 4 and u.shape[-1] % SPLAT_RADIX == 0, 'split attention: a (N,H,W,2w) map, got %s' % (tuple(u.shape),)
    N, H, W, C2 = _check(u).shape
    return N, H, W, C2 // SPLAT_RADIX


def _splat_pooled(H, W, pool):
    return ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if pool else (H, W)


def _splat_ws(u, rows, w):
    N, H, W, _ = u.shape
    k = _lib.call('cpr_splat_chunks', H, W, w, positive=True)
    return k, torch.empty((N * k * rows,), device=u.device, dtype=torch.float32)


def splat_dense_weight(weight):
    """The split-attention conv's parameter (2w, w/2, 3, 3) -- two groups, w/2 -> w each -- as the dense (2w, w, 3, 3) weight with exact
    zeros off the two diagonal blocks (the dense kernels' pack and data-gradient pack are built from it)."""
    O, I, KH, KW = weight.shape
    assert O == 4 * I, 'split-attention conv: a (2w, w/2, k, k) weight, got %s' % (tuple(weight.shape),)
    w = O // 2
    dense = torch.zeros((O, w, KH, KW), device=weight.device, dtype=torch.float32)
    dense[:w, :I].copy_(weight.detach()[:w])
    dense[w:, I:].copy_(weight.detach()[w:])
    return dense


def splat_gap(u):
    """g (N,w) = the mean over pixels of u[..., c] + u[..., w + c]."""
    N, H, W, w = _splat_map(u)
    _, ws = _splat_ws(u, w, w)
    g = torch.empty((N, w), device=u.device, dtype=torch.float32)
    _lib.call('cpr_splat_gap', _ptr(u), _ptr(g), _ptr(ws), N, H, W, w, _stream())
    return g


def splat_attn(g, fc1_w, fc1_b, scale, shift, fc2_w, fc2_b, record=False):
    """att (N,2,w) = the radix softmax of fc2(relu(scale * (fc1 g + b1) + shift)) + b2 (scale / shift: the folded eval BatchNorm);
    record: -> (att, z), z (N,inter) the ReLU's output."""
    N, w = _check(g).shape
    inter = fc1_w.shape[0]
    assert tuple(fc1_w.shape[:2]) == (inter, w) and fc1_w.numel() == inter * w, (fc1_w.shape, g.shape)
    assert tuple(fc2_w.shape[:2]) == (2 * w, inter) and fc2_w.numel() == 2 * w * inter, (fc2_w.shape, g.shape)
    assert fc1_b.numel() == scale.numel() == shift.numel() == inter and fc2_b.numel() == 2 * w
    for t in (fc1_w, fc1_b, scale, shift, fc2_w, fc2_b):
        _check(t)
    att = torch.empty((N, SPLAT_RADIX, w), device=g.device, dtype=torch.float32)
    z = torch.empty((N, inter), device=g.device, dtype=torch.float32) if record else None
    _lib.call('cpr_splat_attn', _ptr(g), _ptr(fc1_w), _ptr(fc1_b), _ptr(scale), _ptr(shift), _ptr(fc2_w), _ptr(fc2_b), _ptr(att), _ptr(z),
              N, w, inter, _stream())
    return (att, z) if record else att


def splat_apply(u, att, pool=False):
    """sum_r att[n,r,c] * u[n,p,r*w+c] (N,H,W,w), or with ``pool`` AvgPool2d(3, 2, padding=1) of it (divisor always 9), one launch."""
    N, H, W, w = _splat_map(u)
    assert tuple(_check(att).shape) == (N, SPLAT_RADIX, w), (att.shape, u.shape)
    OH, OW = _splat_pooled(H, W, pool)
    out = torch.empty((N, OH, OW, w), device=u.device, dtype=torch.float32)
    _lib.call('cpr_splat_apply', _ptr(u), _ptr(att), _ptr(out), N, H, W, w, int(bool(pool)), _stream())
    return out


def splat_attn_grad(dout, u, pool=False):
    """datt (N,2,w) = sum over pixels of dv * u[..., r*w + c]; dv = dout, or with ``pool`` the pool's adjoint of dout."""
    N, H, W, w = _splat_map(u)
    assert tuple(_check(dout).shape) == (N,) + _splat_pooled(H, W, pool) + (w,), (dout.shape, u.shape, pool)
    _, ws = _splat_ws(u, 2 * w, w)
    datt = torch.empty((N, SPLAT_RADIX, w), device=u.device, dtype=torch.float32)
    _lib.call('cpr_splat_attn_grad', _ptr(dout), _ptr(u), _ptr(datt), _ptr(ws), N, H, W, w, int(bool(pool)), _stream())
    return datt


def splat_attn_bwd(att, datt, z, g, fc1_w, fc1_b, scale, mean, inv_sigma, fc2_w, grads=None):
    """The attention MLP's backward -> dg (N,w).  grads: a dict of output tensors, any of 'fc1_w', 'fc1_b', 'bn_w', 'bn_b', 'fc2_w',
    'fc2_b' (written, images added in ascending order)."""
    N, w = _check(g).shape
    inter = fc1_w.shape[0]
    assert tuple(att.shape) == tuple(datt.shape) == (N, SPLAT_RADIX, w) and tuple(z.shape) == (N, inter), (att.shape, datt.shape, z.shape)
    assert fc1_w.numel() == inter * w and fc2_w.numel() == 2 * w * inter
    assert fc1_b.numel() == scale.numel() == mean.numel() == inv_sigma.numel() == inter
    for t in (att, datt, z, fc1_w, fc1_b, scale, mean, inv_sigma, fc2_w):
        _check(t)
    grads = grads or {}
    shapes = dict(fc1_w=inter * w, fc1_b=inter, bn_w=inter, bn_b=inter, fc2_w=2 * w * inter, fc2_b=2 * w)
    for k, t in grads.items():
        assert _check(t).numel() == shapes[k], (k, t.shape)
    dg = torch.empty((N, w), device=g.device, dtype=torch.float32)
    ws = torch.empty((N * (2 * w + 3 * inter),), device=g.device, dtype=torch.float32)
    _lib.call('cpr_splat_attn_bwd', _ptr(att), _ptr(datt), _ptr(z), _ptr(g), _ptr(fc1_w), _ptr(fc1_b), _ptr(scale), _ptr(mean),
              _ptr(inv_sigma), _ptr(fc2_w), _ptr(dg), _ptr(ws), _ptr(grads.get('fc1_w')), _ptr(grads.get('fc1_b')), _ptr(grads.get('bn_w')),
              _ptr(grads.get('bn_b')), _ptr(grads.get('fc2_w')), _ptr(grads.get('fc2_b')), N, w, inter, _stream())
    return dg


def splat_apply_bwd(dout, u, att, dg, pool=False):
    """du (N,H,W,2w) = (att[n,r,c] * dv + dg[n,c] / (H*W)) * (u > 0) and its (2w,) column sums -> (du, colsum)."""
    N, H, W, w = _splat_map(u)
    assert tuple(_check(dout).shape) == (N,) + _splat_pooled(H, W, pool) + (w,), (dout.shape, u.shape, pool)
    assert tuple(_check(att).shape) == (N, SPLAT_RADIX, w) and tuple(_check(dg).shape) == (N, w), (att.shape, dg.shape)
    k = _lib.call('cpr_splat_chunks', H, W, w, positive=True)
    ws = torch.empty((N * k * 2 * w + N * 2 * w,), device=u.device, dtype=torch.float32)
    du = torch.empty_like(u)
    cs = torch.empty((2 * w,), device=u.device, dtype=torch.float32)
    _lib.call('cpr_splat_apply_bwd', _ptr(dout), _ptr(u), _ptr(att), _ptr(dg), _ptr(du), _ptr(cs), _ptr(ws), N, H, W, w, int(bool(pool)),
              _stream())
    return du, cs


# ---- MobileNetV2 (csrc/mbv2.hip): the depthwise 3x3 conv (forward, data gradient, weight gradient) and the ReLU6 passes.  Maps are NHWC
# fp32 at the pitch pad32(C), C % 8 == 0, pad channels exact zeros (never read of an input, written as +0.0 of an output).  The C entry
# points check shapes, strides and flag bits (include/cpr_hip.h) and raise CprHipError('... invalid argument') before any launch.
DW_IN_CLAMP6, DW_RELU6 = 1, 2


class DwPack:
    """A depthwise (C, 1, 3, 3) parameter as the kernels read it (cpr_dw3x3_pack): [9][pad32(C)] floats, tap-major, pad channels zero,
    ``scale`` (C) multiplied in -- the data-gradient pack carries the folded BatchNorm scale.  ``repack`` runs the same kernel on the same
    buffer (nothing calls it after construction today: the backbone's packs lapse with the weight epoch and are rebuilt)."""

    def __init__(self, weight, scale=None):
        C, one, KH, KW = weight.shape
        assert weight.is_cuda, 'the depthwise pack is built on the device'
        assert (one, KH, KW) == (1, 3, 3), 'depthwise conv: a (C, 1, 3, 3) weight, got %s' % (tuple(weight.shape),)
        self.C, self.Cp = C, pad32(C)
        self.w = torch.empty((9 * self.Cp,), device=weight.device, dtype=torch.float32)
        self.repack(weight, scale)

    def repack(self, weight, scale=None):
        src = weight.detach()
        if src.dtype != torch.float32 or not src.is_contiguous():
            src = src.float().contiguous()
        if scale is not None:
            assert _check(scale).numel() == self.C, (scale.shape, self.C)
        _lib.call('cpr_dw3x3_pack', _ptr(src), _ptr(scale), _ptr(self.w), self.C, _stream())
        self.ready = record_ready()
        return self


def _dw_map(t, C):
    N, H, W, Cp = _check(t).shape
    assert Cp == pad32(C), 'a map of %d channels sits at pitch %d, got %s' % (C, pad32(C), tuple(t.shape))
    return N, H, W


def _dw_out_hw(H, W, stride):
    return (H - 1) // max(stride, 1) + 1, (W - 1) // max(stride, 1) + 1


def dw_conv(x, pack, stride=1, scale=None, bias=None, in_clamp6=False, relu6=False, out=None):
    """out (N,OH,OW,Cp) = act(scale * dwconv3x3(in(x), pack) + bias), padding 1; in_clamp6: x is read as min(x, 6) (its producer wrote
    ReLU(v)); relu6: act = min(max(., 0), 6); scale / bias (C) None and no flag: the raw form."""
    pack_ready(pack)
    N, H, W = _dw_map(x, pack.C)
    OH, OW = _dw_out_hw(H, W, stride)
    if out is None:
        out = torch.empty((N, OH, OW, pack.Cp), device=x.device, dtype=torch.float32)
    assert tuple(_check(out).shape) == (N, OH, OW, pack.Cp), (out.shape, x.shape, stride)
    for v in (scale, bias):
        assert v is None or _check(v).numel() == pack.C, (v.shape, pack.C)
    _lib.call('cpr_dw3x3_fwd', _ptr(x), _ptr(pack.w), _ptr(scale), _ptr(bias), _ptr(out), N, H, W, pack.C, stride,
              (DW_IN_CLAMP6 if in_clamp6 else 0) | (DW_RELU6 if relu6 else 0), _stream())
    if TRACE_CONV_VARIANT[0]:
        TRACE_CONV_VARIANT[1] = ('dw', pack.C)
    return out


def dw_dgrad(dy, pack, in_hw, stride=1, mask6=None, add=None, colsum=False, out=None):
    """The data gradient of dw_conv in gather form: dy (N,OH,OW,Cp), ``pack`` the DwPack of the folded weight scale * w -> dx (N,H,W,Cp),
    (H, W) = in_hw.  add (dx's shape) is summed in, then mask6 (dx's shape, the ReLU(v) map the layer read with in_clamp6) keeps the
    elements with 0 < mask6 < 6.  colsum: -> (dx, the (C,) per-channel sums of dx).  out: dx is written there (every element, pad
    channels as +0.0)."""
    pack_ready(pack)
    H, W = in_hw
    N, OH, OW = _dw_map(dy, pack.C)
    assert (OH, OW) == _dw_out_hw(H, W, stride), (dy.shape, in_hw, stride)
    dx = out if out is not None else torch.empty((N, H, W, pack.Cp), device=dy.device, dtype=torch.float32)
    assert tuple(_check(dx).shape) == (N, H, W, pack.Cp), (dx.shape, dy.shape, in_hw)
    for v in (mask6, add):
        assert v is None or tuple(_check(v).shape) == tuple(dx.shape), (v.shape, dx.shape)
    cs = ws = None
    if colsum:
        cs = torch.empty((pack.C,), device=dy.device, dtype=torch.float32)
        ws = torch.empty((_lib.call('cpr_dw3x3_dgrad_workspace', N, H, W, pack.C, positive=True),), device=dy.device, dtype=torch.float32)
    _lib.call('cpr_dw3x3_dgrad', _ptr(dy), _ptr(pack.w), _ptr(add), _ptr(mask6), _ptr(dx), _ptr(cs), _ptr(ws), N, H, W, pack.C, stride,
              _stream())
    return (dx, cs) if colsum else dx


def dw_wgrad(dy, x, C, stride=1, in_clamp6=False, grad=None, out=None):
    """grad_w (C, 1, 3, 3) of dw_conv: dy (N,OH,OW,Cp) against in(x), x (N,H,W,Cp).  Accumulated into ``grad`` when given (one more
    rounded addition), written into ``out`` when given, else a new tensor.  The split over pixels is added up in a fixed order."""
    N, H, W = _dw_map(x, C)
    assert (N,) + _dw_out_hw(H, W, stride) == _dw_map(dy, C), (dy.shape, x.shape, stride)
    ws = torch.empty((_lib.call('cpr_dw3x3_wgrad_workspace', N, H, W, C, stride, positive=True),), device=x.device, dtype=torch.float32)
    acc = grad is not None
    if grad is None:
        grad = out if out is not None else torch.empty((C, 1, 3, 3), device=x.device, dtype=torch.float32)
    assert tuple(grad.shape) == (C, 1, 3, 3) and grad.is_contiguous() and grad.dtype == torch.float32
    _lib.call('cpr_dw3x3_wgrad', _ptr(dy), _ptr(x), _ptr(grad), _ptr(ws), N, H, W, C, stride, int(bool(in_clamp6)), int(acc), _stream())
    return grad


def relu6_bwd_colsum(dy, y=None, add=None, want_g=True, out=None):
    """g = (dy (+ add)) * (0 < y < 6) and the per-channel column sums of g -> (g | None, colsum (C)): the ReLU6 twin of relu_bwd_colsum.
    y: the clamped map or the ReLU(v) map the forward recorded (the predicate is the same).  y None: the column sums of dy alone.
    out (with y): g is written there, every element."""
    C = dy.shape[-1]
    M = dy.numel() // C
    for v in (y, add):
        assert v is None or (_check(v).numel() == dy.numel()), (v.shape, dy.shape)
    assert y is not None or add is None
    g = None
    if want_g and y is not None:
        g = out if out is not None else torch.empty_like(dy)
        assert _check(g).shape == dy.shape, (g.shape, dy.shape)
    cs = torch.empty((C,), device=dy.device, dtype=torch.float32)
    ws = torch.empty((_lib.call('cpr_relu6_bwd_colsum_ws', M, C, positive=True),), device=dy.device, dtype=torch.float32)
    _lib.call('cpr_relu6_bwd_colsum', _ptr(_check(dy)), _ptr(add), _ptr(y), _ptr(g), _ptr(cs), _ptr(ws), M, C, _stream())
    return (dy if (y is None and want_g) else g), cs


def clamp6(x):
    """x = min(x, 6) in place: a ReLU(v) map whose consumers do not clamp on load (a stage output, conv2's output)."""
    _lib.call('cpr_clamp6', _ptr(_check(x)), x.numel(), _stream())
    return x


# ---- Darknet (csrc/darknet.hip): the LeakyReLU passes around the dense convs (whose epilogues know ReLU only) and the weight gradient
# of the 3 -> 32 / stride 1 first conv.  fp32 NHWC maps; nothing here has a bf16 form.
def leaky(z, slope, res=None, out=None):
    """out = F.leaky_relu(z, slope) (+ res), bit for bit (the product is rounded, then the sum).  out None: in place, z is returned;
    res: a map of z's shape (a ResBlock's shortcut)."""
    if out is None:
        out = z
    assert _check(out).shape == _check(z).shape and (res is None or _check(res).shape == z.shape), (z.shape, out.shape)
    _lib.call('cpr_leaky_fwd', _ptr(z), _ptr(res), _ptr(out), z.numel(), float(slope), _stream())
    return out


def leaky_bwd_colsum(dy, y, slope, add=None, want_g=True, out=None):
    """g = (y > 0 ? s : s * slope) with s = dy (+ add) and the per-channel column sums of g -> (g | None, colsum (C)): the LeakyReLU
    twin of relu_bwd_colsum / relu6_bwd_colsum.  y: the pre-activation or the activated map (the predicate is the same).  out: g is
    written there, every element."""
    C = dy.shape[-1]
    M = dy.numel() // C
    for v in (y, add):
        assert v is None or (_check(v).numel() == dy.numel()), (v.shape, dy.shape)
    g = None
    if want_g:
        g = out if out is not None else torch.empty_like(dy)
        assert _check(g).shape == dy.shape, (g.shape, dy.shape)
    ws = torch.empty((_lib.call('cpr_leaky_bwd_colsum_ws', M, C, positive=True),), device=dy.device, dtype=torch.float32)
    cs = torch.empty((C,), device=dy.device, dtype=torch.float32)
    _lib.call('cpr_leaky_bwd_colsum', _ptr(_check(dy)), _ptr(add), _ptr(y), _ptr(g), _ptr(cs), _ptr(ws), M, C, float(slope), _stream())
    return g, cs


def stem3x3s1_wgrad(dy, x, planar=None, out=None):
    """Weight gradient of Darknet's first conv (3x3 / stride 1 / padding 1, 3 -> 32): dy (N,H,W,32) fp32 and the image as the forward
    read it (NHWC4, or the (N,3,H,W) planes) -> (32,3,3,3) fp32 (written into ``out`` when given); the split over pixels is added up
    in a fixed order (csrc/darknet.hip)."""
    N, H, W, layout = _stem_input(_check(x), planar)
    assert _check(dy).shape == (N, H, W, 32), (tuple(dy.shape), tuple(x.shape))
    if out is None:
        out = torch.empty((32, 3, 3, 3), device=x.device, dtype=torch.float32)
    assert _check(out).shape == (32, 3, 3, 3), tuple(out.shape)
    ws = torch.empty((_lib.call('cpr_stem3x3s1_wgrad_workspace', N, H, W, positive=True),), device=x.device, dtype=torch.float32)
    _lib.call('cpr_stem3x3s1_wgrad', _ptr(dy), _ptr(x), _ptr(out), _ptr(ws), N, H, W, layout, _stream())
    return out


# ---- CTResNetNeck (csrc/deconv.hip): the transposed convolution 4x4 / stride 2 / padding 1 without bias.  fp32 NHWC; no bf16 form.
class DeconvPack:
    """An nn.ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1, bias=False) weight (Cin, Cout, 4, 4) repacked for ``deconv4x4s2``: one
    [Cout][4 * Cin] GEMM image per output-parity class (a, b), K ordered (tap row, tap column, cin) -- self.w (4, Cout, 4 * Cin) with
    w[2a + b, co, (2t + u) * Cin + ci] = weight[ci, co, 1 - a + 2t, 1 - b + 2u]."""
    ready = None

    def __init__(self, weight):
        Cin, Cout, KH, KW = weight.shape
        assert (KH, KW) == (4, 4), 'the transposed-conv kernel is 4x4 / stride 2 / padding 1, got a %dx%d weight' % (KH, KW)
        assert weight.is_cuda, 'the transposed-conv pack is built on the device'
        self.Cin, self.Cout, self.dtype = Cin, Cout, torch.float32
        src = weight.detach()
        if src.dtype != torch.float32 or not src.is_contiguous():
            src = src.float().contiguous()
        self.w = torch.empty((4, Cout, 4 * Cin), device=weight.device, dtype=torch.float32)
        _lib.call('cpr_pack_weights_deconv', _ptr(src), _ptr(self.w), Cin, Cout, _stream())
        self.ready = record_ready()


def deconv_pack_image(weight):
    """The image ``DeconvPack`` holds, restated with torch on any device: (4, Cout, 4 * Cin) from the (Cin, Cout, 4, 4) weight (the host
    tests and the device test of the pack kernel read it)."""
    Cin, Cout = weight.shape[:2]
    return torch.stack([torch.stack([weight[:, :, 1 - a + 2 * t, 1 - b + 2 * u].t() for t in range(2) for u in range(2)], 1).reshape(Cout, 4 * Cin)
                        for a in range(2) for b in range(2)])


def deconv4x4s2(x, pack, scale=None, bias=None, relu=False, out=None):
    """x (N,H,W,Cin) fp32 -> (N,2H,2W,Cout) = F.conv_transpose2d(x, weight, stride=2, padding=1) in NHWC, one launch for the four
    output-parity classes, written interleaved (no scatter pass, no atomics; bit-repeatable and independent of the batch).
    Epilogue: * scale[c] + bias[c] (ReLU) -- eval-mode BatchNorm folded; with neither operand the raw sums."""
    N, H, W, Cin = _check(x).shape
    assert Cin == pack.Cin, (Cin, pack.Cin)
    pack_ready(pack)
    if out is None:
        out = torch.empty((N, 2 * H, 2 * W, pack.Cout), device=x.device, dtype=torch.float32)
    assert tuple(_check(out).shape) == (N, 2 * H, 2 * W, pack.Cout)
    for v in (scale, bias):
        assert v is None or _check(v).numel() == pack.Cout
    variant = ctypes.c_int(0) if TRACE_CONV_VARIANT[0] else None
    _lib.call('cpr_deconv4x4s2_fwd', _ptr(x), _ptr(pack.w), _ptr(out), _ptr(scale), _ptr(bias), N, H, W, Cin, pack.Cout,
              CONV_RELU if relu else 0, ctypes.byref(variant) if variant is not None else None, _stream())
    if variant is not None:
        TRACE_CONV_VARIANT[1] = ('deconv', variant.value)
    return out


def deconv4x4s2_dgrad_pack(weight):
    """The pack of the data gradient of ``deconv4x4s2``: dx = conv2d(dy, weight, stride 2, padding 1) with the SAME tensor read as
    (out = Cin, in = Cout, 4, 4) -- a plain forward pack."""
    return PackedConv(weight, 2, 1)


def deconv4x4s2_wgrad(dy, x, weight_shape, grad=None, out=None):
    """Weight gradient (Cin, Cout, 4, 4) of ``deconv4x4s2``: the dense conv's weight gradient with the roles of the maps swapped -- the
    'conv' reads dy (N,2H,2W,Cout) at stride 2 / padding 1 and writes x (N,H,W,Cin)."""
    return conv2d_wgrad(x, dy, weight_shape, 2, 1, grad=grad, out=out)
