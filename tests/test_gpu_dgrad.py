"""-m gpu: the dense conv data gradient on every route it takes, pinned by the route and checked against the fp64 reference of
tests/dgrad_fp64_ref.py (written from the forward definition) at the bars derived there: the transpose / flip / scale pack and its
padding d (K - 1) - p, PhasedDgrad's per-parity taps, offsets and scatter, the zero-insertion extent, the composition rules of
ops.conv2d_dgrad (which operand rides the epilogue, when mask / add / column sums fall to relu_bwd_colsum, when a plain 3x3 takes the
Winograd route), the Cout <= 4 pack, and the bf16 forms the mixed-precision trainer feeds with PackedConv.for_dgrad_bf16 packs.

A case is (N, Cin, H, W, Cout, k, s, p, flags, route) of the FORWARD conv: dy is (N, OH, OW, Cout), dx is (N, H, W, Cin).
flags: scale (folded BatchNorm scale in the pack), add, mask, colsum, bf16, fused (conv2d_dgrad_bf16_fused), nophase (ops._PHASED off:
the zero-insertion form).  Routes: phased, zero-insert, wino, fp32 direct, fp32 streamed 1x1, bf16 <variant word>.

Packs are built as layers.dgrad_packed builds them (ops.dgrad_pack; bf16 stride 1: PackedConv.for_dgrad_bf16) and run as the trainer
runs them: fp32 through ops.conv2d_dgrad; bf16 stride 1 through ops.conv2d (fp32 out, or the mask mode) or
ops.conv2d_dgrad_bf16_fused; bf16 stride 2 by calling the PhasedDgrad (ops.conv2d_dgrad itself takes fp32 gradients only).
Cout <= 4: the pack has four columns and dy four channels; the channels past Cout hold nonzero values here, which the pack's zero
columns must cancel.  The large cases (bf16 LDS-DMA instances, the streamed 1x1) are checked on sampled pixels and whole column-sum
slots; their reduced column sums and EVERY slot are held against dgrad_fp64_ref.tap_scatter (fp64 on the device), pinned to the sampled
reference.  The streamed 1x1 case (64 -> 256 on 2 x 256 x 256, 1024 tiles: the smallest its rule takes) stays within a few seconds."""
import numpy as np
import pytest
import torch

from tests import dgrad_fp64_ref as D
from tests.conv_fp64_ref import sample_pixels
from tests.test_gpu_bf16 import BIG, FUSED_CASES, MASK_CASES, PP, SMALL
from tests.test_gpu_conv_instances import BF, F32, predict_variant

B_SMALL, B_BIG, B_PP = 'bf16 %d' % SMALL, 'bf16 %d' % BIG, 'bf16 %d' % PP
ROUTES = ['phased', 'zero-insert', 'wino', 'fp32 direct', 'fp32 streamed 1x1', 'bf16 64064', B_SMALL, B_BIG, B_PP]


def _mask_case(t):      # test_gpu_bf16.MASK_CASES name the pack: (N, pack Cin, H, W, pack Cout, k, fp32 out, instance)
    N, pcin, H, W, pcout, k, _, want = t
    return (N, pcout, H, W, pcin, k, 1, k // 2, 'bf16 scale mask colsum', 'bf16 %d' % want)


def _fused_case(t):     # test_gpu_bf16.FUSED_CASES: (N, pack Cin, H, W, pack Cout, instance), 1x1
    N, pcin, H, W, pcout, want = t
    return (N, pcout, H, W, pcin, 1, 1, 0, 'bf16 scale fused', 'bf16 %d' % want)


CASES = [
    # ---- fp32, stride 1
    (3, 256, 13, 11, 64, 1, 1, 0, '', 'fp32 direct'),                          # bottleneck conv1, ragged M = 429
    (3, 256, 13, 11, 64, 1, 1, 0, 'scale', 'fp32 direct'),
    (3, 256, 13, 11, 64, 1, 1, 0, 'scale colsum', 'fp32 direct'),              # column sums alone in the epilogue
    (3, 256, 13, 11, 64, 1, 1, 0, 'mask', 'fp32 direct'),                      # the mask alone (FC tower)
    (3, 256, 13, 11, 64, 1, 1, 0, 'scale mask colsum', 'fp32 direct'),
    (3, 256, 13, 11, 64, 1, 1, 0, 'scale add', 'fp32 direct'),
    (3, 256, 13, 11, 64, 1, 1, 0, 'scale mask add colsum', 'fp32 direct'),     # the epilogue add, then a streaming mask
    (1, 512, 9, 7, 2048, 1, 1, 0, '', 'fp32 direct'),                          # long K
    (2, 256, 9, 11, 4, 1, 1, 0, 'scale', 'fp32 direct'),                       # the cols_p = 4 pack
    (2, 256, 9, 11, 4, 1, 1, 0, 'mask', 'fp32 direct'),                        # ... as the logit projection runs it
    (2, 256, 9, 11, 2, 1, 1, 0, 'scale', 'fp32 direct'),                       # the pack's zero-padded columns
    (2, 64, 17, 15, 96, 3, 1, 1, 'scale mask colsum', 'fp32 direct'),          # borders, Cout 96
    (2, 64, 17, 15, 96, 3, 1, 1, 'add', 'fp32 direct'),
    (2, 64, 17, 15, 96, 3, 1, 1, 'scale add colsum', 'fp32 direct'),           # the add and the column sums in one epilogue
    (1, 64, 32, 29, 128, 3, 1, 1, '', 'wino'),                                 # fill 0.91, 8 x 16 regions
    (1, 64, 48, 40, 64, 3, 1, 1, 'scale', 'wino'),                             # the scaled pack through G g G^T, 16 x 16 regions
    (1, 64, 32, 29, 128, 3, 1, 1, 'mask', 'fp32 direct'),                      # must leave the Winograd route
    (2, 64, 256, 256, 256, 1, 1, 0, 'mask', 'fp32 streamed 1x1'),              # K = 256, 1024 tiles
    # ---- fp32, stride 2: phase-decomposed
    (2, 128, 17, 14, 128, 3, 2, 1, 'scale', 'phased'),
    (2, 128, 17, 14, 128, 3, 2, 1, 'scale add', 'phased'),
    (2, 128, 17, 14, 128, 3, 2, 1, 'scale mask colsum', 'phased'),
    (2, 128, 17, 14, 128, 3, 2, 1, 'scale mask add colsum', 'phased'),
    (2, 128, 14, 17, 128, 3, 2, 1, 'scale', 'phased'),
    (2, 128, 14, 17, 128, 3, 2, 1, 'scale add', 'phased'),
    (2, 128, 14, 17, 128, 3, 2, 1, 'scale mask colsum', 'phased'),
    (2, 256, 15, 13, 512, 1, 2, 0, '', 'phased'),
    (2, 256, 15, 13, 512, 1, 2, 0, 'scale colsum', 'phased'),                  # column sums alone: a streaming pass that keeps dx
    (2, 256, 14, 16, 512, 1, 2, 0, '', 'phased'),                              # the last row and column: never read, exactly 0
    (2, 256, 14, 16, 512, 1, 2, 0, 'add', 'phased'),                           # ... exactly the add
    (1, 64, 1, 5, 64, 3, 2, 1, '', 'phased'),                                  # a parity class with no rows
    (2, 64, 1, 5, 64, 3, 2, 1, '', 'phased'),                                  # ... in two images
    (2, 64, 3, 2, 64, 3, 2, 1, '', 'phased'),                                  # a map smaller than the taps
    # ---- fp32, stride 2: zero insertion
    (2, 128, 17, 14, 128, 3, 2, 1, 'scale nophase', 'zero-insert'),
    (2, 128, 14, 17, 128, 3, 2, 1, 'scale add nophase', 'zero-insert'),
    (2, 128, 17, 14, 128, 3, 2, 1, 'scale mask colsum nophase', 'zero-insert'),
    (2, 256, 14, 16, 512, 1, 2, 0, 'nophase', 'zero-insert'),                  # (He, We) = (H, W) past (O - 1) s
    # ---- bf16
    (2, 256, 13, 11, 64, 1, 1, 0, 'bf16 scale', 'bf16 64064'),
    (2, 64, 17, 15, 128, 3, 1, 1, 'bf16 scale', 'bf16 64064'),
    _mask_case(MASK_CASES[0]),                                                 # 3x3, 128 x 128 tile
    _mask_case(MASK_CASES[4]),                                                 # 1x1, weights direct to registers, ragged
    _fused_case(FUSED_CASES[0]), _fused_case(FUSED_CASES[1]), _fused_case(FUSED_CASES[2]),
    (2, 128, 17, 15, 128, 3, 2, 1, 'bf16 scale add', 'phased'),
    (2, 256, 15, 13, 512, 1, 2, 0, 'bf16 scale', 'phased'),
]


def case_id(c):
    return 'n%d_c%d_%dx%d_o%d_k%d_s%d_p%d_%s' % (c[:8] + (c[8].replace(' ', '-') or 'plain',))


def flags(c):
    return c[8].split()


def is_large(c):
    """Checked on sampled pixels (and the device fp64 map for the reduced column sums), not on the whole map."""
    return c[0] * c[2] * c[3] >= 10000


# ---- the route rules, restated (the CPU test checks every case's route against them) ---------------------------------------
def _cdiv(a, b):
    return (a + b - 1) // b


def inner_conv(c):
    """The forward-conv case (tests.test_gpu_conv_instances) of the stride-1 conv over dy that a non-phased data gradient launches:
    PackedConv.for_dgrad / for_dgrad_bf16 (Cin = the forward's Cout, 4 columns for Cout <= 4; Cout = the forward's Cin; padding
    K - 1 - p) over dy, or over the zero-inserted map of extent (H + 2p - K + 1) for a strided layer; ops.conv2d_dgrad hands the
    epilogue the mask OR the add (both: the add, the mask is a streaming pass)."""
    N, Cin, H, W, Cout, k, s, p, _, _ = c
    f = flags(c)
    if s == 1:
        ih, iw = D.out_hw(H, W, k, s, p)
    else:
        ih, iw = H + 2 * p - k + 1, W + 2 * p - k + 1
    if 'bf16' in f:
        fl = 'bf16mask' if ('mask' in f or 'fused' in f) else 'f32out'
        return BF(N, ih, iw, Cout, Cin, k, 1, k - 1 - p, fl, None)
    mask, add, colsum = 'mask' in f, 'add' in f, 'colsum' in f
    if mask and add:
        fl = 'res'
    elif mask:
        fl = 'mask' if colsum else 'resmask'
    elif add:
        fl = 'res mask' if colsum else 'res'
    else:
        fl = 'mask' if colsum else ''
    return F32(N, ih, iw, 4 if Cout <= 4 else Cout, Cin, k, 1, k - 1 - p, fl, None)


def predict_route(c):
    """(route, variant of the last conv launch or None) -- a restatement of ops.dgrad_pack (the phased rule), ops.conv2d_dgrad,
    ops.conv2d / wino_eligible / wino_instance and, through predict_variant, the launchers' tile rules."""
    N, Cin, H, W, Cout, k, s, p, _, _ = c
    f = flags(c)
    if s == 2 and k in (1, 3) and p == k // 2 and 'nophase' not in f:
        return 'phased', None
    v = predict_variant(inner_conv(c))
    if v is not None and v[0] == 'wino':
        v = ('wino32' if H * W <= 40 * 40 else 'wino', 0)
    if s > 1:
        return 'zero-insert', v
    if v is None:
        return None, None
    if v[0] in ('wino', 'wino32'):
        return 'wino', v
    if v[0] == 'bf16':
        return 'bf16 %d' % v[1], v
    return ('fp32 streamed 1x1' if v[1] % 10 == 3 else 'fp32 direct'), v


def slot_pixels(c, variant):
    """Pixels per column-sum slot where the route returns TilePartials (None: a reduced vector from relu_bwd_colsum, or none)."""
    f = flags(c)
    if 'colsum' not in f and 'fused' not in f:
        return None
    if 'bf16' in f:
        return 128          # conv_bf16_dma.h: one slot per 128 pixels in the mask mode (bf16 out) and in the fused form
    if ('mask' in f and 'add' in f) or c[9] == 'phased':
        return None
    return variant[1] // 1000000      # fp32 epilogue partials: one slot per M tile


# ---- inputs: seeded CPU generators (the CPU test looks at the masks) ---------------------------------------------------------
def seed(c):
    return (sum(v * w for v, w in zip(c[:8], (7, 3, 131, 17, 5, 11, 13, 19))) + sum(map(ord, c[8]))) % 100003


def make_mask(c):
    """The forward's post-ReLU input: the ReLU of a seeded normal (exact +0.0 where it was negative), -0.0 planted at every 1013th
    element, bf16 for the bf16 forms."""
    N, Cin, H, W = c[:4]
    g = torch.Generator().manual_seed(seed(c) + 1)
    m = torch.randn((N, H, W, Cin), generator=g).clamp_min_(0)
    m.view(-1)[::1013] = -0.0
    return m.bfloat16() if 'bf16' in flags(c) else m


def make_inputs(c):
    N, Cin, H, W, Cout, k, s, p, _, _ = c
    f = flags(c)
    OH, OW = D.out_hw(H, W, k, s, p)
    g = torch.Generator().manual_seed(seed(c))
    dy = torch.randn((N, OH, OW, 4 if Cout <= 4 else Cout), generator=g)
    w = torch.randn((Cout, Cin, k, k), generator=g) / (Cin * k * k) ** 0.5
    scale = (torch.rand(Cout, generator=g) + 0.5) if 'scale' in f else None
    add = torch.randn((N, H, W, Cin), generator=g) if ('add' in f or 'fused' in f) else None
    mask = make_mask(c) if ('mask' in f or 'fused' in f) else None
    return dict(dy=dy, w=w, scale=scale, add=add, mask=mask)


# ---- the GPU run ------------------------------------------------------------------------------------------------------------
def _run(c, inp):
    from pointtinybenchmark_amd import ops
    N, Cin, H, W, Cout, k, s, p, _, _ = c
    f = flags(c)
    cuda = (lambda t: None if t is None else t.cuda())
    dy, w, scale, add, mask = (cuda(inp[n]) for n in ('dy', 'w', 'scale', 'add', 'mask'))
    out16 = cs = None
    ops.TRACE_CONV_VARIANT[0], ops.TRACE_CONV_VARIANT[1] = True, None
    ops._PHASED[0] = 'nophase' not in f
    try:
        if 'bf16' in f:
            dy = dy.bfloat16()
            if s == 1:
                pt = ops.PackedConv.for_dgrad_bf16(w, p, scale=scale)
                if 'fused' in f:
                    out, out16, cs = ops.conv2d_dgrad_bf16_fused(dy, pt, mask, add)
                elif 'mask' in f:
                    assert ops.conv2d_bf16_mask_slots(dy.shape, pt) > 0
                    out16, cs = ops.conv2d(dy, pt, residual=mask, res_mask=True, colsum=True)
                    out = None
                else:
                    out = ops.conv2d(dy, pt, out_dtype=torch.float32)
            else:
                pt = ops.dgrad_pack(w, s, p, scale=scale, dtype=torch.bfloat16)
                out = pt(dy, (H, W), add=add)
        else:
            pt = ops.dgrad_pack(w, s, p, scale=scale)
            out = ops.conv2d_dgrad(dy, pt, (H, W), s, mask=mask if 'mask' in f else None, add=add, colsum='colsum' in f)
            if 'colsum' in f:
                out, cs = out
        variant = ops.TRACE_CONV_VARIANT[1]
        torch.cuda.synchronize()
    finally:
        ops.TRACE_CONV_VARIANT[0] = False
        ops._PHASED[0] = True
    if isinstance(pt, ops.PhasedDgrad):
        route = 'phased'
        assert pt.dtype == (torch.bfloat16 if 'bf16' in f else torch.float32) and variant[0] == ('bf16' if 'bf16' in f else 'fp32')
    elif s > 1:
        route = 'zero-insert'
    elif variant[0] in ('wino', 'wino32'):
        route = 'wino'
    elif variant[0] == 'bf16':
        route = 'bf16 %d' % variant[1]
    else:
        route = 'fp32 streamed 1x1' if variant[1] % 10 == 3 else 'fp32 direct'
    part = None
    if cs is not None and hasattr(cs, 'reduce'):
        part, cs = cs.part, cs.reduce()
        torch.cuda.synchronize()
    return dict(out=out, out16=out16, cs=cs, part=part, route=route, variant=variant, dy=dy)


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_dgrad_route_vs_fp64(c):
    N, Cin, H, W, Cout, k, s, p, _, want = c
    f = flags(c)
    name = case_id(c)
    inp = make_inputs(c)
    g = _run(c, inp)
    assert g['route'] == want, 'expected route %r, took %r (last launch %r)' % (want, g['route'], g['variant'])
    inner = predict_route(c)[1]
    assert inner is None or g['variant'] == inner, 'expected the launch %r, the launcher chose %r' % (inner, g['variant'])
    bf = 'bf16' in f
    M = N * H * W
    slot = slot_pixels(c, g['variant'])
    assert (slot is not None) == (g['part'] is not None), 'column sums: TilePartials %s' % ('expected' if slot else 'not expected')
    large = is_large(c)
    dy = g['dy'][..., :Cout]                     # bf16 cases: as the kernel read it
    ws = D.bf16_operands(dy, inp['w'], inp['scale'])[1] if bf else D.scaled_weights(inp['w'], inp['scale'])
    add, mask = inp['add'], inp['mask']
    kw = dict(scaled='scale' in f, bf16=bf, wino=want == 'wino')
    if large:
        bm = 256 if want in (B_BIG, B_PP) else 128
        m, slots = sample_pixels(N, H, W, bm, slot=slot, seed=M % 9973)
        t, mag = D.gather(dy, ws, s, p, (H, W), m)
    else:
        m, slots = np.arange(M), (list(range(_cdiv(M, slot))) if slot else [])
        t, mag = D.full_map(dy, ws, s, p, (H, W))
    if want == 'wino':
        kw['mag_wino'] = D.wino_magnitude(dy, ws, m)
    r = D.finish(t, mag, None if add is None else D.rows(add, m), None if mask is None else D.rows(mask, m), **kw)
    worst = worst16 = worst_s = worst_cs = 0.0
    if g['out'] is not None:
        got = D.rows(g['out'], m)
        worst = D.check(name, got, r['ref'], r['bar32'], m=m, OHW=(H, W))
        if want == 'wino':      # the per-element Winograd bound beside the whole-map one
            print('\nDGRAD wino per-element bound: worst %.4f' % D.check(name + ' Winograd bound', got, r['ref'], r['bar_wino'], m=m, OHW=(H, W)))
        # pixels no tap reaches (the odd rows and columns of a 1x1 / stride 2 layer, the last row and column of its even map among
        # them: the forward never read them): exactly 0, or exactly the add
        dead = (mag == 0).all(1)
        if s == 2 and k == 1 and not large:
            assert bool(dead.reshape(N, H, W)[:, 1::2].all()) and bool(dead.reshape(N, H, W)[:, :, 1::2].all())
        if bool(dead.any()):
            exact = torch.zeros_like(got) if add is None else D.rows(add, m)
            if mask is not None:
                exact = torch.where(D.rows(mask, m) > 0, exact, torch.zeros_like(exact))
            assert torch.equal(got[dead], exact[dead]), '%s: pixels the forward never read are not exactly the add / 0' % name
    if g['out16'] is not None:
        got16 = D.rows(g['out16'], m)
        worst16 = D.check(name + ' bf16 out', got16, r['ref'], r['bar32'] + D.bf16_half_ulp(r['ref']), m=m, OHW=(H, W))
        if g['out'] is not None:
            assert torch.equal(g['out16'], g['out'].bfloat16()), '%s: g16 is not the bf16 rounding of g32' % name
    if slot is not None:
        sref, sbar = D.slot_colsum_refs(r, m, slots, slot, M)
        got_s = g['part'].reshape(-1, Cin, 2)[torch.as_tensor(slots), :, 0].cpu().double()
        worst_s = D.check(name + ' slots', got_s, sref, sbar)
    if g['cs'] is not None:
        if large:
            # every pixel in fp64 on the device, pinned to the sampled CPU reference
            td, magd = D.tap_scatter(dy, ws.to(dy.device), s, p, (H, W))
            mi = torch.as_tensor(m, device=td.device)
            assert bool(((td[mi].cpu() - t).abs() <= 1e-12 * mag).all()) and bool(((magd[mi].cpu() - mag).abs() <= 1e-12 * mag).all())
            dev = (lambda v: None if v is None else v.reshape(M, Cin).cuda().double())
            rd = D.finish(td, magd, dev(add), dev(mask), **kw)
            cref, cbar = (v.cpu() for v in D.colsum_ref(rd))
            if slot is not None:     # ... and every slot, not the sampled ones alone: a slot dropped anywhere in the map
                aref, abar = (v.cpu() for v in D.all_slot_colsum_refs(rd, slot))
                got_a = g['part'].reshape(-1, Cin, 2)[:aref.shape[0], :, 0].cpu().double()
                worst_s = max(worst_s, D.check(name + ' all slots', got_a, aref, abar))
        else:
            cref, cbar = D.colsum_ref(r)
        worst_cs = D.check(name + ' column sums', g['cs'].cpu().double().view(1, -1), cref.view(1, -1), cbar.view(1, -1))
    print('\nDGRAD %-18s worst_out %.4f worst_out16 %.4f worst_slots %.3g worst_colsum %.3g  %s'
          % (want, worst, worst16, worst_s, worst_cs, name))
