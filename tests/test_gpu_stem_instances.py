"""-m gpu: the kernels in front of layer1 pinned per element, on whole maps, to the fp64 references and bars of tests/stem_fp64_ref.py --
the fused 7x7 / 2 conv + BN + ReLU + max-pool with its recording instance (csrc/stem_f32.hip), the bf16 conv, the fused bf16 pool and its
recording instance (csrc/stem_bf16.hip), the three launches of the deep stem one by one (csrc/stem_deep.hip) and stem_pool_bwd_kernel with
its column-sum slots (csrc/stem_bwd.hip) -- at their tile seams: three tiles on both axes (an interior tile with both halos real), one-row,
one-column and two-column last tiles, exactly full tiles, odd conv maps (an out-of-map row and column in the last windows), maps below
one tile, null scale / bias, whole channels clipped.

Protocol of every case: the C entry point writes into slices of larger buffers (floats NaN-filled, byte maps filled with 0xA5, a byte no map
can hold); the guards must stay bit for bit, every element must be written, a second run, the ops wrapper, the planar (N, 3, H, W) input, the
NHWC4 input with a NaN 4th channel and the single-image launches of images 0 and N - 1 must give the same bits.  ``coverage`` names the states
the tables must reach; tests/test_stem_instances_host.py asserts the admission rules of every case and that the bars refuse the faults they
exist for."""
import collections
import time

import pytest
import torch

from tests import stem_fp64_ref as SR

BYTE_FILL = 0xA5

Fused = collections.namedtuple('Fused', 'N H W combo why')          # combo: '', noscale, nobias, none, dead8
Conv16 = collections.namedtuple('Conv16', 'N H W relu combo why')
Deep = collections.namedtuple('Deep', 'N H W why')
Bwd = collections.namedtuple('Bwd', 'N OH OW why')

FUSED_CASES = [
    Fused(2, 67, 131, '', '3 x 3 tiles: an interior tile with both halos real, a one-row and one-column last tile'),
    Fused(1, 65, 129, '', 'OH, OW = 33, 65: the last windows hold an out-of-map row and column'),
    Fused(2, 64, 128, '', 'PH, PW = 16, 32: exactly full tiles'),
    Fused(1, 61, 69, '', 'OH 31, OW 35, PW 18: a two-column last tile, odd H and W'),
    Fused(1, 33, 257, '', 'PH 9, PW 65: five tile columns'),
    Fused(3, 5, 4, '', 'below one tile, three images'),
    Fused(2, 1, 1, '', 'one-pixel maps'),
    Fused(1, 2, 3, '', 'below one tile'),
    Fused(1, 3, 2, '', 'below one tile'),
    Fused(2, 67, 131, 'noscale', 'scale null'),
    Fused(2, 67, 131, 'nobias', 'bias null'),
    Fused(2, 67, 131, 'none', 'scale and bias null'),
    Fused(2, 67, 131, 'dead8', 'bias = -50 on eight channels: whole channels 0 / 255'),
]
CONV16_CASES = [
    Conv16(2, 67, 131, 1, '', 'conv tiles 16, 16, 2 by 32, 32, 2'),
    Conv16(1, 63, 127, 1, '', 'full tiles'),
    Conv16(3, 5, 4, 1, '', 'below one tile, three images'),
    Conv16(2, 1, 1, 1, '', 'one-pixel maps'),
    Conv16(2, 67, 131, 0, '', 'no ReLU'),
    Conv16(2, 67, 131, 1, 'none', 'scale and bias null'),
    Conv16(2, 67, 131, 0, 'none', 'no epilogue at all'),
]
DEEP_CASES = [
    Deep(2, 35, 131, 'A / B tiles 16, 2 by 32, 32, 2; C tiles 4, 4, 1 by 16, 16, 1'),
    Deep(1, 33, 129, 'OH, OW = 17, 65: odd'),
    Deep(2, 64, 128, 'full tiles everywhere'),
    Deep(1, 29, 61, 'one partial A / B tile, PH, PW = 8, 16'),
    Deep(3, 5, 3, 'below one tile, three images'),
    Deep(1, 1, 1, 'one-pixel map'),
    Deep(1, 2, 2, 'below one tile'),
]
BWD_CASES = [
    Bwd(2, 34, 66, '5 slots, the last of 392 pixels, slot 2 straddles the images'),
    Bwd(1, 33, 65, 'odd: vy / vx false in the last row and column'),
    Bwd(4, 3, 2, 'OW < 16: a 16-pixel step crosses rows and images'),
    Bwd(3, 1, 40, 'a single row: a 16-pixel step crosses images'),
    Bwd(1, 1, 1, 'one pixel'),
]
DEAD = list(range(0, 64, 8))
SEED_SHIFT = {(1, 2, 3): 1}      # a map of 128 conv values: the first seed that meets the admission rules (30-70 % clipped) from fp64 alone


def case_id(c):
    return '_'.join(str(v) for v in c[:-1] if v != '')


def seed(c):
    """By table and shape: the epilogue variants of a shape share its image and weights."""
    return (c[0] * 7 + c[1] * 131 + c[2] * 17 + 1000 * len(type(c).__name__) + SEED_SHIFT.get(tuple(c[:3]), 0)) % 100003


def fused_inputs(c):
    """The recipe of stem_fp64_ref.stem7_inputs with the case's epilogue variant (Fused and Conv16 cases)."""
    inp = SR.stem7_inputs(c.N, c.H, c.W, seed(c))
    if c.combo in ('noscale', 'none'):
        inp['scale'] = None
    if c.combo in ('nobias', 'none'):
        inp['bias'] = None
    if c.combo == 'dead8':
        inp['bias'][DEAD] = -50.0
    return inp


def bwd_image_hw(c):
    """An image whose 7x7 / 2 conv map is (OH, OW)."""
    return 2 * c.OH - 1, 2 * c.OW - 1


def coverage(fused=FUSED_CASES, conv16=CONV16_CASES, deep=DEEP_CASES, bwd=BWD_CASES):
    """{state: reached by some case} -- the tile-seam states the tables exist for, from the restated geometry of stem_fp64_ref."""
    out = {}
    fg = [(c, SR.fused_geom(c.H, c.W)) for c in fused]
    plain = [(c, g) for c, g in fg if c.combo == '']

    def put(name, ok):
        out[name] = bool(ok)
    put('fused: 3 x 3 tiles (an interior tile with both halos real), one-row and one-column last tile, two images',
        any(g['tilesY'] >= 3 and g['tilesX'] >= 3 and g['lastY'] == 1 and g['lastX'] == 1 and c.N >= 2 for c, g in plain))
    put('fused: OH and OW odd (an out-of-map row and column in the last windows)', any(g['OH'] % 2 and g['OW'] % 2 and g['OH'] > 16 for c, g in plain))
    put('fused: OH and OW even (the last windows end inside the map)', any(g['OH'] % 2 == 0 and g['OW'] % 2 == 0 and g['OH'] > 16 for c, g in plain))
    put('fused: exactly full tiles', any(g['lastY'] == SR.FUSED_TILE[0] and g['lastX'] == SR.FUSED_TILE[1] and g['tilesY'] > 1 and g['tilesX'] > 1 for c, g in plain))
    put('fused: a two-column last tile, odd H and W', any(g['lastX'] == 2 and c.H % 2 and c.W % 2 for c, g in plain))
    put('fused: five tile columns', any(g['tilesX'] >= 5 for c, g in plain))
    put('fused: a map below one tile with three images', any(g['tilesY'] == 1 and g['tilesX'] == 1 and g['PH'] < 8 and g['PW'] < 16 and c.N >= 3 for c, g in plain))
    put('fused: a one-pixel map', any(c.H == 1 and c.W == 1 for c, g in plain))
    put('fused: a one-row conv map and a one-column conv map', any(g['OH'] == 1 and g['OW'] > 1 for c, g in plain) and any(g['OW'] == 1 and g['OH'] > 1 for c, g in plain))
    for combo in ('noscale', 'nobias', 'none', 'dead8'):
        put('fused: %s on 3 x 3 tiles' % combo, any(c.combo == combo and g['tilesY'] >= 3 and g['tilesX'] >= 3 for c, g in fg))
    cg = [(c, SR.conv_tiles(SR.half(c.H), SR.half(c.W))) for c in conv16]
    put('bf16 conv: tiles 16, 16, 2 by 32, 32, 2', any(g['tilesY'] == 3 and g['tilesX'] == 3 and g['lastY'] == 2 and g['lastX'] == 2 and c.relu and not c.combo for c, g in cg))
    put('bf16 conv: full tiles', any(g['lastY'] == 16 and g['lastX'] == 32 and g['tilesY'] > 1 and g['tilesX'] > 1 for c, g in cg))
    put('bf16 conv: below one tile with three images', any(g['tilesY'] == 1 and g['tilesX'] == 1 and c.N >= 3 for c, g in cg))
    put('bf16 conv: a one-pixel map', any(c.H == 1 and c.W == 1 for c, g in cg))
    put('bf16 conv: relu = 0 on three tiles', any(not c.relu and g['tilesY'] == 3 for c, g in cg))
    put('bf16 conv: scale and bias null', any(c.combo == 'none' for c, g in cg))
    dg = [(c, SR.deep_geom(c.H, c.W)) for c in deep]
    put('deep: A / B tiles 16, 2 by 32, 32, 2 and C tiles 4, 4, 1 by 16, 16, 1, two images',
        any(g['ab']['tilesY'] == 2 and g['ab']['lastY'] == 2 and g['ab']['tilesX'] == 3 and g['ab']['lastX'] == 2 and g['c']['tilesY'] == 3 and
            g['c']['lastY'] == 1 and g['c']['tilesX'] == 3 and g['c']['lastX'] == 1 and c.N >= 2 for c, g in dg))
    put('deep: OH and OW odd', any(g['OH'] % 2 and g['OW'] % 2 and g['OH'] > 8 for c, g in dg))
    put('deep: full tiles everywhere', any(g['ab']['lastY'] == 16 and g['ab']['lastX'] == 32 and g['c']['lastY'] == 4 and g['c']['lastX'] == 16 and
                                          g['ab']['tilesY'] > 1 and g['ab']['tilesX'] > 1 for c, g in dg))
    put('deep: one partial A / B tile, PH, PW = 8, 16', any(g['ab']['tilesY'] == 1 and g['ab']['tilesX'] == 1 and g['ab']['lastY'] < 16 and g['ab']['lastX'] < 32 and
                                                           (g['PH'], g['PW']) == (8, 16) for c, g in dg))
    put('deep: below one tile with three images', any(g['PH'] < 4 and g['PW'] < 16 and c.N >= 3 for c, g in dg))
    put('deep: a one-pixel map', any(c.H == 1 and c.W == 1 for c, g in dg))
    sl = [(c, SR.slots(c.N, c.OH, c.OW)) for c in bwd]
    put('bwd: 5 slots, a partial last one, a slot that straddles two images',
        any(len(s) == 5 and s[-1][1] < SR.SLOT and any(a < c.OH * c.OW < a + n for a, n in s) and c.N == 2 for c, s in sl))
    put('bwd: OH and OW odd', any(c.OH % 2 and c.OW % 2 and c.OH > 1 for c, s in sl))
    put('bwd: OW < 16, several rows and images in one slot', any(c.OW < 16 and c.OH > 1 and c.N > 1 and len(s) == 1 for c, s in sl))
    put('bwd: a single row, several images in one slot', any(c.OH == 1 and c.OW > 16 and c.N > 1 and len(s) == 1 for c, s in sl))
    put('bwd: one pixel', any((c.N, c.OH, c.OW) == (1, 1, 1) for c, s in sl))
    return out


# ---- buffers ----------------------------------------------------------------------------------------------------------------------
def _fill(dtype):
    return BYTE_FILL if dtype == torch.uint8 else float('nan')


def bits(t):
    return t if t.dtype == torch.uint8 else t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def guarded(shape, dtype=torch.float32):
    """A filled buffer with one guard block (the size of shape[1:]) before and after, and the slice between them."""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), _fill(dtype), device='cuda', dtype=dtype)
    return buf, buf[1:1 + shape[0]]


def guards_intact(buf):
    fill = torch.full_like(buf[:1], _fill(buf.dtype))
    return torch.equal(bits(buf[:1]), bits(fill)) and torch.equal(bits(buf[-1:]), bits(fill))


def written(t):
    return not bool((t == BYTE_FILL).any()) if t.dtype == torch.uint8 else not bool(torch.isnan(t).any())


def cu(t):
    return None if t is None else t.cuda().contiguous()


def protocol(name, run, img, ops_run=None, nan4=True):
    """run(x on the device, layout) -> tuple of outputs (slices of guarded buffers; run asserts the guards).  The bit-equality part of the
    module docstring; returns the outputs of the NHWC4 run.  ops_run(x NHWC4) -> a tuple aligned with run's (None: not produced)."""
    x4, xp = SR.nhwc4(img).cuda(), img.cuda().contiguous()
    base = run(x4, 0)
    for i, o in enumerate(base):
        assert written(o), '%s: output %d has elements that were not written' % (name, i)

    def same(what, got, ref=None):
        for i, (g, r) in enumerate(zip(got, ref or base)):
            if g is not None:
                assert same_bits(g, r), '%s: %s differs from the NHWC4 run in output %d (%d elements)' % (name, what, i, int((bits(g) != bits(r)).sum()))
    same('a second run', run(x4, 0))
    same('the planar input', run(xp, 1))
    if nan4:
        same('a NaN 4th channel', run(SR.nhwc4(img, float('nan')).cuda(), 0))
    N = img.shape[0]
    if N > 1:
        for n in (0, N - 1):
            same('the single-image launch of image %d' % n, run(x4[n:n + 1].contiguous(), 0), [o[n:n + 1] for o in base])
    if ops_run is not None:
        same('the ops wrapper', ops_run(x4))
    return base


# ---- launches through the C entry points ------------------------------------------------------------------------------------------
def launch_pool7(kind, x, layout, wp, scale, bias, H, W, rec):
    """cpr_stem7x7s2_pool_{f32, bf16}[_rec] -> (out,) or (out, arg)."""
    from pointtinybenchmark_amd import _lib, ops
    N, g = x.shape[0], SR.fused_geom(H, W)
    shape = (N, g['PH'], g['PW'], 64)
    obuf, out = guarded(shape, torch.float32 if kind == 'f32' else torch.bfloat16)
    abuf, arg = guarded(shape, torch.uint8) if rec else (None, None)
    args = [ops._ptr(x), ops._ptr(wp), ops._ptr(scale), ops._ptr(bias), ops._ptr(out)] + ([ops._ptr(arg)] if rec else []) + [N, H, W, layout, ops._stream()]
    _lib.call('cpr_stem7x7s2_pool_%s%s' % (kind, '_rec' if rec else ''), *args)
    torch.cuda.synchronize()
    assert guards_intact(obuf) and (abuf is None or guards_intact(abuf)), 'the guards around the outputs were written'
    return (out, arg) if rec else (out,)


def launch_conv16(x, layout, wp, scale, bias, H, W, relu):
    from pointtinybenchmark_amd import _lib, ops
    N = x.shape[0]
    buf, out = guarded((N, SR.half(H), SR.half(W), 64), torch.bfloat16)
    _lib.call('cpr_stem7x7s2_bf16', ops._ptr(x), ops._ptr(wp), ops._ptr(scale), ops._ptr(bias), ops._ptr(out), N, H, W, relu, layout, ops._stream())
    torch.cuda.synchronize()
    assert guards_intact(buf), 'the guards around the output were written'
    return (out,)


def launch_deep(x, layout, packs, folds, H, W, out_bf16):
    """cpr_stem_deep_fwd -> (mid1, mid2, out)."""
    from pointtinybenchmark_amd import _lib, ops
    N, g = x.shape[0], SR.deep_geom(H, W)
    b1, mid1 = guarded((N, g['OH'], g['OW'], 32))
    b2, mid2 = guarded((N, g['OH'], g['OW'], 32))
    bo, out = guarded((N, g['PH'], g['PW'], 64), torch.bfloat16 if out_bf16 else torch.float32)
    (s1, c1), (s2, c2), (s3, c3) = folds
    _lib.call('cpr_stem_deep_fwd', ops._ptr(x), ops._ptr(packs[0].w), ops._ptr(s1), ops._ptr(c1), ops._ptr(packs[1].w), ops._ptr(s2), ops._ptr(c2),
              ops._ptr(packs[2].w), ops._ptr(s3), ops._ptr(c3), ops._ptr(mid1), ops._ptr(mid2), ops._ptr(out), N, H, W, layout, int(out_bf16),
              ops._stream())
    torch.cuda.synchronize()
    assert guards_intact(b1) and guards_intact(b2) and guards_intact(bo), 'the guards around the outputs were written'
    return mid1, mid2, out


def launch_bwd(dp, arg, OH, OW):
    """cpr_stem_pool_bwd -> (dy, part)."""
    from pointtinybenchmark_amd import _lib, ops
    N = dp.shape[0]
    nslots = len(SR.slots(N, OH, OW))
    assert _lib.call('cpr_stem_pool_bwd_blocks', N * OH * OW, positive=True) == nslots
    bd, dy = guarded((N, OH, OW, 64))
    bp, part = guarded((nslots, 64, 2))
    _lib.call('cpr_stem_pool_bwd', ops._ptr(dp), ops._ptr(arg), ops._ptr(dy), ops._ptr(part), N, OH, OW, ops._stream())
    torch.cuda.synchronize()
    assert guards_intact(bd) and guards_intact(bp), 'the guards around the outputs were written'
    return dy, part


# ---- the tests --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tables_reach_every_state():
    missing = [n for n, ok in coverage().items() if not ok]
    assert not missing, 'the tables no longer reach: %s' % '; '.join(missing)


@pytest.mark.gpu
@pytest.mark.parametrize('c', FUSED_CASES, ids=case_id)
def test_fused_f32_instances_vs_fp64(c):
    from pointtinybenchmark_amd import ops
    t0, name = time.time(), 'fused f32 ' + case_id(c)
    inp = fused_inputs(c)
    wp, sc, bi = ops.stem_weight_f32(inp['w'].cuda()), cu(inp['scale']), cu(inp['bias'])
    out, arg = protocol(name + ' rec', lambda x, lay: launch_pool7('f32', x, lay, wp, sc, bi, c.H, c.W, True), inp['img'],
                        lambda x4: ops.stem7x7s2_pool_f32(x4, wp, sc, bi, planar=False, record=True))
    (plain,) = protocol(name, lambda x, lay: launch_pool7('f32', x, lay, wp, sc, bi, c.H, c.W, False), inp['img'],
                        lambda x4: (ops.stem7x7s2_pool_f32(x4, wp, sc, bi, planar=False),))
    assert same_bits(plain, out), '%s: the recording instance differs from the plain one' % name
    t, e = SR.conv_ref(inp['img'], inp['w'], 2, 3, inp['scale'], inp['bias'])
    ref, bar = SR.pool_ref(t, e)
    got, amap = SR.nchw(out), SR.nchw(arg)
    q = float(SR.ratio(got, ref, bar).max())
    print('\nSTEM %s worst |err| / bar %.4f' % (name, q))
    SR.check_map(name, got, ref, bar)
    und = SR.check_argmap(name, got, amap, t, e)
    print('STEM %s undecided byte-map share %.2e, zeros %.4f  %.2f s' % (name, und, float((got == 0).double().mean()), time.time() - t0))
    assert und <= SR.UNDECIDED_MAX
    if c.combo == 'dead8':
        assert not bool(got[:, DEAD].any()) and bool((amap[:, DEAD] == 255).all()), '%s: a clipped channel is not 0 / 255 everywhere' % name


@pytest.mark.gpu
@pytest.mark.parametrize('c', FUSED_CASES, ids=case_id)
def test_fused_bf16_instances_equal_the_pooled_bf16_conv(c):
    """The fused bf16 pool and its recording instance: the bits of maxpool3x3s2 of the bf16 conv kernel's own output, outputs and byte maps,
    and exactly the first-of-ties maximum of that map (pool_exact); the conv map itself is held to the bf16 bar."""
    from pointtinybenchmark_amd import ops
    t0, name = time.time(), 'fused bf16 ' + case_id(c)
    inp = fused_inputs(c)
    wp, sc, bi = ops.stem_weight_bf16(inp['w'].cuda()), cu(inp['scale']), cu(inp['bias'])
    (conv,) = launch_conv16(SR.nhwc4(inp['img']).cuda(), 0, wp, sc, bi, c.H, c.W, 1)
    p_out, p_arg = ops.maxpool3x3s2(conv, record=True)
    out, arg = protocol(name + ' rec', lambda x, lay: launch_pool7('bf16', x, lay, wp, sc, bi, c.H, c.W, True), inp['img'],
                        lambda x4: ops.stem7x7s2_pool_bf16(x4, wp, sc, bi, planar=False, record=True))
    (plain,) = protocol(name, lambda x, lay: launch_pool7('bf16', x, lay, wp, sc, bi, c.H, c.W, False), inp['img'],
                        lambda x4: (ops.stem7x7s2_pool_bf16(x4, wp, sc, bi, planar=False),))
    assert same_bits(plain, out), '%s: the recording instance differs from the plain one' % name
    assert same_bits(out, p_out), '%s: differs from maxpool3x3s2 of the bf16 conv in %d elements' % (name, int((bits(out) != bits(p_out)).sum()))
    assert same_bits(arg, p_arg), '%s: byte map differs from maxpool3x3s2 of the bf16 conv in %d elements' % (name, int((arg != p_arg).sum()))
    z = SR.nchw(conv)
    mx, am = SR.pool_exact(z)
    assert torch.equal(SR.nchw(out), mx), '%s: not the maximum of the kernel\'s own conv map' % name
    assert torch.equal(SR.nchw(arg).long(), am), '%s: byte map is not the first maximum of the kernel\'s own conv map' % name
    x16, w16 = SR.bf16_operands(inp['img'], wp)
    t, e = SR.conv_ref(x16, w16, 2, 3, inp['scale'], inp['bias'])
    ref = t.clamp_min(0)
    q = SR.check_map(name + ' conv', z, ref, e + SR.bf16_half_ulp(ref))
    print('\nSTEM %s conv worst |err| / bar %.4f, tied windows %.4f  %.2f s' % (
        name, q, float((SR.pool_exact_last_of_ties(z)[1] != am).double().mean()), time.time() - t0))
    if c.combo == 'dead8':
        assert not bool(mx[:, DEAD].any()) and bool((am[:, DEAD] == 255).all())


@pytest.mark.gpu
@pytest.mark.parametrize('c', CONV16_CASES, ids=case_id)
def test_bf16_conv_instances_vs_fp64(c):
    from pointtinybenchmark_amd import ops
    t0, name = time.time(), 'bf16 conv ' + case_id(c)
    inp = fused_inputs(c)
    wp, sc, bi = ops.stem_weight_bf16(inp['w'].cuda()), cu(inp['scale']), cu(inp['bias'])
    (out,) = protocol(name, lambda x, lay: launch_conv16(x, lay, wp, sc, bi, c.H, c.W, c.relu), inp['img'],
                      lambda x4: (ops.stem7x7s2_bf16(x4, wp, sc, bi, relu=bool(c.relu), planar=False),))
    x16, w16 = SR.bf16_operands(inp['img'], wp)
    t, e = SR.conv_ref(x16, w16, 2, 3, inp['scale'], inp['bias'])
    ref = t.clamp_min(0) if c.relu else t
    got = SR.nchw(out)
    q = SR.check_map(name, got, ref, e + SR.bf16_half_ulp(ref))
    if not c.relu:
        assert bool((got < 0).any())
    print('\nSTEM %s worst |err| / bar %.4f  %.2f s' % (name, q, time.time() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize('c', DEEP_CASES, ids=case_id)
def test_deep_stem_launches_vs_fp64(c):
    """Each launch on the exact operands it read: mid1 against the image, mid2 against the kernel's own mid1, the pooled map against the
    kernel's own mid2; the bf16 mode = the fp32 mode's mid maps and the rounding of its output, bit for bit."""
    from pointtinybenchmark_amd import ops
    t0, name = time.time(), 'deep ' + case_id(c)
    inp = SR.deep_inputs(c.N, c.H, c.W, seed(c))
    packs = [ops.PackedConv(w.cuda(), s, 1) for w, s in zip(inp['w'], (2, 1, 1))]
    for pc in packs:
        ops.pack_ready(pc)
    folds = [(cu(s), cu(b)) for s, b in inp['folds']]
    torch.cuda.synchronize()

    def wrapper(dtype):
        return lambda x4: (ops.stem3x3s2(x4, packs[0], *folds[0], planar=False), None, ops.stem_deep(x4, packs, folds, planar=False, out_dtype=dtype))
    mid1, mid2, out = protocol(name, lambda x, lay: launch_deep(x, lay, packs, folds, c.H, c.W, 0), inp['img'], wrapper(torch.float32))
    m1b, m2b, out16 = protocol(name + ' bf16', lambda x, lay: launch_deep(x, lay, packs, folds, c.H, c.W, 1), inp['img'], wrapper(torch.bfloat16))
    assert same_bits(mid1, m1b) and same_bits(mid2, m2b), '%s: the mid maps of the two modes differ' % name
    assert same_bits(out16, out.to(torch.bfloat16)), '%s: the bf16 output is not the rounding of the fp32 output in %d elements' % (
        name, int((bits(out16) != bits(out.to(torch.bfloat16))).sum()))
    (s1, c1), (s2, c2), (s3, c3) = inp['folds']
    t, e = SR.conv_ref(inp['img'], inp['w'][0], 2, 1, s1, c1)
    qa = SR.check_map(name + ' launch A', SR.nchw(mid1), t.clamp_min(0), e)
    t, e = SR.conv_ref(SR.nchw(mid1), inp['w'][1], 1, 1, s2, c2)
    qb = SR.check_map(name + ' launch B', SR.nchw(mid2), t.clamp_min(0), e)
    t, e = SR.conv_ref(SR.nchw(mid2), inp['w'][2], 1, 1, s3, c3)
    ref, bar = SR.pool_ref(t, e)
    qc = SR.check_map(name + ' launch C', SR.nchw(out), ref, bar)
    print('\nSTEM %s worst |err| / bar A %.4f B %.4f C %.4f, zeros %.4f  %.2f s' % (name, qa, qb, qc, float((out == 0).float().mean()), time.time() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize('c', BWD_CASES, ids=case_id)
def test_stem_pool_bwd_vs_the_gather_and_fp64_slots(c):
    from pointtinybenchmark_amd import ops
    from tests.test_gpu_stem_train import _gather_torch
    t0, name = time.time(), 'pool bwd ' + case_id(c)
    H, W = bwd_image_hw(c)
    inp = SR.stem7_inputs(c.N, H, W, seed(c))
    _, arg = ops.stem7x7s2_pool_f32(SR.nhwc4(inp['img']).cuda(), ops.stem_weight_f32(inp['w'].cuda()), cu(inp['scale']), cu(inp['bias']), planar=False,
                                    record=True)
    g = torch.Generator().manual_seed(seed(c) + 1)
    dp = torch.randn(tuple(arg.shape), generator=g)
    dp[..., ::5] = 0.0
    dp = dp.cuda()
    dy, part = launch_bwd(dp, arg, c.OH, c.OW)
    assert written(dy) and written(part), '%s: elements were not written' % name
    dy2, part2 = launch_bwd(dp, arg, c.OH, c.OW)
    assert same_bits(dy, dy2) and same_bits(part, part2), '%s: the second run differs' % name
    dyo, tp = ops.stem_pool_bwd(dp, arg, (c.OH, c.OW))
    assert same_bits(dy, dyo) and same_bits(part, tp.part), '%s: the ops wrapper differs' % name
    if c.N > 1:
        for n in (0, c.N - 1):
            d1, _ = launch_bwd(dp[n:n + 1].contiguous(), arg[n:n + 1].contiguous(), c.OH, c.OW)
            assert same_bits(d1, dy[n:n + 1]), '%s: image %d differs from its single-image launch' % (name, n)
    want = _gather_torch(dp, arg, c.OH, c.OW)
    assert same_bits(dy, want), '%s: dy differs from the torch gather in %d elements' % (name, int((bits(dy) != bits(want)).sum()))
    chosen = _gather_torch(torch.ones_like(dp), arg, c.OH, c.OW) > 0
    assert bool((bits(dy)[~chosen] == 0).all()), '%s: a pixel no window chose is not +0.0' % name
    assert bool(chosen.any()) and bool((~chosen).any())          # (a one-pixel map: the channels the ReLU clipped are the unchosen ones)
    ref, bar = SR.slot_refs(dy)
    got = part.cpu().double()
    assert bool((bits(part)[..., 1] == 0).all()), '%s: element 1 of a slot is not +0.0' % name
    q = SR.check(name + ' slots', got[..., 0], ref, bar)
    print('\nSTEM %s slots worst |err| / bar %.4f (%d slots)  %.2f s' % (name, q, ref.shape[0], time.time() - t0))


# ---- argument refusals (no launch, so no GPU needed) ------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_any_launch():
    from pointtinybenchmark_amd import _lib
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    buf = torch.zeros(1 << 16, device=dev)
    p = buf.data_ptr()

    def refused(name, args, **bad):
        """args: ordered {parameter: value}; every value of ``bad`` replaces one."""
        a = collections.OrderedDict(args)
        a.update(bad)
        with pytest.raises(_lib.CprHipError, match='invalid argument'):
            _lib.call(name, *a.values())

    def sweep(name, args, ptrs, dims, layout=True):
        for k in ptrs:
            refused(name, args, **{k: None})
        for k in dims:
            refused(name, args, **{k: 0})
            refused(name, args, **{k: -1})
        if layout:
            refused(name, args, layout=2)
            refused(name, args, layout=-1)

    for kind in ('f32', 'bf16'):
        plain = [('x', p), ('w', p), ('scale', p), ('bias', p), ('out', p), ('N', 1), ('H', 8), ('W', 8), ('layout', 0), ('stream', None)]
        sweep('cpr_stem7x7s2_pool_' + kind, plain, ('x', 'w', 'out'), ('N', 'H', 'W'))
        rec = plain[:5] + [('arg', p)] + plain[5:]
        sweep('cpr_stem7x7s2_pool_%s_rec' % kind, rec, ('x', 'w', 'out', 'arg'), ('N', 'H', 'W'))
    conv = [('x', p), ('w', p), ('scale', p), ('bias', p), ('out', p), ('N', 1), ('H', 8), ('W', 8), ('relu', 1), ('layout', 0), ('stream', None)]
    sweep('cpr_stem7x7s2_bf16', conv, ('x', 'w', 'out'), ('N', 'H', 'W'))
    names = ('x', 'w1', 's1', 'b1', 'w2', 's2', 'b2', 'w3', 's3', 'b3', 'mid1', 'mid2', 'out')
    deep = [(n, p) for n in names] + [('N', 1), ('H', 8), ('W', 8), ('layout', 0), ('out_bf16', 0), ('stream', None)]
    sweep('cpr_stem_deep_fwd', deep, names, ('N', 'H', 'W'))
    refused('cpr_stem_deep_fwd', deep, out_bf16=2)
    a = [('x', p), ('w', p), ('scale', p), ('bias', p), ('out', p), ('N', 1), ('H', 8), ('W', 8), ('layout', 0), ('stream', None)]
    sweep('cpr_stem3x3s2_fwd', a, ('x', 'w', 'scale', 'bias', 'out'), ('N', 'H', 'W'))
    bwd = [('dp', p), ('arg', p), ('dy', p), ('part', p), ('N', 1), ('OH', 4), ('OW', 4), ('stream', None)]
    sweep('cpr_stem_pool_bwd', bwd, ('dp', 'arg', 'dy', 'part'), ('N', 'OH', 'OW'), layout=False)
    with pytest.raises(_lib.CprHipError, match='invalid argument'):
        _lib.call('cpr_stem_pool_bwd_blocks', 0, positive=True)
