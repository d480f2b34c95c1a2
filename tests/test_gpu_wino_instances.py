"""-m gpu: the two fused Winograd forward kernels (csrc/conv_wino.hip = kernel '64', csrc/conv_wino32.hip = kernel '32') pinned per
element to the fp64 direct convolution of tests/wino_fp64_ref.py on every state of their persistent tile loops: runs of 1, 2 and 3
tiles, the fused affine table swapped across images and kept within one, idle workgroups, maps below one region, one-row and one-column
regions, the shortest K loops, the whole affine table, every layout and epilogue, the statistics slots region by region.

A case is (kernel, N, H, W, Cin, Cout, flags, why).  flags: scale, bias, relu (epilogue), gn (statistics slots), inab / inrelu (fused
input affine, with ReLU), inb8 / outb8 (channel-blocked input / output), offset (inputs with per-channel |mean| / std = 4), entry (the
C entry point only: ops.wino_eligible / PackedConv decline the shape), auto (through ops.conv2d with ops.WINO_TILE = 'auto').  Every
other case goes through ops.conv3x3_wino with ops.WINO_TILE forced; the route word of ops.TRACE_CONV_VARIANT is asserted either way.

Every case runs twice -- the second time through the C entry point into a NaN-filled output that is a slice of a larger NaN-filled
buffer and a NaN-filled gn_part of exactly the queried size -- and must give the same bits, leave the guards NaN bit for bit, write
every output element and slot, and meet bar 1 (the Winograd bound), bar 2 (the direct bar, on the zero-mean cases without a fused
affine) and the slot bars of wino_fp64_ref.  ``coverage`` names the states the table must reach; tests/test_wino_instances_host.py
asserts them at 256 CUs, this file again at the device's own CU count."""
import collections
import time

import numpy as np
import pytest
import torch

from tests import conv_fp64_ref as R
from tests import wino_fp64_ref as WR
from tests.test_gpu_wino import _from_b8 as from_b8, _to_b8 as to_b8

Case = collections.namedtuple('Case', 'kernel N H W Cin Cout flags why')


def _table(k):
    """The cases of one kernel ('64' / '32'): the same states on both, at shapes that fit the kernel's regions and grid cap."""
    big = k == '64'
    small = (2, 19, 21, 32, 64)          # 2 x 2 / 3 x 2 regions: one spare row of pixels short of whole tiles, odd sizes
    lay = (2, 19, 37, 64, 128)
    cs = [
        # ---- idle workgroups, maps below one region, the shortest K loops (entry point only)
        Case(k, 1, 13, 13, 32, 64, 'entry', 'T = 1: seven idle workgroups, 4 chunks') if big else
        Case(k, 1, 5, 9, 16, 64, 'entry', 'T = 1: seven idle workgroups, 4 chunks'),
        Case(k, 1, 1, 1, 32 if big else 16, 64, 'entry bias', 'one-pixel map'),
        Case(k, 3, 17, 33, 48, 192, 'entry scale bias relu gn', 'T = 54: T % 8 = 6, one-row and one-column regions, 6 chunks') if big else
        Case(k, 3, 9, 17, 24, 192, 'entry scale bias relu gn', 'T = 36: T % 8 = 4, one-row and one-column regions, 6 chunks'),
        # ---- persistent loop: runs of 1 and 2, runs of 2 and 3
        Case(k, 3, 80, 80, 32, 256, '', 'T = 300: runs of 1 and 2 tiles') if big else
        Case(k, 9, 40, 40, 64, 256, '', 'T = 540: runs of 1 and 2 tiles, the stagger is on'),
        Case(k, 6, 80, 80, 32, 256, 'relu', 'T = 600: runs of 2 and 3 tiles') if big else
        Case(k, 18, 40, 40, 32, 256, 'relu', 'T = 1080: runs of 2 and 3 tiles'),
        # ---- the affine table across images and within one, partial right and bottom regions, >= 3 x 3 regions
        Case(k, 7, 44, 40, 64, 384, 'inab inrelu bias', 'table swap, NHWC, ReLU') if big else
        Case(k, 11, 36, 44, 64, 320, 'inab inrelu bias', 'table reload, NHWC, ReLU'),
        Case(k, 7, 44, 40, 64, 384, 'inab inb8 bias gn', 'table swap, blocked') if big else
        Case(k, 11, 36, 44, 64, 320, 'inab inb8 bias gn', 'table reload, blocked'),
        Case(k, 5, 70, 90, 64, 192, 'inab inrelu inb8 outb8 gn', 'table swap, blocked in and out, ReLU') if big else
        Case(k, 5, 36, 40, 256, 512, 'inab inrelu inb8 outb8 gn', 'table reload, the whole 256-entry table, blocked, ReLU'),
        Case(k, 5, 70, 90, 64, 192, 'inab', 'table swap, NHWC') if big else
        Case(k, 5, 36, 40, 256, 512, 'inab', 'table reload, the whole 256-entry table, NHWC'),
        # ---- cout tiles, layouts, offset inputs
        Case(k, 1, 24, 40, 64, 512, 'scale bias', 'Cout 512: eight cout tiles'),
        Case(k, *lay, 'inb8 bias relu', 'blocked in, NHWC out'),
        Case(k, *lay, 'outb8 bias', 'NHWC in, blocked out'),
        Case(k, *lay, 'inb8 outb8 scale bias', 'blocked in and out'),
        Case(k, 2, 35, 40, 64, 64, 'offset bias', 'inputs with |mean| / std = 4'),
        # ---- every epilogue alone, with statistics, statistics with a blocked output
        Case(k, *small, '', 'no epilogue'),
        Case(k, *small, 'bias', ''),
        Case(k, *small, 'scale bias', ''),
        Case(k, *small, 'relu', ''),
        Case(k, *small, 'gn', ''),
        Case(k, *small, 'bias gn', ''),
        Case(k, *small, 'scale bias gn', ''),
        Case(k, *small, 'relu gn', ''),
        Case(k, *small, 'gn outb8', ''),
    ]
    if big:
        cs += [
            Case(k, 2, 20, 24, 512, 64, 'inab inrelu', 'the whole 512-entry table'),
            Case(k, 1, 19, 21, 528, 64, 'entry bias', 'Cin 528 > 512 without an affine: 66 chunks'),
            Case(k, 1, 48, 40, 64, 128, 'auto scale bias relu', 'the dispatcher: 1920 pixels'),
            Case(k, 2, 44, 60, 32, 64, 'auto bias gn', 'the dispatcher: 2640 pixels'),
        ]
    else:
        cs += [
            Case(k, 2, 19, 21, 40, 64, 'entry bias relu', 'Cin 40: 10 chunks'),
            Case(k, 2, 40, 40, 64, 128, 'auto bias relu', 'the dispatcher: 1600 pixels'),
            Case(k, 1, 30, 29, 32, 64, 'auto gn', 'the dispatcher: 870 pixels'),
        ]
    return cs


CASES = _table('64') + _table('32')


def flags(c):
    return set(c.flags.split())


def case_id(c):
    return 'w%s_n%d_%dx%d_c%d_o%d_%s' % (c.kernel, c.N, c.H, c.W, c.Cin, c.Cout, c.flags.replace(' ', '-') or 'plain')


def takes_bar2(c):
    """Bar 2 (the direct bar) is asserted on the zero-mean cases without a fused affine."""
    return not ({'inab', 'offset'} & flags(c))


def auto_instance(c):
    """ops.wino_eligible and ops.WINO_AUTO restated: the kernel the dispatcher gives the shape ('64' / '32'), None if it declines."""
    fill = c.H * c.W / float(-(-c.H // 16) * 16 * (-(-c.W // 16) * 16))
    if not (c.Cin % 32 == 0 and c.Cout % 64 == 0 and fill >= 0.6):
        return None
    can32 = 'inab' not in flags(c) or c.Cin <= 256
    return '32' if can32 and c.H * c.W <= 40 * 40 else '64'


def coverage(cases, ncu):
    """{condition: holds} over the table at ``ncu`` CUs -- the states the issue lists, per kernel."""
    out = {}
    for k in ('64', '32'):
        rh, rw = WR.REGION[k]
        cs = [c for c in cases if c.kernel == k]
        T = {c: WR.tiles(c.N, c.H, c.W, c.Cout, k) for c in cs}
        kinds = {c: WR.run_kinds(WR.walk(c.N, c.H, c.W, c.Cout, k, ncu)) for c in cs}
        reg = {c: WR.regions(c.H, c.W, k) for c in cs}

        def put(name, ok):
            out['%s: %s' % (k, name)] = bool(ok)
        put('T = 1 on a map below one region', any(T[c] == 1 and 1 < c.H < rh and 1 < c.W < rw for c in cs))
        put('one-pixel map', any(c.H == 1 and c.W == 1 for c in cs))
        put('T % 8 != 0 with one spare row and column', any(T[c] % 8 and c.H % rh == 1 and c.W % rw == 1 and c.H > rh and c.W > rw for c in cs))
        put('runs of 1 and 2 tiles in one launch', any(kinds[c]['lens'] == {1, 2} for c in cs))
        put('runs of 2 and 3 tiles in one launch', any(kinds[c]['lens'] == {2, 3} for c in cs))
        for inrelu in (False, True):
            for inb8 in (False, True):
                put('affine table changed and kept within runs, partial right and bottom regions, inrelu=%d inb8=%d' % (inrelu, inb8),
                    any('inab' in flags(c) and ('inrelu' in flags(c)) == inrelu and ('inb8' in flags(c)) == inb8 and kinds[c]['change']
                        and kinds[c]['stay'] and c.H % rh and c.W % rw for c in cs))
        put('the whole affine table', any('inab' in flags(c) and c.Cin == WR.XFMAX[k] for c in cs))
        if k == '64':
            put('Cin > 512 without an affine', any('inab' not in flags(c) and c.Cin > 512 for c in cs))
        for co in (64, 192, 512):
            put('Cout %d' % co, any(c.Cout == co for c in cs))
        for ci in ((32, 48) if k == '64' else (16, 24, 40)):
            put('Cin %d' % ci, any(c.Cin == ci for c in cs))
        put('3 x 3 regions under a fused affine', any('inab' in flags(c) and reg[c][0] >= 3 and reg[c][1] >= 3 for c in cs))
        for inb8 in (False, True):
            for outb8 in (False, True):
                put('layout inb8=%d outb8=%d' % (inb8, outb8), any(('inb8' in flags(c)) == inb8 and ('outb8' in flags(c)) == outb8 for c in cs))
        for epi in ((), ('bias',), ('scale', 'bias'), ('relu',)):
            put('epilogue %s alone' % (' + '.join(epi) or 'none'), any(flags(c) - {'entry', 'auto'} == set(epi) for c in cs))
            put('epilogue %s with statistics' % (' + '.join(epi) or 'none'), any(flags(c) - {'entry', 'auto'} == set(epi) | {'gn'} for c in cs))
        put('statistics with a blocked output', any({'gn', 'outb8'} <= flags(c) for c in cs))
        put('offset inputs', any('offset' in flags(c) for c in cs))
        put('two cases through the dispatcher', sum('auto' in flags(c) for c in cs) >= 2)
    return out


# ---- inputs: seeded CPU generators (the CPU test emulates the kernels on the same operands) ---------------------------------------
def seed(c):
    return (sum(v * w for v, w in zip(c[1:6], (7, 131, 17, 3, 5))) + sum(map(ord, c.flags)) + int(c.kernel)) % 100003


def make_inputs(c):
    f = flags(c)
    g = torch.Generator().manual_seed(seed(c))
    x = torch.randn((c.N, c.H, c.W, c.Cin), generator=g)
    if 'offset' in f:
        x = x + torch.where(torch.rand(c.Cin, generator=g) < 0.5, -4.0, 4.0)
    w = torch.randn((c.Cout, c.Cin, 3, 3), generator=g) / (9 * c.Cin) ** 0.5
    scale = (torch.rand(c.Cout, generator=g) + 0.5) if 'scale' in f else None
    bias = torch.randn(c.Cout, generator=g) if 'bias' in f else None
    in_ab = None
    if 'inab' in f:      # a row per image, b of both signs
        in_ab = (torch.rand((c.N, c.Cin), generator=g) + 0.5, torch.randn((c.N, c.Cin), generator=g) * 0.5)
    return dict(x=x, w=w, scale=scale, bias=bias, in_ab=in_ab)


# ---- the GPU run ------------------------------------------------------------------------------------------------------------
PACK = {'64': 'cpr_wino_pack_weights', '32': 'cpr_wino32_pack_weights'}
FWD = {'64': 'cpr_conv3x3_wino_fwd', '32': 'cpr_conv3x3_wino32_fwd'}
WORD = {'64': 'wino', '32': 'wino32'}
NAN_BITS = 0x7fc00000


def rows_at_kpad(w):
    """w (Cout, Cin, 3, 3) as the direct kernel's pack [Cout][3][3][Cin] at row stride Kpad -- what the pack kernels read -- for the
    widths ops.PackedConv declines.  Returns (device rows, Kpad)."""
    Cout, Cin = w.shape[:2]
    K = 9 * Cin
    Kpad = (K + 31) // 32 * 32
    rows = torch.zeros((Cout, Kpad))
    rows[:, :K] = w.permute(0, 2, 3, 1).reshape(Cout, K)
    return rows.cuda(), Kpad


def pack_image(kind, rows, Cin, Cout, Kpad):
    """The kernel's weight image from a NaN-filled buffer."""
    from pointtinybenchmark_amd import _lib, ops
    u = torch.full((16 * Cin * Cout,), float('nan'), device='cuda')
    _lib.call(PACK[kind], ops._ptr(rows), ops._ptr(u), Cin, Cout, Kpad, ops._stream())
    return u


def slots_per_image(kind, H, W):
    from pointtinybenchmark_amd import _lib
    if kind == '32':
        return _lib.call('cpr_conv3x3_wino32_slots', H, W, positive=True)
    return ((H + 15) // 16) * ((W + 15) // 16)


def guarded(shape):
    """A NaN-filled buffer with one image-sized guard before and after, and the slice between them."""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), float('nan'), device='cuda')
    return buf, buf[1:1 + shape[0]]


def guards_intact(buf):
    bits = buf.view(torch.int32)
    return bool((bits[0] == NAN_BITS).all()) and bool((bits[-1] == NAN_BITS).all())


def entry_launch(kind, x, u, out, scale, bias, in_ab, part, N, H, W, Cin, Cout, relu, in_relu, layout):
    from pointtinybenchmark_amd import _lib, ops
    a, b = in_ab if in_ab is not None else (None, None)
    _lib.call(FWD[kind], ops._ptr(x), ops._ptr(u), ops._ptr(out), ops._ptr(scale), ops._ptr(bias), ops._ptr(a), ops._ptr(b), ops._ptr(part),
              N, H, W, Cin, Cout, 1 if relu else 0, int(in_relu), layout, ops._stream())


def run_case(c, inp=None):
    """Both runs of a case -> dict(out NHWC (N, H, W, Cout), part (N * slots, Cout, 2) or None, x NHWC on the device, inp)."""
    from pointtinybenchmark_amd import ops
    f = flags(c)
    inp = inp or make_inputs(c)
    cuda = (lambda t: None if t is None else t.cuda())
    x, scale, bias = cuda(inp['x']), cuda(inp['scale']), cuda(inp['bias'])
    in_ab = None if inp['in_ab'] is None else tuple(t.cuda() for t in inp['in_ab'])
    xin = to_b8(x) if 'inb8' in f else x
    layout = (1 if 'inb8' in f else 0) | (2 if 'outb8' in f else 0)
    oshape = (c.N, c.Cout // 8, c.H, c.W, 8) if 'outb8' in f else (c.N, c.H, c.W, c.Cout)
    nslots = c.N * slots_per_image(c.kernel, c.H, c.W)
    kw = dict(relu='relu' in f, in_relu='inrelu' in f)

    def entry(u):
        buf, out = guarded(oshape)
        part = torch.full((nslots, c.Cout, 2), float('nan'), device='cuda') if 'gn' in f else None
        entry_launch(c.kernel, xin, u, out, scale, bias, in_ab, part, c.N, c.H, c.W, c.Cin, c.Cout, layout=layout, **kw)
        torch.cuda.synchronize()
        assert guards_intact(buf), '%s: the guards around the output were written' % case_id(c)
        return out, part

    if 'entry' in f:
        rows, Kpad = rows_at_kpad(inp['w'])
        u = pack_image(c.kernel, rows, c.Cin, c.Cout, Kpad)
        out1, part1 = entry(u)
    else:
        pc = ops.PackedConv(cuda(inp['w']), 1, 1)
        buf1, out1 = guarded(oshape)
        keep = ops.WINO_TILE[0]
        ops.WINO_TILE[0] = 'auto' if 'auto' in f else c.kernel
        ops.TRACE_CONV_VARIANT[0], ops.TRACE_CONV_VARIANT[1] = True, None
        try:
            fn = ops.conv2d if 'auto' in f else ops.conv3x3_wino
            got = fn(xin, pc, scale=scale, bias=bias, gn_part='gn' in f, out=out1, in_ab=in_ab, out_b8='outb8' in f, **kw)
            variant = ops.TRACE_CONV_VARIANT[1]
            torch.cuda.synchronize()
        finally:
            ops.WINO_TILE[0] = keep
            ops.TRACE_CONV_VARIANT[0] = False
        assert variant == (WORD[c.kernel], layout | (4 if in_ab is not None else 0)), \
            '%s: expected the %s kernel, the launch was %r' % (case_id(c), WORD[c.kernel], variant)
        part1 = got[1] if 'gn' in f else None
        assert (got[0] if 'gn' in f else got) is out1 and guards_intact(buf1)
        u = pc.wino if c.kernel == '64' else pc.wino32
    out2, part2 = entry(u)
    assert torch.equal(out1.view(torch.int32), out2.view(torch.int32)), '%s: the second run differs from the first' % case_id(c)
    if 'gn' in f:
        assert tuple(part1.shape) == (nslots, c.Cout, 2)
        assert torch.equal(part1.view(torch.int32), part2.view(torch.int32)), '%s: the second run\'s slots differ' % case_id(c)
    return dict(out=from_b8(out2) if 'outb8' in f else out2, part=part2, x=x, inp=inp)


def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def states(c, ncu):
    k = WR.run_kinds(WR.walk(c.N, c.H, c.W, c.Cout, c.kernel, ncu))
    return 'T=%d runs=%s%s%s' % (WR.tiles(c.N, c.H, c.W, c.Cout, c.kernel), sorted(k['lens']), ' change' if k['change'] else '', ' stay' if k['stay'] else '')


@pytest.mark.gpu
def test_table_reaches_every_state_on_this_device():
    ncu = device_cus()
    missing = [n for n, ok in coverage(CASES, ncu).items() if not ok]
    assert not missing, 'at %d CUs the table no longer reaches: %s' % (ncu, '; '.join(missing))


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_wino_instance_vs_fp64(c):
    f = flags(c)
    name = case_id(c)
    t0 = time.time()
    g = run_case(c)
    inp, out = g['inp'], g['out']
    ncu = device_cus()
    m, rgs = WR.sample(c.N, c.H, c.W, c.Cout, c.kernel, ncu, seed=seed(c))
    r = WR.reference(g['x'], inp['w'], m, scale=inp['scale'], bias=inp['bias'], relu='relu' in f, in_ab=inp['in_ab'], in_relu='inrelu' in f)
    assert not bool(torch.isnan(out).any()), '%s: output elements were not written' % name
    got = R._rows(out, m)
    q2 = float(R.ratio(got, r['ref'], r['bar_direct']).max())
    worst_s = 0.0
    print('\nWINO %s bar1 %.4f bar2 %.4f%s  %s  %s' % (c.kernel, float(R.ratio(got, r['ref'], r['bar_wino']).max()), q2,
                                                     '' if takes_bar2(c) else ' (not asserted)', states(c, ncu), name))
    OHW = (c.H, c.W)
    WR.check(name + ' bar 1', got, r['ref'], r['bar_wino'], m=m, OHW=OHW)
    if takes_bar2(c):
        WR.check(name + ' bar 2', got, r['ref'], r['bar_direct'], m=m, OHW=OHW)
    if 'gn' in f:
        part = g['part'].cpu().double()
        assert not bool(torch.isnan(part).any()), '%s: statistics slots were not written' % name
        sref, sbar = WR.slot_refs(r, m, rgs, c.N, c.H, c.W, c.kernel)
        worst_s = WR.check(name + ' slots', part[torch.as_tensor(rgs)].reshape(len(rgs), -1), sref.reshape(len(rgs), -1), sbar.reshape(len(rgs), -1))
    print('WINO %s slots %.4f  %.2f s  %d pixels %d regions  %s' % (c.kernel, worst_s, time.time() - t0, len(m), len(rgs), name))


# ---- batch independence -----------------------------------------------------------------------------------------------------
BATCH_CASES = [
    Case('64', 3, 80, 80, 32, 256, '', 'runs of 1 and 2'),
    Case('64', 7, 44, 40, 64, 384, 'inab inrelu bias gn', 'table swap'),
    Case('32', 9, 40, 40, 64, 256, '', 'runs of 1 and 2'),
    Case('32', 11, 36, 44, 64, 320, 'inab inrelu bias gn', 'table reload'),
]


@pytest.mark.gpu
@pytest.mark.parametrize('c', BATCH_CASES, ids=case_id)
def test_image_of_a_batch_equals_its_single_image_run(c):
    """Images 0, 1 and N - 1 of the batch equal their single-image launches bit for bit, outputs and slots: the tile walk changes
    completely with N (a run of the batch launch crosses images, the single-image launch has one tile per workgroup), the arithmetic
    of a tile must not."""
    from pointtinybenchmark_amd import ops
    f = flags(c)
    assert max(WR.run_kinds(WR.walk(c.N, c.H, c.W, c.Cout, c.kernel, device_cus()))['lens']) >= 2
    inp = make_inputs(c)
    x, w, bias = inp['x'].cuda(), inp['w'].cuda(), None if inp['bias'] is None else inp['bias'].cuda()
    ab = None if inp['in_ab'] is None else tuple(t.cuda() for t in inp['in_ab'])
    if ab is not None:
        assert all(not torch.equal(v[i], v[j]) for v in ab for i in range(c.N) for j in range(i))      # a row of its own per image
    pc = ops.PackedConv(w, 1, 1)
    keep = ops.WINO_TILE[0]
    ops.WINO_TILE[0] = c.kernel
    try:
        def run(n0, n1):
            y = ops.conv3x3_wino(x[n0:n1].contiguous(), pc, None, bias, 'relu' in f, gn_part='gn' in f,
                                 in_ab=None if ab is None else (ab[0][n0:n1].contiguous(), ab[1][n0:n1].contiguous()), in_relu='inrelu' in f)
            return y if 'gn' in f else (y, None)
        yb, pb = run(0, c.N)
        P = slots_per_image(c.kernel, c.H, c.W)
        for n in (0, 1, c.N - 1):
            y1, p1 = run(n, n + 1)
            assert torch.equal(y1[0], yb[n]), 'image %d of the batch differs from its single-image run' % n
            if 'gn' in f:
                assert torch.equal(p1, pb[n * P:(n + 1) * P]), 'slots of image %d of the batch differ from its single-image run' % n
    finally:
        ops.WINO_TILE[0] = keep


# ---- weight images ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('kind,Cin,Cout', [('64', 48, 192), ('64', 64, 128), ('32', 24, 128), ('32', 40, 64), ('32', 64, 192)])
def test_weight_image_vs_fp64(kind, Cin, Cout):
    """U from the pack kernels against fp64 G g G^T through the restated layout: every element of a NaN-filled buffer written, the
    layout a bijection, the bar from the counted roundings of the two passes (wino_fp64_ref.pack_reference)."""
    g = torch.Generator().manual_seed(Cin * 7 + Cout)
    w = torch.randn((Cout, Cin, 3, 3), generator=g)
    rows, Kpad = rows_at_kpad(w)
    u = pack_image(kind, rows, Cin, Cout, Kpad).cpu()
    assert not bool(torch.isnan(u).any()), 'elements of the weight image were not written'
    idx = WR.u_layout(kind, Cin, Cout)
    assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(16 * Cin * Cout))
    ref, bar = WR.pack_reference(w)
    got = u[torch.as_tensor(idx)].double()
    worst = WR.check('weight image %s %d -> %d' % (kind, Cin, Cout), got.reshape(16, -1), ref.reshape(16, -1), bar.reshape(16, -1))
    print('\nWINO %s pack %d -> %d worst %.4f' % (kind, Cin, Cout, worst))


@pytest.mark.gpu
def test_refreshed_weight_images_equal_a_fresh_pack():
    """After a weight change layers._PackCache.refresh_all (PackJob.refresh_images) leaves the bits of a freshly built PackedConv in
    both weight images, and the next convolution with the refreshed pack equals the fresh one bit for bit."""
    from pointtinybenchmark_amd import layers, ops
    g = torch.Generator().manual_seed(77)
    conv = torch.nn.Conv2d(64, 128, 3, 1, 1, bias=False).cuda()
    w2 = (torch.randn((128, 64, 3, 3), generator=g) * 0.05).cuda()
    x = torch.randn((2, 24, 40, 64), generator=g).cuda()
    cache = layers._PackCache()
    keep = ops.WINO_TILE[0]
    try:
        pc = layers.packed_conv(cache, conv)
        old = {}
        for kind in ('64', '32'):
            ops.WINO_TILE[0] = kind
            old[kind] = ops.conv3x3_wino(x, pc)
        assert pc.wino is not None and pc.wino32 is not None
        ptrs = (pc.w.data_ptr(), pc.wino.data_ptr(), pc.wino32.data_ptr())
        with torch.no_grad():
            conv.weight.copy_(w2)
        cache.refresh_all()
        assert layers.packed_conv(cache, conv) is pc and ptrs == (pc.w.data_ptr(), pc.wino.data_ptr(), pc.wino32.data_ptr())
        fresh = ops.PackedConv(w2, 1, 1)
        for kind in ('64', '32'):
            ops.WINO_TILE[0] = kind
            y_fresh = ops.conv3x3_wino(x, fresh)
            y = ops.conv3x3_wino(x, pc)
            assert torch.equal(y, y_fresh) and not torch.equal(y, old[kind])
        torch.cuda.synchronize()
        assert torch.equal(pc.w, fresh.w) and torch.equal(pc.wino, fresh.wino) and torch.equal(pc.wino32, fresh.wino32)
    finally:
        ops.WINO_TILE[0] = keep


# ---- argument refusals (no launch, so no GPU needed) ------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_any_launch():
    from pointtinybenchmark_amd import _lib
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    N, H, W = 1, 8, 8
    buf = {n: torch.zeros(sz, device=dev) for n, sz in (('x', N * H * W * 528), ('u', 16 * 528 * 128), ('y', N * H * W * 128), ('v', 528),
                                                        ('part', 128 * 2))}
    P = {n: t.data_ptr() for n, t in buf.items()}

    def refused(kind, x='x', u='u', y='y', a=None, b=None, N=N, H=H, W=W, Cin=64, Cout=64, fl=0, layout=0):
        p = (lambda n: None if n is None else P[n])
        with pytest.raises(_lib.CprHipError, match='invalid argument'):
            _lib.call(FWD[kind], p(x), p(u), p(y), P['v'], P['v'], p(a), p(b), P['part'], N, H, W, Cin, Cout, fl, 0, layout, None)

    for kind in ('64', '32'):
        for null in ('x', 'u', 'y'):
            refused(kind, **{null: None})
        refused(kind, Cout=96)
        refused(kind, a='v')                     # in_a without in_b
        refused(kind, fl=2)
        refused(kind, fl=8)
        refused(kind, layout=4)
        for dim in ('N', 'H', 'W', 'Cin', 'Cout'):
            refused(kind, **{dim: 0})
            refused(kind, **{dim: -1})
    refused('64', Cin=24)
    refused('64', Cin=16)
    refused('32', Cin=12)
    refused('64', Cin=528, a='v', b='v')
    refused('32', Cin=264, a='v', b='v')
    for kind in ('64', '32'):
        for bad in (dict(wgt=None), dict(u=None), dict(Cin=0), dict(Cout=96), dict(Kpad=9 * 64 - 1)):
            a = dict(wgt=P['x'], u=P['u'], Cin=64, Cout=64, Kpad=9 * 64)
            a.update(bad)
            with pytest.raises(_lib.CprHipError, match='invalid argument'):
                _lib.call(PACK[kind], a['wgt'], a['u'], a['Cin'], a['Cout'], a['Kpad'], None)
