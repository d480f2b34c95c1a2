"""-m gpu: the weight-pack kernels through their C entry points -- ``cpr_pack_weights[_multi]``, ``cpr_pack_weights_bf16[_multi]``
(csrc/pack.hip), ``cpr_pack_weights_grouped[_multi]`` (csrc/conv_group.hip), ``cpr_res2_pack_weights`` (csrc/res2net.hip) and
``cpr_dw3x3_pack`` (csrc/mbv2.hip) -- against the exact images and the case tables of tests/pack_exact_ref.py.  A pack is a permutation,
at most one fp32 multiply and at most one rounding, so every comparison is on the bits (uint32 / uint16 views); nothing has a tolerance.

Every output is a slice of an arena of 0xFF bytes (NaN as fp32 and as bf16) with at least 64 guard elements on either side.  After each
launch every byte of the arena outside the slices must still be 0xFF and every element of a slice must equal the restated image: a pad
that a kernel does not write shows as 0xFFFFFFFF where the image has +0.0.  Each case runs a second time on the same buffers after its
master and scale changed in place -- the in-place refresh -- and must give the image of the new values.  The masters and scales sit
between 0xFF bytes too, so a read past their end brings NaN into the image.  Where ``ops`` takes the shape, its class builds the same
bits.  The multi-job tables are built with the real ``layers.PackJob.row`` / ``GroupPackJob.row`` and uploaded as
``_PackCache.refresh_all`` uploads them; each job must equal its single-tensor launch and the restated image.

tests/test_pack_instances_host.py holds the references to independent constructions and asserts the tables' coverage without a GPU.
The file prints its wall time when its last test is done (pytest -s shows it); CHANGELOG.md records it."""
import time
import types

import numpy as np
import pytest
import torch

from tests import pack_exact_ref as R

pytestmark = pytest.mark.gpu

GUARD_BYTES = 256            # >= 64 elements of either type before and after every slice
INPUT_GUARD_BYTES = 4096     # 0xFF bytes before and after every master and scale
T0 = [None]


@pytest.fixture(scope='module', autouse=True)
def _wall_time():
    T0[0] = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print('\ntests/test_gpu_pack_instances.py: %.1f s wall time' % (time.perf_counter() - T0[0]))


# ---- plumbing ----------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    from pointtinybenchmark_amd import _lib
    return _lib.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _stream())


def dev(a):
    """A master or a scale on the device, itself in the middle of 0xFF bytes: a read past its end finds NaN, not whatever the allocator
    left there (zeros, as often as not, which a pad would hide)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    nbytes = t.numel() * t.element_size()
    buf = torch.full((2 * INPUT_GUARD_BYTES + (nbytes + 255) // 256 * 256,), 0xFF, dtype=torch.uint8, device='cuda')
    view = buf[INPUT_GUARD_BYTES:INPUT_GUARD_BYTES + nbytes].view(t.dtype).view(t.shape)
    view.copy_(t)
    return view


class Arena:
    """Slices in the middle of one buffer of 0xFF bytes.  specs: (elements, dtype) per slice."""

    def __init__(self, specs):
        pos, self.spans = GUARD_BYTES, []
        for n, dtype in specs:
            nbytes = n * torch.empty((), dtype=dtype).element_size()
            self.spans.append((pos, nbytes, dtype))
            pos += (nbytes + 255) // 256 * 256 + GUARD_BYTES
        self.buf = torch.full((pos,), 0xFF, dtype=torch.uint8, device='cuda')
        self.views = [self.buf[o:o + nb].view(dtype) for o, nb, dtype in self.spans]
        self.outside = np.ones(pos, dtype=bool)
        for o, nb, _ in self.spans:
            self.outside[o:o + nb] = False

    def intact(self, name):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        bad = np.flatnonzero(self.outside & (b != 0xFF))
        assert bad.size == 0, '%s: %d bytes outside the outputs changed, the first at byte %d' % (name, bad.size, bad[0])


def bits_of(t):
    """Device tensor -> numpy uint32 / uint16 bits."""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32).numpy().view(np.uint32) if t.dtype == torch.float32 else t.view(torch.int16).numpy().view(np.uint16)


def want_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(name, got, want):
    g, w = bits_of(got).reshape(-1), want_bits(want).reshape(-1)
    assert g.dtype == w.dtype and g.size == w.size, '%s: %s x %d != %s x %d' % (name, g.dtype, g.size, w.dtype, w.size)
    ne = np.flatnonzero(g != w)
    assert ne.size == 0, '%s: %d of %d elements differ, the first at %d: 0x%X != 0x%X' % (name, ne.size, g.size, ne[0], g[ne[0]], w[ne[0]])


def inputs(shape, n_scale, use_scale, seed):
    w = R.master(shape, seed)
    s = R.scale_of(n_scale, seed) if use_scale else None
    return w, s


def twice(name, arena, launch, reference, shape, n_scale, use_scale, seed):
    """launch(w_dev, s_dev) into the arena; the views must equal reference(w, s) (a list of images, one per view); then again after
    the master and the scale changed IN PLACE.  Returns the device master and scale holding the second values."""
    w, s = inputs(shape, n_scale, use_scale, seed)
    wd, sd = dev(w), None if s is None else dev(s)
    for rnd in range(2):
        if rnd:
            w, s = inputs(shape, n_scale, use_scale, seed + 1000)
            wd.copy_(torch.from_numpy(w))
            if sd is not None:
                sd.copy_(torch.from_numpy(s))
        launch(wd, sd)
        arena.intact('%s run %d' % (name, rnd))
        for i, (view, want) in enumerate(zip(arena.views, reference(w, s))):
            same('%s run %d image %d' % (name, rnd, i), view, want)
    return wd, sd


# ---- dense fp32 ----------------------------------------------------------------------------------------------------
def d_id(c):
    return '%dx%dx%dx%d-t%d-s%d%s' % (c['shape'] + (c['transpose'], c['scale'], '-frag' if c['frag'] else ''))


def launch32(wd, sd, out, c):
    O, I, KH, KW = c['shape']
    _, _, colsp, Kpad = R.dense32_geometry(c)
    call('cpr_pack_weights', wd, sd, out, O, I, KH, KW, colsp, Kpad, c['transpose'])


@pytest.mark.parametrize('c', R.DENSE32, ids=d_id)
def test_dense_fp32_pack(c):
    from pointtinybenchmark_amd import ops
    O, I, KH, KW = c['shape']
    rows, cols, colsp, Kpad = R.dense32_geometry(c)
    arena = Arena([(rows * Kpad, torch.float32)])
    wd, sd = twice(d_id(c), arena, lambda w, s: launch32(w, s, arena.views[0], c),
                   lambda w, s: [R.dense_f32(w, s, c['transpose'], colsp, Kpad)], c['shape'], O, c['scale'], 11)
    if c['transpose']:
        pc = ops.PackedConv.for_dgrad(wd, 0, sd, pad_override=None if KH == KW else 0)
    else:
        pc = ops.PackedConv(wd, 1, 0)
    torch.cuda.synchronize()
    assert (pc.Cout, pc.Cin, pc.Kpad) == (rows, colsp, Kpad)
    same(d_id(c) + ' ops', pc.w, bits_of(arena.views[0]))


# ---- dense bf16 ----------------------------------------------------------------------------------------------------
def geometry16(c):
    rows, cols = R.dense_dims(c['shape'], c['transpose'])
    return rows, cols, c['shape'][2] * c['shape'][3] * cols


def launch16(wd, sd, out, frag, c):
    O, I, KH, KW = c['shape']
    call('cpr_pack_weights_bf16', wd, sd, out, frag, O, I, KH, KW, c['transpose'])


def images16(w, s, c, with_frag):
    img = R.dense_bf16(w, s, c['transpose'])
    return [img, R.frag_of(img)] if with_frag else [img]


# with and without a fragment image; the shapes the entry point refuses one for (rows % 64, K % 16) run without only
DENSE16_RUNS = [(c, f) for c in R.DENSE16 for f in ((False, True) if c['frag'] else (False,))]


@pytest.mark.parametrize('c,with_frag', DENSE16_RUNS, ids=[d_id(dict(c, frag=f)) for c, f in DENSE16_RUNS])
def test_dense_bf16_pack(c, with_frag):
    from pointtinybenchmark_amd import ops
    O, I, KH, KW = c['shape']
    rows, cols, K = geometry16(c)
    arena = Arena([(rows * K, torch.bfloat16)] + ([(rows * K, torch.bfloat16)] if with_frag else []))
    frag = arena.views[1] if with_frag else None
    wd, sd = twice(d_id(c), arena, lambda w, s: launch16(w, s, arena.views[0], frag, c), lambda w, s: images16(w, s, c, with_frag),
                   c['shape'], O, c['scale'], 23)
    if c['entry'] != 'ops':
        return
    pc = ops.PackedConv.for_dgrad_bf16(wd, 0, scale=sd) if c['transpose'] else ops.PackedConv(wd, 1, 0, torch.bfloat16)
    torch.cuda.synchronize()
    same(d_id(c) + ' ops', pc.w, bits_of(arena.views[0]))
    assert (pc.wfrag is not None) == (rows % 256 == 0 and K % 64 == 0)
    if pc.wfrag is not None:
        built = pc.wfrag
        same(d_id(c) + ' ops frag', built, R.frag_of(bits_of(pc.w)))
        pc.wfrag = None                               # frag_image now builds it the second way: view + permute of pc.w
        second = pc.frag_image()
        torch.cuda.synchronize()
        assert second is not built and second.shape == built.shape
        same(d_id(c) + ' frag_image', second, bits_of(built))


# ---- special values --------------------------------------------------------------------------------------------------
SPECIAL_SHAPE = (64, 64, 1, 1)
SPECIAL_CASE = R._d(SPECIAL_SHAPE)


def run_specials(patterns):
    """The three packs of a master tiled with ``patterns`` -> (master bits, fp32 forward, fp32 transposed without scale, bf16 forward),
    each as the bits the conv would read, and the fp32 bits each element came from."""
    w = R.tiled(patterns, SPECIAL_SHAPE)
    wd = dev(w)
    arena = Arena([(4096, torch.float32), (4096, torch.float32), (4096, torch.bfloat16)])
    launch32(wd, None, arena.views[0], SPECIAL_CASE)
    launch32(wd, None, arena.views[1], dict(SPECIAL_CASE, transpose=1))
    launch16(wd, None, arena.views[2], None, SPECIAL_CASE)
    arena.intact('specials')
    src = w.view(np.uint32).reshape(64, 64)
    return src, src.T, [bits_of(v).reshape(64, 64) for v in arena.views]


def check_specials(patterns):
    src, src_t, (fwd, tr, b16) = run_specials(patterns)
    print('patterns       :', ' '.join('%08X' % p for p in patterns))
    print('fp32 copy      :', ' '.join('%08X' % v for v in fwd.reshape(-1)[:len(patterns)]))
    print('fp32 * 1.f     :', ' '.join('%08X' % v for v in tr.T.reshape(-1)[:len(patterns)]))
    print('bf16           :', ' '.join('%04X' % v for v in b16.reshape(-1)[:len(patterns)]))
    print('bf16 (integer) :', ' '.join('%04X' % v for v in R.bf16_bits(src.view(np.float32)).reshape(-1)[:len(patterns)]))
    assert np.array_equal(fwd, src), 'the forward fp32 pack is a copy: every pattern, NaN payload included'
    nan = R.is_nan32(src_t)
    assert np.array_equal(tr[~nan], src_t[~nan]) and R.is_nan32(tr[nan]).all(), 'a multiply by 1.f changed a value'
    want = R.bf16_bits(src.view(np.float32))
    nan = R.is_nan32(src)
    assert np.array_equal(b16[~nan], want[~nan]) and R.is_nan16(b16[nan]).all(), 'bf16 rounding differs from nearest-even'


def test_special_values_round_and_copy_exactly():
    """Ties to even in both directions, the neighbours of a tie, the largest finite values (to inf), signed zeros, infinities, the
    smallest normal and a NaN."""
    check_specials([p for p in R.SPECIALS if p not in R.SUBNORMALS])


def test_subnormals_survive_the_packs():
    """fp32 subnormals through the copy, the multiply by 1.f and the bf16 rounding (0x007FFFFF rounds up into the normals): a device-side
    flush to zero fails here and nowhere else."""
    check_specials(list(R.SUBNORMALS))


# ---- grouped, Res2Net, depthwise ----------------------------------------------------------------------------------------------------
def m_id(m):
    return 'fwd' if not m[0] else ('dgrad-scale' if m[1] else 'dgrad')


@pytest.mark.parametrize('mode', R.MODES, ids=m_id)
@pytest.mark.parametrize('C,cg', R.GROUPED)
def test_grouped_pack(C, cg, mode):
    from pointtinybenchmark_amd import ops
    transpose, use_scale = mode
    arena = Arena([(9 * cg * C, torch.float32)])
    name = 'grouped (%d,%d) %s' % (C, cg, m_id(mode))
    wd, sd = twice(name, arena, lambda w, s: call('cpr_pack_weights_grouped', w, s, arena.views[0], C, cg, transpose),
                   lambda w, s: [R.grouped(w, s, cg, transpose)], (C, cg, 3, 3), C, use_scale, 31)
    pc = ops.PackedConv.for_dgrad_grouped(wd, C // cg, sd) if transpose else ops.PackedConv(wd, 1, 1, groups=C // cg)
    torch.cuda.synchronize()
    same(name + ' ops', pc.w, bits_of(arena.views[0]))


@pytest.mark.parametrize('mode', R.MODES, ids=m_id)
@pytest.mark.parametrize('width', R.RES2)
def test_res2_pack(width, mode):
    from pointtinybenchmark_amd import ops
    transpose, use_scale = mode
    arena = Arena([(9 * width * width, torch.float32)])
    name = 'res2 %d %s' % (width, m_id(mode))
    wd, sd = twice(name, arena, lambda w, s: call('cpr_res2_pack_weights', w, s, arena.views[0], width, transpose),
                   lambda w, s: [R.res2(w, s, transpose)], (width, width, 3, 3), width, use_scale, 41)
    pk = ops.Res2Pack(wd, sd, transpose=bool(transpose))
    torch.cuda.synchronize()
    same(name + ' ops', pk.w, bits_of(arena.views[0]))


@pytest.mark.parametrize('use_scale', [False, True], ids=['noscale', 'scale'])
@pytest.mark.parametrize('C', R.DW)
def test_depthwise_pack(C, use_scale):
    from pointtinybenchmark_amd import ops
    Cp = R.pad32(C)
    arena = Arena([(9 * Cp, torch.float32)])
    name = 'dw %d s%d' % (C, use_scale)
    wd, sd = twice(name, arena, lambda w, s: call('cpr_dw3x3_pack', w, s, arena.views[0], C), lambda w, s: [R.dw(w, s, Cp)],
                   (C, 1, 3, 3), C, use_scale, 53)
    pk = ops.DwPack(wd, sd)
    torch.cuda.synchronize()
    assert pk.Cp == Cp
    same(name + ' ops', pk.w, bits_of(arena.views[0]))
    # DwPack.repack: the same buffer, after the weight changed
    before = pk.w.data_ptr()
    w2, s2 = inputs((C, 1, 3, 3), C, use_scale, 2053)
    wd.copy_(torch.from_numpy(w2))
    if sd is not None:
        sd.copy_(torch.from_numpy(s2))
    assert pk.repack(wd, sd) is pk and pk.w.data_ptr() == before
    torch.cuda.synchronize()
    same(name + ' repack', pk.w, R.dw(w2, s2, Cp))


# ---- multi-job kernels ----------------------------------------------------------------------------------------------------
class MultiKind:
    """One of the three multi-job launches: its job class, how a table entry becomes inputs, outputs, a single-tensor launch and the
    restated images."""

    def __init__(self, kind):
        from pointtinybenchmark_amd import layers
        self.kind = kind
        self.job_class = layers.GroupPackJob if kind == 'g' else layers.PackJob
        self.entry = {'32': 'cpr_pack_weights_multi', '16': 'cpr_pack_weights_bf16_multi', 'g': 'cpr_pack_weights_grouped_multi'}[kind]
        self.row = {'32': layers.PackJob._ROW32, '16': layers.PackJob._ROW16, 'g': layers.GroupPackJob._ROWG}[kind]

    def shape(self, c):
        return (c['C'], c['cg'], 3, 3) if self.kind == 'g' else c['shape']

    def n_scale(self, c):
        return self.shape(c)[0]

    def specs(self, c):
        if self.kind == '32':
            rows, _, _, Kpad = R.dense32_geometry(c)
            return [(rows * Kpad, torch.float32)]
        if self.kind == '16':
            rows, _, K = geometry16(c)
            return [(rows * K, torch.bfloat16)] * (2 if c['frag'] else 1)
        return [(9 * c['cg'] * c['C'], torch.float32)]

    def threads(self, c):
        return {'32': R.dense32_threads, '16': R.dense16_threads, 'g': R.grouped_threads}[self.kind](c)

    def stub(self, c, views):
        """What PackJob reads of an ops.PackedConv, with the images in the arena."""
        if self.kind == '32':
            rows, _, colsp, Kpad = R.dense32_geometry(c)
            return types.SimpleNamespace(dtype=torch.float32, groups=1, Cout=rows, Cin=colsp, Kpad=Kpad, w=views[0], wfrag=None)
        if self.kind == '16':
            rows, _, K = geometry16(c)
            return types.SimpleNamespace(dtype=torch.bfloat16, groups=1, Cout=rows, Kpad=K, w=views[0], wfrag=views[1] if c['frag'] else None)
        return types.SimpleNamespace(dtype=torch.float32, groups=c['C'] // c['cg'], C=c['C'], cg=c['cg'], w=views[0], wfrag=None)

    def single(self, c, wd, sd, views):
        if self.kind == '32':
            launch32(wd, sd, views[0], c)
        elif self.kind == '16':
            launch16(wd, sd, views[0], views[1] if c['frag'] else None, c)
        else:
            call('cpr_pack_weights_grouped', wd, sd, views[0], c['C'], c['cg'], c['transpose'])

    def images(self, c, w, s):
        if self.kind == '32':
            _, _, colsp, Kpad = R.dense32_geometry(c)
            return [R.dense_f32(w, s, c['transpose'], colsp, Kpad)]
        if self.kind == '16':
            return images16(w, s, c, c['frag'])
        return [R.grouped(w, s, c['cg'], c['transpose'])]


MULTI = [(k, name) for k, tables in (('32', R.MULTI32), ('16', R.MULTI16), ('g', R.MULTIG)) for name in tables]


@pytest.mark.parametrize('kind,table', MULTI, ids=['%s-%s' % m for m in MULTI])
def test_multi_job_pack(kind, table):
    mk = MultiKind(kind)
    cases = {'32': R.MULTI32, '16': R.MULTI16, 'g': R.MULTIG}[kind][table]
    specs = [mk.specs(c) for c in cases]
    arena = Arena([s for sp in specs for s in sp])          # every job's outputs in one guarded arena
    alone = Arena([s for sp in specs for s in sp])          # the single-tensor launches' outputs
    views, lone, at = [], [], 0
    for sp in specs:
        views.append(arena.views[at:at + len(sp)])
        lone.append(alone.views[at:at + len(sp)])
        at += len(sp)
    host = [inputs(mk.shape(c), mk.n_scale(c), c['scale'], 61 + i) for i, c in enumerate(cases)]
    wds = [dev(w) for w, _ in host]
    sds = [None if s is None else dev(s) for _, s in host]
    jobs = []
    for c, wd, sd, v in zip(cases, wds, sds, views):
        fold = None if sd is None else types.SimpleNamespace(value=(sd,))
        jobs.append(mk.job_class(wd, mk.stub(c, v), c['transpose'], fold))
    rows, block0 = [], 0
    for j in jobs:
        row, block0 = j.row(j.ptrs(), block0)
        rows.append(row)
    total_blocks = block0
    # the table has the boundaries the case claims: parsed back from the very bytes that are uploaded
    fields = [mk.row.unpack(r) for r in rows]
    spans = [(f[-1], f[3]) if kind == '32' else (f[-3], f[-2]) for f in fields]
    owner = R.block_to_job(spans)
    assert len(owner) == total_blocks and [s[1] for s in spans] == [R.job_blocks(mk.threads(c)) for c in cases]
    assert [int((owner == i).sum()) for i in range(len(cases))] == [s[1] for s in spans]
    if table == 'two_one_block':
        assert list(owner) == [0, 1]
    for c, f in zip(cases, fields):          # null scale / frag pointers exactly where the case says
        assert f[0] != 0 and f[2] != 0 and (f[1] != 0) == bool(c['scale'])
        if kind == '16':
            assert (f[3] != 0) == bool(c['frag'])
    dev_table = torch.frombuffer(bytearray(b''.join(rows)), dtype=torch.uint8).cuda()      # as _PackCache.refresh_all uploads it
    for rnd in range(2):
        if rnd:                                  # every master and scale changes in place; the table and the pointers stay
            host = [inputs(mk.shape(c), mk.n_scale(c), c['scale'], 1061 + i) for i, c in enumerate(cases)]
            for (w, s), wd, sd in zip(host, wds, sds):
                wd.copy_(torch.from_numpy(w))
                if sd is not None:
                    sd.copy_(torch.from_numpy(s))
        call(mk.entry, dev_table, len(jobs), total_blocks)
        arena.intact('%s %s run %d' % (kind, table, rnd))
        for c, wd, sd, v in zip(cases, wds, sds, lone):
            mk.single(c, wd, sd, v)
        alone.intact('%s %s single run %d' % (kind, table, rnd))
        for i, (c, (w, s)) in enumerate(zip(cases, host)):
            for got, one, want in zip(views[i], lone[i], mk.images(c, w, s)):
                name = '%s %s run %d job %d' % (kind, table, rnd, i)
                same(name + ' against the restated image', got, want)
                same(name + ' against the single-tensor kernel', got, bits_of(one))


# ---- _PackCache at small scale ----------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().float().cpu().numpy()


def _perturb(mods, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mods:
            for p in m.parameters():
                p.copy_((torch.randn(p.shape, generator=g) * 0.05 + (1.0 if p.dim() == 1 and p is getattr(m, 'weight', None) else 0.0)).cuda())
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_((torch.randn(m.running_mean.shape, generator=g) * 0.1).cuda())
                m.running_var.copy_((torch.rand(m.running_var.shape, generator=g) + 0.5).cuda())


def test_pack_cache_refreshes_six_small_layers_in_place():
    from pointtinybenchmark_amd import layers, ops
    nn = torch.nn
    conv3 = nn.Conv2d(32, 64, 3, padding=1, bias=False).cuda()
    stem = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda()
    conv16 = nn.Conv2d(64, 256, 1, bias=False).cuda()
    convg = nn.Conv2d(48, 48, 3, padding=1, groups=2, bias=False).cuda()
    convd, bnd = nn.Conv2d(32, 64, 3, padding=1, bias=False).cuda(), nn.BatchNorm2d(64).cuda()
    bnu = nn.BatchNorm2d(40).cuda()
    extra = nn.Conv2d(64, 32, 1, bias=False).cuda()
    mods = [conv3, stem, conv16, convg, convd, bnd, bnu, extra]
    _perturb(mods, 71)
    cache = layers._PackCache()

    def build(with_extra):
        got = dict(conv3=layers.packed_conv(cache, conv3), stem=layers.packed_conv(cache, stem),
                   conv16=layers.packed_conv(cache, conv16, torch.bfloat16), convg=layers.packed_conv(cache, convg),
                   fold_d=layers.folded_bn(cache, bnd), dgrad=layers.dgrad_packed(cache, convd, bnd), fold_u=layers.folded_bn(cache, bnu))
        if with_extra:
            got['extra'] = layers.packed_conv(cache, extra)
        return got

    def check(got, tag):
        torch.cuda.synchronize()
        for bn, key in ((bnd, 'fold_d'), (bnu, 'fold_u')):
            sc, sh, _ = ops.bn_fold(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
            same('%s %s scale' % (tag, key), got[key][0], bits_of(sc))
            same('%s %s shift' % (tag, key), got[key][1], bits_of(sh))
        scale = _np(got['fold_d'][0])
        dense = [('conv3', conv3, 0, None), ('stem', stem, 0, None), ('dgrad', convd, 1, scale)] + \
            ([('extra', extra, 0, None)] if 'extra' in got else [])
        for key, conv, transpose, s in dense:
            pc, w = got[key], _np(conv.weight)
            fresh = ops.PackedConv.for_dgrad(conv.weight, conv.padding[0], got['fold_d'][0]) if transpose else \
                ops.PackedConv(conv.weight, conv.stride[0], conv.padding[0])
            same('%s %s fresh' % (tag, key), pc.w, bits_of(fresh.w))
            same('%s %s image' % (tag, key), pc.w, R.dense_f32(w, s, transpose, pc.Cin, pc.Kpad))
        pc = got['conv16']
        fresh = ops.PackedConv(conv16.weight, 1, 0, torch.bfloat16)
        img = R.dense_bf16(_np(conv16.weight), None, 0)
        assert pc.wfrag is not None
        same(tag + ' conv16 fresh', pc.w, bits_of(fresh.w))
        same(tag + ' conv16 fresh frag', pc.wfrag, bits_of(fresh.wfrag))
        same(tag + ' conv16 image', pc.w, img)
        same(tag + ' conv16 frag image', pc.wfrag, R.frag_of(img))
        pc = got['convg']
        same(tag + ' convg fresh', pc.w, bits_of(ops.PackedConv(convg.weight, 1, 1, groups=2).w))
        same(tag + ' convg image', pc.w, R.grouped(_np(convg.weight), None, 24, 0))

    first = build(False)
    check(first, 'built')
    assert len(cache._jobs) == 7 and cache._tables is None
    held = {k: (v.w.data_ptr() if hasattr(v, 'w') else v[0].data_ptr()) for k, v in first.items()}

    def refresh(seed, with_extra):
        _perturb(mods, seed)                 # 1. every parameter changes in place
        layers.bump_weight_epoch()           # 2.
        cache.refresh_all()                  # 3.
        got = build(with_extra)              # hits: the refreshed values themselves, nothing rebuilt
        return got

    second = refresh(72, False)
    assert all(second[k] is first[k] for k in first), 'a refreshed entry was rebuilt'
    assert {k: (v.w.data_ptr() if hasattr(v, 'w') else v[0].data_ptr()) for k, v in second.items()} == held
    check(second, 'refreshed')
    tables = cache._tables
    assert tables is not None and sorted(t[0] for t in tables[1]) == sorted(
        ['cpr_bn_fold_multi', 'cpr_pack_weights_multi', 'cpr_pack_weights_bf16_multi', 'cpr_pack_weights_grouped_multi'])
    assert {t[0]: t[2] for t in tables[1]} == {'cpr_bn_fold_multi': 2, 'cpr_pack_weights_multi': 3, 'cpr_pack_weights_bf16_multi': 1,
                                               'cpr_pack_weights_grouped_multi': 1}
    third = refresh(73, False)
    assert cache._tables is tables, 'a second refresh_all rebuilt the job tables'
    assert all(third[k] is first[k] for k in first)
    check(third, 'refreshed again')
    seventh = build(True)                    # a seventh layer: its job drops the tables
    assert cache._tables is None and len(cache._jobs) == 8
    fourth = refresh(74, True)
    assert cache._tables is not None and cache._tables is not tables
    assert {t[0]: t[2] for t in cache._tables[1]}['cpr_pack_weights_multi'] == 4
    assert all(fourth[k] is seventh[k] for k in seventh)
    check(fourth, 'seven layers')
