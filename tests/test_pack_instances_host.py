"""CPU only: the exact pack images of tests/pack_exact_ref.py are the layouts the consumers read -- each against an independent
construction (the CPU branch of ops.PackedConv, the view / permute of ops.PackedConv.frag_image) or against a numpy emulation of how
the consuming kernel addresses its pack, which must reproduce F.conv2d and its autograd input gradient in fp64 -- every image is a
bijection of the master onto its non-pad slots, the job rows of layers.PackJob / GroupPackJob are the structs of the .hip files, the
launch caps are the sources', the case tables reach every state tests/test_gpu_pack_instances.py is there for, four wrong restatements
differ from the right ones on those tables, and the entry points refuse bad arguments before any launch."""
import inspect
import os
import re
import struct
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pack_exact_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pointtinybenchmark_amd', 'csrc')
ERR_ARG = -1001


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _lib():
    from pointtinybenchmark_amd import _lib
    return _lib.load()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bf16_bits_of(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def d_id(c):
    return '%dx%dx%dx%d-t%d-s%d' % (c['shape'] + (c['transpose'], c['scale']))


def _inputs(c, seed=5):
    w = R.master(c['shape'], seed)
    return w, (R.scale_of(c['shape'][0], seed) if c['scale'] else None)


# ---- the bf16 rounding rule ----------------------------------------------------------------------------------------------------
def test_integer_rounding_rule_is_torchs_bfloat16_conversion():
    rng = np.random.default_rng(3)
    b = rng.integers(0, 1 << 32, size=1 << 21, dtype=np.uint64).astype(np.uint32)
    b = np.concatenate([b, np.array(R.SPECIALS, dtype=np.uint32)])
    x = b.view(np.float32)
    got, want = R.bf16_bits(x), _bf16_bits_of(_t(x).to(torch.bfloat16))
    nan = R.is_nan32(b)
    assert np.array_equal(got[~nan], want[~nan]) and R.is_nan16(got[nan]).all() and R.is_nan16(want[nan]).all()
    one = lambda p: int(R.bf16_bits(np.array([p], dtype=np.uint32).view(np.float32))[0])
    assert one(0x3F808000) == 0x3F80 and one(0x3F818000) == 0x3F82          # ties go to the even mantissa, down and up
    assert one(0x3F807FFF) == 0x3F80 and one(0x3F808001) == 0x3F81
    assert one(0x7F7FFFFF) == 0x7F80 and one(0x7F7F8000) == 0x7F80 and one(0x7F7F7FFF) == 0x7F7F
    assert one(0x80000000) == 0x8000 and one(0x00000001) == 0 and one(0x00008000) == 0 and one(0x00018000) == 2
    assert one(0x007FFFFF) == 0x0080 and one(0x807FFFFF) == 0x8080 and len(set(R.SPECIALS)) == len(R.SPECIALS) == 18


# ---- each restated layout against an independent construction ---------------------------------------------------------------------------
@pytest.mark.parametrize('c', [c for c in R.DENSE32 if c['shape'][0] <= 96], ids=d_id)
def test_dense_fp32_image_is_the_cpu_branch_of_packedconv(c):
    from pointtinybenchmark_amd import ops
    w, s = _inputs(c)
    rows, cols, colsp, Kpad = R.dense32_geometry(c)
    img = R.dense_f32(w, s, c['transpose'], colsp, Kpad)
    if c['transpose']:       # the stride-1 conv over dy: the scaled master, taps flipped, in / out swapped (for_dgrad_bf16's docstring)
        ws = _t(w) if s is None else _t(w) * _t(s)[:, None, None, None]
        pc = ops.PackedConv(ws.flip(2, 3).permute(1, 0, 2, 3), 1, 0)
    else:
        pc = ops.PackedConv(_t(w), 1, 0)
    assert (pc.Cout, pc.Cin, pc.Kpad) == (rows, colsp, Kpad)
    assert np.array_equal(_bits(img), _bits(pc.w.numpy()))


@pytest.mark.parametrize('c', [c for c in R.DENSE16 if c['entry'] == 'ops' and c['shape'][0] <= 256], ids=d_id)
def test_dense_bf16_image_is_the_cpu_branch_of_packedconv(c):
    from pointtinybenchmark_amd import ops
    w, s = _inputs(c)
    img = R.dense_bf16(w, s, c['transpose'])
    if c['transpose']:
        ws = _t(w) if s is None else _t(w) * _t(s)[:, None, None, None]
        pc = ops.PackedConv(ws.flip(2, 3).permute(1, 0, 2, 3), 1, 0, torch.bfloat16)
    else:
        pc = ops.PackedConv(_t(w), 1, 0, torch.bfloat16)
    assert np.array_equal(img, _bf16_bits_of(pc.w))


@pytest.mark.parametrize('rows,K', [(64, 64), (128, 64), (256, 576)])
def test_fragment_image_is_the_view_and_permute_of_frag_image(rows, K):
    """The same expression as ops.PackedConv.frag_image, on the bits (the method itself asks for rows % 256 == 0; the image is
    defined for every rows % 64 == 0) -- and the method on a CPU pack where it takes the shape."""
    from pointtinybenchmark_amd import ops
    img = np.arange(rows * K, dtype=np.uint16).reshape(rows, K)
    G, KS = rows // 64, K // 16
    want = _t(img.view(np.int16)).view(G, 32, 2, KS, 2, 8).permute(0, 3, 2, 4, 1, 5).contiguous().numpy().view(np.uint16)
    assert np.array_equal(R.frag_of(img), want)
    assert sorted(R.frag_of(img).reshape(-1)) == sorted(img.reshape(-1))
    if rows % 256 == 0 and K % 64 == 0:
        pc = ops.PackedConv(_t(R.master((rows, 64, 3, 3), 9)), 1, 1, torch.bfloat16)
        assert pc.wfrag is None
        assert np.array_equal(_bf16_bits_of(pc.frag_image()), R.frag_of(_bf16_bits_of(pc.w)))


# ---- each special layout against its consumer ---------------------------------------------------------------------------------------
H = W = 5


def _padded(x):
    """(H, W, C) -> zero border of one pixel."""
    return np.pad(x, ((1, 1), (1, 1), (0, 0)))


def emulate_grouped(x, wp, C, cg):
    """conv_group_fwd_kernel's addressing: thread `quad` reads float4 wr[((tap * CH + ch) * 4 + j) * C4 + quad] and multiplies its
    component e with input channel g0 + 4 ch + e into output channel 4 quad + j.  x (H, W, C) fp64 -> (H, W, C)."""
    C4, CH = C // 4, cg // 4
    wq = wp.astype(np.float64).reshape(-1, 4)              # float4s
    xp, out = _padded(x), np.zeros((H, W, C))
    for quad in range(C4):
        g0 = quad * 4 // cg * cg
        for tap in range(9):
            kh, kw = tap // 3, tap % 3
            for ch in range(CH):
                v = xp[kh:kh + H, kw:kw + W, g0 + 4 * ch:g0 + 4 * ch + 4]
                for j in range(4):
                    out[:, :, 4 * quad + j] += v @ wq[((tap * CH + ch) * 4 + j) * C4 + quad]
    return out


def emulate_res2(x, wp, width):
    """res2_conv_kernel: thread `pair` reads float2 wq[tap * w2 * 2 * w2 + (2 kp + j) * w2 + pair], component e against input channel
    2 kp + e, into output channel 2 pair + j."""
    w2 = width // 2
    wq = wp.astype(np.float64).reshape(-1, 2)
    xp, out = _padded(x), np.zeros((H, W, width))
    for pair in range(w2):
        for tap in range(9):
            kh, kw = tap // 3, tap % 3
            for kp in range(w2):
                v = xp[kh:kh + H, kw:kw + W, 2 * kp:2 * kp + 2]
                for j in range(2):
                    out[:, :, 2 * pair + j] += v @ wq[tap * w2 * 2 * w2 + (2 * kp + j) * w2 + pair]
    return out


def emulate_dw(x, wp, C, Cp, flip):
    """dw_fwd_kernel: wt[t] = wp[t * Cp + c .. c + 3], acc += win[t] * wt[t] with win[kh * 3 + kw] = in[o + kh - 1][col + kw - 1]; the
    stride-1 data gradient walks dy the same way against wt[8 - t] (flip)."""
    wt = wp.astype(np.float64).reshape(9, Cp)
    xp, out = _padded(x), np.zeros((H, W, C))
    for t in range(9):
        out += xp[t // 3:t // 3 + H, t % 3:t % 3 + W, :] * wt[8 - t if flip else t, :C]
    return out


def _conv_and_dgrad(w, s, groups, seed):
    """fp64: x, conv2d(x) (no scale), dy, and the autograd input gradient of conv2d(x) * s (s None: of conv2d(x))."""
    g = torch.Generator().manual_seed(seed)
    C = w.shape[0]
    x = torch.randn(1, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(1, C, H, W, generator=g, dtype=torch.float64)
    wt = _t(w).double()
    y = F.conv2d(x, wt, padding=1, groups=groups)
    ys = y if s is None else y * _t(s).double()[None, :, None, None]
    dx, = torch.autograd.grad(ys, x, dy)
    hwc = lambda t: t.detach()[0].permute(1, 2, 0).numpy()
    return hwc(x), hwc(y), hwc(dy), hwc(dx)


def _close(a, b):
    return np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


@pytest.mark.parametrize('C,cg', [g for g in R.GROUPED if g[0] <= 112])
def test_grouped_image_feeds_the_grouped_kernels_addressing(C, cg):
    w, s = R.master((C, cg, 3, 3), 13), R.scale_of(C, 13)
    x, y, dy, _ = _conv_and_dgrad(w, None, C // cg, 14)
    assert _close(emulate_grouped(x, R.grouped(w, None, cg, 0), C, cg), y)
    _, _, _, dx = _conv_and_dgrad(R._scaled(w, s), None, C // cg, 14)      # the pack holds fl32(w * s): the gradient of that very layer
    assert _close(emulate_grouped(dy, R.grouped(w, s, cg, 1), C, cg), dx)
    _, _, _, dx1 = _conv_and_dgrad(w, None, C // cg, 14)
    assert _close(emulate_grouped(dy, R.grouped(w, None, cg, 1), C, cg), dx1)


@pytest.mark.parametrize('width', [v for v in R.RES2 if v <= 26])
def test_res2_image_feeds_the_slice_kernels_addressing(width):
    w, s = R.master((width, width, 3, 3), 15), R.scale_of(width, 15)
    x, y, dy, _ = _conv_and_dgrad(w, None, 1, 16)
    assert _close(emulate_res2(x, R.res2(w, None, 0), width), y)
    _, _, _, dx = _conv_and_dgrad(R._scaled(w, s), None, 1, 16)
    assert _close(emulate_res2(dy, R.res2(w, s, 1), width), dx)
    _, _, _, dx1 = _conv_and_dgrad(w, None, 1, 16)
    assert _close(emulate_res2(dy, R.res2(w, None, 1), width), dx1)


@pytest.mark.parametrize('C', R.DW)
def test_depthwise_image_feeds_the_depthwise_kernels_addressing(C):
    w, s = R.master((C, 1, 3, 3), 17), R.scale_of(C, 17)
    Cp = R.pad32(C)
    x, y, dy, _ = _conv_and_dgrad(w, None, C, 18)
    assert _close(emulate_dw(x, R.dw(w, None, Cp).reshape(-1), C, Cp, False), y)
    _, _, _, dx = _conv_and_dgrad(R._scaled(w, s), None, C, 18)
    assert _close(emulate_dw(dy, R.dw(w, s, Cp).reshape(-1), C, Cp, True), dx)
    assert not R.dw(w, s, Cp)[:, C:].view(np.uint32).any()


def test_dense_image_feeds_an_implicit_gemm_over_the_taps():
    """The dense consumer: out[r] = sum over k = (kh * KW + kw) * colsp + c of row r times the input patch -- forward against F.conv2d,
    the transposed pack (non-square taps, separate flips) over dy against the autograd input gradient."""
    for shape, pad in (((8, 3, 3, 3), (1, 1)), ((6, 5, 2, 3), (1, 2))):
        O, I, KH, KW = shape
        w, s = R.master(shape, 19), R.scale_of(O, 19)
        g = torch.Generator().manual_seed(20)
        x = torch.randn(1, I, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, _t(w).double(), padding=pad)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        dx, = torch.autograd.grad(F.conv2d(x, _t(R._scaled(w, s)).double(), padding=pad), x, dy)      # the pack holds fl32(w * s)

        def gemm(inp, pack, rows, cols, colsp, ph, pw, OH, OW):
            xp = np.pad(inp, ((ph, ph), (pw, pw), (0, 0)))
            out = np.zeros((OH, OW, rows))
            P = pack.astype(np.float64)
            for kh in range(KH):
                for kw in range(KW):
                    k0 = (kh * KW + kw) * colsp
                    out += xp[kh:kh + OH, kw:kw + OW, :] @ P[:, k0:k0 + cols].T
            return out

        hwc = lambda t: t.detach()[0].permute(1, 2, 0).numpy()
        colsp = R.dense_colsp(I)
        fwd = R.dense_f32(w, None, 0, colsp, R.dense_kpad(KH, KW, colsp))
        assert _close(gemm(hwc(x), fwd, O, I, colsp, pad[0], pad[1], y.shape[2], y.shape[3]), hwc(y))
        colsp = R.dense_colsp(O)
        tr = R.dense_f32(w, s, 1, colsp, R.dense_kpad(KH, KW, colsp))
        got = gemm(hwc(dy), tr, I, O, colsp, KH - 1 - pad[0], KW - 1 - pad[1], H, W)
        assert _close(got, hwc(dx))


# ---- bijections ------------------------------------------------------------------------------------------------------------------
def _arange(shape):
    return np.arange(1, 1 + int(np.prod(shape)), dtype=np.float32).reshape(shape)      # exact in fp32 below 2^24, never zero


def _bijective(img, n_master, n_pad):
    v = np.sort(np.asarray(img, dtype=np.float64).reshape(-1))
    return np.array_equal(v[:n_pad], np.zeros(n_pad)) and np.array_equal(v[n_pad:], np.arange(1, n_master + 1))


def test_every_restated_image_is_a_bijection_onto_its_non_pad_slots():
    for c in R.DENSE32:
        if c['shape'][0] * c['shape'][1] > 64 * 96:
            continue
        rows, cols, colsp, Kpad = R.dense32_geometry(c)
        n = int(np.prod(c['shape']))
        assert _bijective(R.dense_f32(_arange(c['shape']), None, c['transpose'], colsp, Kpad), n, rows * Kpad - n), c
    for C, cg in R.GROUPED[:-1]:
        for tr in (0, 1):
            assert _bijective(R.grouped(_arange((C, cg, 3, 3)), None, cg, tr), 9 * cg * C, 0), (C, cg, tr)
    for width in R.RES2[:-1]:
        for tr in (0, 1):
            assert _bijective(R.res2(_arange((width, width, 3, 3)), None, tr), 9 * width * width, 0), (width, tr)
    for C in R.DW:
        assert _bijective(R.dw(_arange((C, 1, 3, 3)), None, R.pad32(C)), 9 * C, 9 * (R.pad32(C) - C)), C
    for c in R.DENSE16:          # bf16 holds integers up to 256 exactly: the permutation alone, on an index image
        rows, cols = R.dense_dims(c['shape'], c['transpose'])
        if rows * cols > 96 * 64:
            continue
        idx = R.dense_taps(_arange(c['shape']), None, c['transpose']).reshape(rows, -1)
        assert _bijective(idx, idx.size, 0), c
        if c['frag']:
            assert _bijective(R.frag_of(idx), idx.size, 0), c


# ---- job rows, structs, launch caps -----------------------------------------------------------------------------------------------
def _struct_fields(text, name):
    """[(name, 'Q' | 'i' | 'f')] of a struct of pointers, ints and floats, in declaration order."""
    body = re.search(r'struct %s \{(.*?)\};' % name, text, re.S).group(1)
    body = re.sub(r'//[^\n]*', '', body)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        m = re.match(r'(const\s+)?(float|int|unsigned short)\s*(.*)', decl, re.S)
        base = m.group(2)
        for item in m.group(3).split(','):
            item = item.strip()
            fields.append((item.lstrip('* '), 'Q' if '*' in item else {'int': 'i', 'float': 'f'}[base]))
    return fields


def _fmt(fields):
    return '<' + ''.join(k for _, k in fields)


def test_job_rows_are_the_structs_of_the_sources():
    from pointtinybenchmark_amd import layers
    pack, group = _src('pack.hip'), _src('conv_group.hip')
    f16, f32_, fg = _struct_fields(pack, 'PackJob'), _struct_fields(pack, 'Pack32Job'), _struct_fields(group, 'GroupPackJob')
    assert (layers.PackJob._ROW16.size, layers.PackJob._ROW32.size, layers.GroupPackJob._ROWG.size) == (64, 64, 48)
    for row, fields in ((layers.PackJob._ROW16, f16), (layers.PackJob._ROW32, f32_), (layers.GroupPackJob._ROWG, fg)):
        assert struct.Struct(_fmt(fields)).size == row.size and struct.calcsize(_fmt(fields)) == struct.calcsize(row.format)
        assert row.unpack(bytes(range(row.size))) == struct.unpack(_fmt(fields), bytes(range(row.size)))
        # natural alignment: the packed little-endian row is the compiler's layout (pointers first, then 4-byte fields)
        assert [k for _, k in fields] == sorted((k for _, k in fields), key=lambda k: k != 'Q')
    w = torch.zeros(5, 6, 7, 8)
    stub32 = types.SimpleNamespace(dtype=torch.float32, Cin=11, Kpad=12 * 32, w=None, wfrag=None)
    stub16 = types.SimpleNamespace(dtype=torch.bfloat16, Cin=11, Kpad=6 * 7 * 8, w=None, wfrag=None)
    j32, j16 = layers.PackJob(w, stub32, 1, None), layers.PackJob(w, stub16, 1, None)
    row, end = j32.row((101, 102, 103, 104), 77)
    got = dict(zip([n for n, _ in f32_], layers.PackJob._ROW32.unpack(row)))
    assert got == dict(w=101, scale=102, out=103, nblocks=j32.nblocks, pad=0, O=5, I=6, KH=7, KW=8, colsp=11, Kpad=384, transpose=1,
                       block0=77) and end == 77 + j32.nblocks
    row, end = j16.row((101, 102, 103, 104), 77)
    got = dict(zip([n for n, _ in f16], layers.PackJob._ROW16.unpack(row)))
    assert got == dict(w=101, scale=102, out=103, frag=104, O=5, I=6, KH=7, KW=8, transpose=1, block0=77, nblocks=j16.nblocks, pad=0) \
        and end == 77 + j16.nblocks
    stubg = types.SimpleNamespace(dtype=torch.float32, C=72, cg=24, w=torch.zeros(9 * 24 * 72), wfrag=None)
    jg = layers.GroupPackJob(torch.zeros(72, 24, 3, 3), stubg, 1, None)
    row, end = jg.row((101, 102, 103), 77)
    got = dict(zip([n for n, _ in fg], layers.GroupPackJob._ROWG.unpack(row)))
    assert got == dict(w=101, scale=102, out=103, C=72, cg=24, transpose=1, block0=77, nblocks=jg.nblocks, pad=0) and end == 77 + jg.nblocks
    # blocks per job: one per 256 threads (fp32: elements; bf16: element pairs), at most 64
    assert j32.nblocks == R.job_blocks(6 * 384) and j16.nblocks == R.job_blocks(6 * (7 * 8 * 5 // 2)) and jg.nblocks == R.job_blocks(9 * 24 * 72)
    for tables, kind in ((R.MULTI32, '32'), (R.MULTI16, '16')):
        for jobs in tables.values():
            for c in jobs:
                if kind == '32':
                    rows, _, colsp, Kpad = R.dense32_geometry(c)
                    stub = types.SimpleNamespace(dtype=torch.float32, Cin=colsp, Kpad=Kpad, w=None, wfrag=None)
                    want = R.job_blocks(R.dense32_threads(c))
                else:
                    stub = types.SimpleNamespace(dtype=torch.bfloat16, w=None, wfrag=None)
                    want = R.job_blocks(R.dense16_threads(c))
                assert layers.PackJob(torch.zeros(c['shape']), stub, c['transpose'], None).nblocks == want, c
    for jobs in R.MULTIG.values():
        for c in jobs:
            stub = types.SimpleNamespace(C=c['C'], cg=c['cg'], w=torch.zeros(9 * c['cg'] * c['C']))
            assert layers.GroupPackJob(torch.zeros(c['C'], c['cg'], 3, 3), stub, c['transpose'], None).nblocks == R.job_blocks(R.grouped_threads(c))


def test_launch_caps_are_the_constants_in_the_sources():
    from pointtinybenchmark_amd import layers
    pack, group, res2net = _src('pack.hip'), _src('conv_group.hip'), _src('res2net.hip')
    m = re.findall(r'cdivll\(total, 256\) < (\d+) \? cdivll\(total, 256\) : (\d+)', pack)
    assert len(m) == 2 and all(int(a) == int(b) == R.DENSE_GRID_CAP for a, b in m)
    for text, cap in ((group, R.GROUP_GRID_CAP), (res2net, R.RES2_GRID_CAP)):
        m = re.findall(r'const int total = 9 \* [^;]+;\s*const int grid = cdiv\(total, 256\) < (\d+) \? cdiv\(total, 256\) : (\d+)', text)
        assert len(m) == 1 and int(m[0][0]) == int(m[0][1]) == cap
    kernels = 'pack_weights_kernel|pack_weights_multi_kernel|pack_weights_bf16_kernel|pack_weights_bf16_multi_kernel|pack_group_kernel|' \
        'pack_group_multi_kernel|res2_pack_kernel|dw_pack_kernel'
    launches = re.findall(r'hipLaunchKernelGGL\((%s), dim3\([^;]*?\), dim3\((\d+)\)' % kernels, pack + group + res2net + _src('mbv2.hip'))
    assert sorted(k for k, _ in launches) == sorted(kernels.split('|')) and all(int(b) == R.BLOCK for _, b in launches)
    src = inspect.getsource(layers.PackJob) + inspect.getsource(layers.GroupPackJob)
    assert re.findall(r'max\(1, min\((\d+), ', src) == [str(R.JOB_BLOCK_CAP)] * 2
    assert 'dim3(cdiv(9 * Cp, 256)), dim3(256)' in _src('mbv2.hip')


def test_block_to_job_is_the_block_range_of_each_job():
    assert list(R.block_to_job([(0, 1), (1, 1)])) == [0, 1]
    assert list(R.block_to_job([(0, 2), (2, 1), (3, 3)])) == [0, 0, 1, 2, 2, 2]
    assert list(R.block_to_job([(0, 64)])) == [0] * 64
    with pytest.raises(AssertionError):
        R.block_to_job([(0, 2), (3, 1)])
    # the kernels' search: the last job whose block0 <= block
    jobs = [(0, 1), (1, 64), (65, 2), (67, 1), (68, 64)]
    b0 = [j[0] for j in jobs]
    for b, want in enumerate(R.block_to_job(jobs)):
        lo, hi = 0, len(jobs) - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            lo, hi = (mid, hi) if b0[mid] <= b else (lo, mid - 1)
        assert lo == want


# ---- coverage --------------------------------------------------------------------------------------------------------------------
def test_the_tables_reach_every_state():
    cov = R.coverage()
    assert set(cov) == set(R.STATES) and len(R.STATES) == len(set(R.STATES))
    empty = [s for s, cases in cov.items() if not cases]
    assert not empty, empty
    # the figures the tables are quoted with
    assert R.dense32_geometry(R.DENSE32[0]) == (64, 3, 4, 224) and R.dense32_geometry(R.DENSE32[5]) == (64, 2, 4, 32)
    assert R.dense32_threads(R.DENSE32[-1]) == 1179648 and R.dense16_threads(R.DENSE16[-1]) == 1179648
    assert 9 * 32 * 1024 == 294912 and 9 * 172 * 172 == 266256 and R.dense32_threads(R._d((64, 64, 3, 3))) == 36864


# ---- wrong restatements fail -------------------------------------------------------------------------------------------------------
def test_wrong_restatements_differ_on_the_tables():
    hit = dict(kw=0, jh=0, scale_r=0, pad32=0, pad_dw=0)
    for c in R.DENSE32 + R.DENSE16:
        if not c['transpose'] or c['shape'][0] * c['shape'][1] > 64 * 256:
            continue
        w, s = _inputs(c)
        right = R.dense_taps(w, s, 1)
        no_kw_flip = R.dense_taps(w[:, :, :, ::-1], s, 1)          # flipping the master's kw first cancels the pack's kw flip
        differs = not np.array_equal(right, no_kw_flip)
        assert differs == (c['shape'][3] > 1), c
        hit['kw'] += differs
    assert hit['kw'] >= 3
    for c in R.DENSE16:
        if c['frag'] and c['shape'][0] <= 256:
            img = R.dense_bf16(*_inputs(c), c['transpose'])
            hit['jh'] += not np.array_equal(R.frag_of(img), R.frag_of(img, swap_jh=True))
    assert hit['jh'] >= 3
    for C, cg in R.GROUPED[:-1]:
        w, s = R.master((C, cg, 3, 3), 21), R.scale_of(C, 21)
        hit['scale_r'] += not np.array_equal(R.grouped(w, s, cg, 1), R.grouped(w, s, cg, 1, scale_by_r=True))
    assert hit['scale_r'] == len(R.GROUPED) - 1
    for c in R.DENSE32:
        if c['shape'][0] > 96:
            continue
        w, s = _inputs(c)
        rows, cols, colsp, Kpad = R.dense32_geometry(c)
        differs = not np.array_equal(_bits(R.dense_f32(w, s, c['transpose'], colsp, Kpad)),
                                     _bits(R.dense_f32(w, s, c['transpose'], colsp, Kpad, pad_bits=0xFFFFFFFF)))
        assert differs == (colsp > cols or Kpad > c['shape'][2] * c['shape'][3] * colsp), c
        hit['pad32'] += differs
    assert hit['pad32'] >= 2
    for C in R.DW:
        w = R.master((C, 1, 3, 3), 22)
        differs = not np.array_equal(_bits(R.dw(w, None, R.pad32(C))), _bits(R.dw(w, None, R.pad32(C), pad_bits=0xFFFFFFFF)))
        assert differs == (C % 32 != 0)
        hit['pad_dw'] += differs
    assert hit['pad_dw'] >= 3


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call returns the invalid-argument code before any launch (no GPU needed; the buffers are host memory no kernel ever sees)."""
    L = _lib()
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data
    # cpr_pack_weights(w, scale, out, O, I, KH, KW, colsp, Kpad, transpose, stream)
    assert L.cpr_pack_weights(p, None, p, 64, 32, 3, 3, 32, 287, 0, None) == ERR_ARG            # Kpad < KH * KW * colsp
    assert L.cpr_pack_weights(p, None, p, 64, 32, 3, 3, 16, 288, 0, None) == ERR_ARG            # colsp < cols
    assert L.cpr_pack_weights(p, None, p, 64, 32, 3, 3, 32, 288, 1, None) == ERR_ARG            # ... of the transposed pack: cols = O
    assert L.cpr_pack_weights(p, None, p, 0, 32, 3, 3, 32, 288, 0, None) == ERR_ARG             # O = 0
    assert L.cpr_pack_weights(None, None, p, 64, 32, 3, 3, 32, 288, 0, None) == ERR_ARG
    assert L.cpr_pack_weights(p, None, None, 64, 32, 3, 3, 32, 288, 0, None) == ERR_ARG
    # cpr_pack_weights_bf16(w, scale, out, frag, O, I, KH, KW, transpose, stream)
    assert L.cpr_pack_weights_bf16(p, None, p, None, 64, 3, 3, 3, 0, None) == ERR_ARG           # odd cols
    assert L.cpr_pack_weights_bf16(p, None, p, None, 3, 64, 3, 3, 1, None) == ERR_ARG           # odd cols of the transposed pack
    assert L.cpr_pack_weights_bf16(p, None, p, p, 32, 64, 1, 1, 0, None) == ERR_ARG             # frag with rows % 64 != 0
    assert L.cpr_pack_weights_bf16(p, None, p, p, 64, 6, 1, 1, 0, None) == ERR_ARG              # frag with K % 16 != 0
    assert L.cpr_pack_weights_bf16(p, None, p, None, 0, 64, 1, 1, 0, None) == ERR_ARG
    # cpr_pack_weights_grouped(w, scale, out, C, cg, transpose, stream)
    assert L.cpr_pack_weights_grouped(p, None, p, 48, 12, 0, None) == ERR_ARG                   # cg = 12
    assert L.cpr_pack_weights_grouped(p, None, p, 40, 16, 0, None) == ERR_ARG                   # C % cg != 0
    assert L.cpr_pack_weights_grouped(p, None, p, 0, 4, 0, None) == ERR_ARG and L.cpr_pack_weights_grouped(p, None, p, 128, 64, 0, None) == ERR_ARG
    # cpr_res2_pack_weights(w, scale, out, width, transpose, stream)
    assert L.cpr_res2_pack_weights(p, None, p, 13, 0, None) == ERR_ARG                          # odd width
    assert L.cpr_res2_pack_weights(p, None, p, 14, 2, None) == ERR_ARG                          # transpose = 2
    assert L.cpr_res2_pack_weights(p, None, p, 0, 0, None) == ERR_ARG and L.cpr_res2_pack_weights(p, None, p, 514, 0, None) == ERR_ARG
    # cpr_dw3x3_pack(w, scale, wp, C, stream)
    assert L.cpr_dw3x3_pack(p, None, p, 12, None) == ERR_ARG and L.cpr_dw3x3_pack(p, None, p, 0, None) == ERR_ARG      # C % 8 != 0
    for entry in ('cpr_pack_weights_multi', 'cpr_pack_weights_bf16_multi', 'cpr_pack_weights_grouped_multi'):
        fn = getattr(L, entry)
        assert fn(p, 0, 4, None) == ERR_ARG and fn(p, 4, 0, None) == ERR_ARG and fn(None, 4, 4, None) == ERR_ARG, entry
