"""Exact references of the weight-pack kernels (csrc/pack.hip, conv_group.hip, res2net.hip, mbv2.hip), their case tables and the
coverage conditions of those tables.  numpy only, no device.

A pack is a permutation of the OIHW master, at most one fp32 multiply (the forward conv's folded scale in a data-gradient pack) and at
most one rounding (fp32 -> bf16, to nearest even), so each image has one right answer down to the bit.  Every function here states an
image from the READ side -- which weight the consuming kernel multiplies at the address it loads -- with index arrays, not with the
pack kernels' own decomposition of a flat output index:

  dense      the implicit-GEMM conv reads row r of [rows][Kpad] at k = (kh * KW + kw) * colsp + c as the weight of input channel c at
             tap (kh, kw) of its output channel r.  The data gradient is that conv over dy: its input channels are the layer's output
             channels o, its output channels the layer's input channels i, its taps the layer's taps flipped on both axes, and the
             layer's folded scale[o] rides on the weight.
  fragment   lane (l, h) of cout block j of a k-step feeds one MFMA with img[64 g + 2 l + j][16 ks + 8 h .. + 8].
  grouped    thread `quad` owns output channels 4 quad + j and walks tap -> chunk: float4 ((tap * CH + chunk) * 4 + j) * C4 + quad holds
             the weights of input channels g0 + 4 chunk + e, g0 the first channel of the outputs' group.
  res2       the same with pairs: float2 ((tap * w2 + kp) * 2 + j) * w2 + pair, input channels 2 kp + e, outputs 2 pair + j.
  depthwise  float4 at t * Cp + c: tap t of channels c .. c + 3, zeros behind the real channels.

tests/test_pack_instances_host.py holds these to independent constructions and to emulations of the consumers, without a GPU;
tests/test_gpu_pack_instances.py holds the kernels to them bit for bit."""
import numpy as np

BLOCK = 256
DENSE_GRID_CAP = 4096         # cpr_pack_weights, cpr_pack_weights_bf16
GROUP_GRID_CAP = 1024         # cpr_pack_weights_grouped
RES2_GRID_CAP = 1024          # cpr_res2_pack_weights
JOB_BLOCK_CAP = 64            # blocks of one job of a multi-job launch (layers.PackJob.nblocks)

# fp32 bit patterns at the edges of the bf16 rounding and of an fp32 multiply by one
SUBNORMALS = (0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF)
QNAN = 0x7FC00001
SPECIALS = (0x00000000, 0x80000000,
            0x3F808000, 0x3F818000,                # ties: to the even mantissa below, to the even mantissa above
            0x3F807FFF, 0x3F808001,                # just under and just over a tie
            0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF,    # the largest finite value and the tie under it round to inf; one bit less does not
            0x7F800000, 0xFF800000,
            0x00800000) + SUBNORMALS + (QNAN,)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def bits32(a):
    return f32(a).view(np.uint32)


def from_bits32(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


def is_nan32(b):
    b = np.asarray(b, dtype=np.uint32)
    return ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)


def is_nan16(b):
    b = np.asarray(b, dtype=np.uint16)
    return ((b & 0x7F80) == 0x7F80) & ((b & 0x007F) != 0)


def bf16_bits(x):
    """fp32 -> bf16 bits, to nearest, ties to the even mantissa: (b + 0x7FFF + ((b >> 16) & 1)) >> 16 on the fp32 bits (a carry out of
    the mantissa moves the exponent up, the largest finite values reach inf).  A NaN keeps its sign and becomes quiet."""
    b = bits32(x).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    r = np.where(is_nan32(b.astype(np.uint32)), (b >> 16) | 0x40, r)
    return r.astype(np.uint16)


def _scaled(w, scale):
    """fl32(w[o] * scale[o]): one fp32 multiply per element (numpy keeps subnormals); no scale: the master itself."""
    w = f32(w)
    if scale is None:
        return w
    return f32(w * f32(scale).reshape(-1, 1, 1, 1))


def dense_taps(w, scale, transpose):
    """V[r][kh][kw][c]: the fp32 weight the dense conv multiplies input channel c with at tap (kh, kw) of its output channel r."""
    w = f32(w)
    if not transpose:
        return np.ascontiguousarray(w.transpose(0, 2, 3, 1))
    return np.ascontiguousarray(_scaled(w, scale)[:, :, ::-1, ::-1].transpose(1, 2, 3, 0))


def dense_dims(shape, transpose):
    O, I, KH, KW = shape
    return (I, O) if transpose else (O, I)


def dense_colsp(cols):
    """The padded column count the product asks for: 4 for the stem's 3 channels and for a gradient of <= 4 channels."""
    return 4 if cols <= 4 else cols


def dense_kpad(KH, KW, colsp):
    return (KH * KW * colsp + 31) // 32 * 32


def dense_f32(w, scale, transpose, colsp, Kpad, pad_bits=0):
    """[rows][Kpad] fp32.  pad_bits: what the pad holds (0: the right image; the host test's `pad left unwritten` restatement puts the
    guard pattern there)."""
    V = dense_taps(w, scale, transpose)
    rows, KH, KW, cols = V.shape
    assert colsp >= cols and Kpad >= KH * KW * colsp
    body = np.full((rows, KH, KW, colsp), pad_bits, dtype=np.uint32)
    body[..., :cols] = V.view(np.uint32)
    out = np.full((rows, Kpad), pad_bits, dtype=np.uint32)
    out[:, :KH * KW * colsp] = body.reshape(rows, -1)
    return out.view(np.float32)


def dense_bf16(w, scale, transpose):
    """[rows][K] bf16 bits (uint16), K = KH * KW * cols, no padding."""
    V = dense_taps(w, scale, transpose)
    return bf16_bits(V.reshape(V.shape[0], -1))


def frag_of(img_bits, swap_jh=False):
    """frag[g][ks][j][h][l][e] = img[64 g + 2 l + j][16 ks + 8 h + e].  swap_jh: the wrong image with j and h exchanged in the address
    (the host test shows the tables tell it from the right one)."""
    rows, K = img_bits.shape
    assert rows % 64 == 0 and K % 16 == 0
    g, ks, j, h, l, e = np.ogrid[:rows // 64, :K // 16, :2, :2, :32, :8]
    if swap_jh:
        j, h = h, j
    return np.ascontiguousarray(img_bits[64 * g + 2 * l + j, 16 * ks + 8 * h + e])


def grouped_index(C, cg):
    """(tap, r, g0, k) of every element of P[tap][chunk][j][quad][e], broadcastable to that shape."""
    tap, chunk, j, quad, e = np.ogrid[:9, :cg // 4, :4, :C // 4, :4]
    r = 4 * quad + j
    return tap, r, r // cg * cg, 4 * chunk + e


def grouped(w, scale, cg, transpose, scale_by_r=False):
    """9 * cg * C floats.  scale_by_r: the wrong image that takes the scale of the pack's output channel r instead of the layer's
    output channel g0 + k."""
    w = f32(w)
    C = w.shape[0]
    assert w.shape == (C, cg, 3, 3) and C % cg == 0 and cg % 4 == 0
    tap, r, g0, k = grouped_index(C, cg)
    if not transpose:
        P = w[r, k, tap // 3, tap % 3]
    elif scale_by_r and scale is not None:
        P = f32(w[g0 + k, r - g0, (8 - tap) // 3, (8 - tap) % 3] * f32(scale)[r + 0 * k])
    else:
        P = _scaled(w, scale)[g0 + k, r - g0, (8 - tap) // 3, (8 - tap) % 3]
    return np.ascontiguousarray(np.broadcast_to(P, (9, cg // 4, 4, C // 4, 4))).reshape(-1)


def res2(w, scale, transpose):
    """9 * width * width floats, P[tap][kp][j][pair][e]."""
    w = f32(w)
    width = w.shape[0]
    assert w.shape == (width, width, 3, 3) and width % 2 == 0
    tap, kp, j, pair, e = np.ogrid[:9, :width // 2, :2, :width // 2, :2]
    r, k = 2 * pair + j, 2 * kp + e
    if transpose:
        P = _scaled(w, scale)[k, r, (8 - tap) // 3, (8 - tap) % 3]
    else:
        P = w[r, k, tap // 3, tap % 3]
    return np.ascontiguousarray(P).reshape(-1)


def dw(w, scale, Cp, pad_bits=0):
    """[9][Cp] floats, tap-major, channels [C, Cp) zero."""
    w = f32(w)
    C = w.shape[0]
    assert w.shape == (C, 1, 3, 3) and Cp >= C
    out = np.full((9, Cp), pad_bits, dtype=np.uint32)
    out[:, :C] = np.ascontiguousarray(_scaled(w, scale).reshape(C, 9).T).view(np.uint32)
    return out.view(np.float32)


def pad32(c):
    return (c + 31) // 32 * 32


def job_blocks(threads):
    """Blocks of one job of a multi-job launch: one per 256 threads, at most JOB_BLOCK_CAP (the job grid-strides inside them)."""
    return max(1, min(JOB_BLOCK_CAP, (threads + BLOCK - 1) // BLOCK))


def block_to_job(jobs):
    """jobs: (block0, nblocks) per job, block0 ascending and contiguous -> the job index of every block of the launch."""
    b0 = np.array([j[0] for j in jobs], dtype=np.int64)
    nb = np.array([j[1] for j in jobs], dtype=np.int64)
    assert b0[0] == 0 and np.all(b0[1:] == b0[:-1] + nb[:-1]), 'block ranges must tile the launch'
    blocks = np.arange(int(b0[-1] + nb[-1]))
    return np.searchsorted(b0, blocks, side='right') - 1


# ---- case tables ---------------------------------------------------------------------------------------------------
def _d(shape, transpose=0, scale=False, frag=False, entry='ops'):
    return dict(shape=shape, transpose=transpose, scale=scale, frag=frag, entry=entry)


# dense fp32 (cpr_pack_weights): shape (O, I, KH, KW)
DENSE32 = [
    _d((64, 3, 7, 7)),                       # the stem: colsp 4, Kpad 224, 28 pad floats and a zero fourth channel
    _d((96, 32, 1, 1)),                      # no pad at all
    _d((48, 96, 3, 3)),
    _d((64, 32, 3, 3), 1, True),
    _d((64, 32, 3, 3), 1, False),
    _d((2, 64, 1, 1), 1, True),              # cols_p 4, Kpad 32: 28 pad floats in a 32-float row
    _d((64, 32, 2, 1), 1, True),             # the per-parity sub-kernels of a strided layer: the two flips are separate
    _d((64, 32, 1, 2), 1, True),
    _d((512, 256, 3, 3)),                    # 1,179,648 elements: past the 4096-block grid, a ragged second pass
]
# dense bf16 (cpr_pack_weights_bf16); entry 'c': a shape ops refuses, through the C entry point only
DENSE16 = [
    _d((64, 64, 1, 1), frag=True),                  # one group of 64 rows, four k-steps
    _d((256, 64, 3, 3), frag=True),                 # the shape ops itself asks a fragment image for
    _d((128, 64, 1, 1), frag=True),                 # rows % 64 == 0 but not % 256
    _d((96, 64, 3, 3)),
    _d((64, 256, 3, 3), 1, True, frag=True),        # rows 256
    _d((8, 6, 3, 3), entry='c'),                    # cols even but tiny: a pair of k never straddles a tap
    _d((6, 8, 3, 3), 1, False, entry='c'),
    _d((512, 512, 3, 3), frag=True),                # past the grid cap
]
MODES = [(0, False), (1, False), (1, True)]          # forward, transposed without scale, transposed with scale
GROUPED = [(8, 4), (48, 24), (72, 24), (64, 32), (112, 56), (1024, 32)]      # (C, cg); the last: 294,912 elements, past the cap
RES2 = [2, 6, 14, 26, 172]                                                   # widths; the last: 266,256 elements, past the cap, ragged
DW = [8, 24, 40, 96]                                                         # C; 96 has no pad channels

# multi-job tables: the same dicts, in launch order
MULTI32 = {
    'one': [_d((48, 96, 3, 3))],
    'two_one_block': [_d((4, 32, 1, 1)), _d((2, 8, 1, 1), 1, True)],
    'mixed': [_d((4, 32, 1, 1)), _d((64, 64, 3, 3)), _d((64, 32, 3, 3), 1, True), _d((64, 32, 3, 3), 1, False), _d((64, 3, 7, 7)),
              _d((2, 64, 1, 1), 1, True), _d((64, 32, 1, 2), 1, True)],
}
MULTI16 = {
    'one': [_d((64, 64, 1, 1), frag=True)],
    'two_one_block': [_d((8, 6, 3, 3)), _d((6, 8, 3, 3), 1, True)],
    'mixed': [_d((8, 6, 3, 3)), _d((64, 64, 3, 3), frag=True), _d((128, 64, 1, 1)), _d((64, 256, 3, 3), 1, True, frag=True),
              _d((64, 64, 1, 1), 1, False), _d((96, 64, 3, 3))],
}


def _g(C, cg, transpose=0, scale=False):
    return dict(C=C, cg=cg, transpose=transpose, scale=scale)


MULTIG = {
    'one': [_g(8, 4)],
    'two_one_block': [_g(4, 4), _g(4, 4, 1, True)],
    'mixed': [_g(4, 4), _g(64, 32), _g(72, 24, 1, True), _g(72, 24, 1, False), _g(112, 56), _g(8, 4, 1, True), _g(48, 24)],
}


def dense32_geometry(c):
    rows, cols = dense_dims(c['shape'], c['transpose'])
    KH, KW = c['shape'][2:]
    colsp = dense_colsp(cols)
    return rows, cols, colsp, dense_kpad(KH, KW, colsp)


def dense32_threads(c):
    rows, _, _, Kpad = dense32_geometry(c)
    return rows * Kpad


def dense16_threads(c):
    rows, cols = dense_dims(c['shape'], c['transpose'])
    return rows * (c['shape'][2] * c['shape'][3] * cols // 2)


def grouped_threads(c):
    return 9 * c['cg'] * c['C']


def _passes(threads, blocks):
    return -(-threads // (blocks * BLOCK))


def _ragged(threads, blocks):
    return threads % (blocks * BLOCK) != 0


def _pow2(n):
    return n & (n - 1) == 0


def _multi_states(prefix, tables, threads_of, reached):
    for name, jobs in tables.items():
        nb = [job_blocks(threads_of(j)) for j in jobs]
        if len(jobs) == 1:
            reached[prefix + '.one_job'].append(name)
        if len(jobs) == 2 and nb == [1, 1]:
            reached[prefix + '.two_one_block_jobs'].append(name)
        if len(jobs) >= 5:
            reached[prefix + '.five_or_more_jobs'].append(name)
            if 1 in nb:
                reached[prefix + '.mixed_has_one_block_job'].append(name)
            if any(n == JOB_BLOCK_CAP and _passes(threads_of(j), n) >= 2 and _ragged(threads_of(j), n) for j, n in zip(jobs, nb)):
                reached[prefix + '.mixed_has_capped_job_with_ragged_passes'].append(name)
            if any(a['transpose'] and b['transpose'] and a['scale'] != b['scale'] for a, b in zip(jobs, jobs[1:])):
                reached[prefix + '.mixed_scale_next_to_null_scale'].append(name)
            if any(t % BLOCK for t in map(threads_of, jobs)):
                reached[prefix + '.mixed_has_partial_last_block'].append(name)


STATES = (
    ['dense32.' + s for s in ('stem_pad_and_zero_channel', 'no_pad', 'forward_3x3', 'transposed_with_scale', 'transposed_without_scale',
                              'transposed_cols_p4', 'flip_kh_only', 'flip_kw_only', 'past_grid_cap_ragged')] +
    ['dense16.' + s for s in ('frag_one_group', 'frag_rows_256', 'frag_rows_64_not_256', 'no_frag', 'transposed_scale_frag',
                              'tiny_cols_forward', 'tiny_cols_transposed', 'past_grid_cap_ragged')] +
    ['grouped.' + s for s in ('smallest', 'quads_not_pow2', 'chunks_not_pow2', 'past_grid_cap_ragged', 'several_groups', 'all_modes')] +
    ['res2.' + s for s in ('smallest', 'pairs_not_pow2', 'past_grid_cap_ragged', 'all_modes')] +
    ['dw.' + s for s in ('pad_channels', 'no_pad_channels', 'partial_last_block', 'with_and_without_scale')] +
    [p + '.' + s for p in ('multi32', 'multi16', 'multig')
     for s in ('one_job', 'two_one_block_jobs', 'five_or_more_jobs', 'mixed_has_one_block_job', 'mixed_has_capped_job_with_ragged_passes',
               'mixed_scale_next_to_null_scale', 'mixed_has_partial_last_block')] +
    ['multi32.mixed_has_stem', 'multi16.mixed_frag_next_to_null_frag', 'multig.mixed_shapes_differ']
)


def coverage():
    """state -> the cases of the tables that reach it.  tests/test_pack_instances_host.py asserts none is empty; the GPU test imports
    the same tables, so a case dropped there shows up here."""
    reached = {s: [] for s in STATES}
    for c in DENSE32:
        rows, cols, colsp, Kpad = dense32_geometry(c)
        O, I, KH, KW = c['shape']
        K = KH * KW * colsp
        name = '%s t%d s%d' % (c['shape'], c['transpose'], c['scale'])
        blocks = min(DENSE_GRID_CAP, -(-rows * Kpad // BLOCK))
        if not c['transpose'] and colsp > cols and Kpad > K:
            reached['dense32.stem_pad_and_zero_channel'].append(name)
        if colsp == cols and Kpad == K:
            reached['dense32.no_pad'].append(name)
        if not c['transpose'] and (KH, KW) == (3, 3):
            reached['dense32.forward_3x3'].append(name)
        if c['transpose'] and c['scale'] and (KH, KW) == (3, 3):
            reached['dense32.transposed_with_scale'].append(name)
        if c['transpose'] and not c['scale']:
            reached['dense32.transposed_without_scale'].append(name)
        if c['transpose'] and colsp == 4 and cols < 4 and Kpad - K == 28:
            reached['dense32.transposed_cols_p4'].append(name)
        if c['transpose'] and KH > 1 and KW == 1:
            reached['dense32.flip_kh_only'].append(name)
        if c['transpose'] and KW > 1 and KH == 1:
            reached['dense32.flip_kw_only'].append(name)
        if rows * Kpad > DENSE_GRID_CAP * BLOCK and _ragged(rows * Kpad, blocks):
            reached['dense32.past_grid_cap_ragged'].append(name)
    for c in DENSE16:
        rows, cols = dense_dims(c['shape'], c['transpose'])
        K = c['shape'][2] * c['shape'][3] * cols
        name = '%s t%d s%d f%d' % (c['shape'], c['transpose'], c['scale'], c['frag'])
        th = dense16_threads(c)
        if c['frag']:
            assert rows % 64 == 0 and K % 16 == 0, name
        if c['frag'] and rows == 64 and K == 64:
            reached['dense16.frag_one_group'].append(name)
        if c['frag'] and rows % 256 == 0 and K % 64 == 0 and c['entry'] == 'ops':
            reached['dense16.frag_rows_256'].append(name)
        if c['frag'] and rows % 256 != 0:
            reached['dense16.frag_rows_64_not_256'].append(name)
        if not c['frag'] and cols % 64 == 0:
            reached['dense16.no_frag'].append(name)
        if c['frag'] and c['transpose'] and c['scale']:
            reached['dense16.transposed_scale_frag'].append(name)
        if cols < 16 and not c['transpose']:
            reached['dense16.tiny_cols_forward'].append(name)
        if cols < 16 and c['transpose']:
            reached['dense16.tiny_cols_transposed'].append(name)
        if th > DENSE_GRID_CAP * BLOCK and _ragged(th, DENSE_GRID_CAP):
            reached['dense16.past_grid_cap_ragged'].append(name)
    for C, cg in GROUPED:
        name, th = '(%d,%d)' % (C, cg), 9 * cg * C
        if th == min(9 * g * c for c, g in GROUPED):
            reached['grouped.smallest'].append(name)
        if not _pow2(C // 4):
            reached['grouped.quads_not_pow2'].append(name)
        if not _pow2(cg // 4):
            reached['grouped.chunks_not_pow2'].append(name)
        if th > GROUP_GRID_CAP * BLOCK and _ragged(th, GROUP_GRID_CAP):
            reached['grouped.past_grid_cap_ragged'].append(name)
        if C // cg >= 2:
            reached['grouped.several_groups'].append(name)
    for W in RES2:
        th = 9 * W * W
        if W == 2:
            reached['res2.smallest'].append(str(W))
        if not _pow2(W // 2):
            reached['res2.pairs_not_pow2'].append(str(W))
        if th > RES2_GRID_CAP * BLOCK and _ragged(th, RES2_GRID_CAP):
            reached['res2.past_grid_cap_ragged'].append(str(W))
    if MODES == [(0, False), (1, False), (1, True)]:
        reached['grouped.all_modes'].append('MODES')
        reached['res2.all_modes'].append('MODES')
    for C in DW:
        if pad32(C) > C:
            reached['dw.pad_channels'].append(str(C))
        else:
            reached['dw.no_pad_channels'].append(str(C))
        if 9 * pad32(C) % BLOCK:
            reached['dw.partial_last_block'].append(str(C))
    reached['dw.with_and_without_scale'].append('both, every C')
    _multi_states('multi32', MULTI32, dense32_threads, reached)
    _multi_states('multi16', MULTI16, dense16_threads, reached)
    _multi_states('multig', MULTIG, grouped_threads, reached)
    for name, jobs in MULTI32.items():
        if len(jobs) >= 5 and any(j['shape'] == (64, 3, 7, 7) for j in jobs):
            reached['multi32.mixed_has_stem'].append(name)
    for name, jobs in MULTI16.items():
        if len(jobs) >= 5 and any(a['frag'] != b['frag'] for a, b in zip(jobs, jobs[1:])):
            reached['multi16.mixed_frag_next_to_null_frag'].append(name)
    for name, jobs in MULTIG.items():
        if len(jobs) >= 5 and len({(j['C'], j['cg']) for j in jobs}) >= 3:
            reached['multig.mixed_shapes_differ'].append(name)
    return reached


# ---- seeded inputs (shared by the host and the GPU test) ---------------------------------------------------------------------------
def master(shape, seed):
    """randn * 0.05, fp32."""
    return f32(np.random.default_rng(seed).standard_normal(shape) * 0.05)


def scale_of(n, seed):
    """rand + 0.5, fp32."""
    return f32(np.random.default_rng(seed + 7919).random(n) + 0.5)


def tiled(patterns, shape):
    """The bit patterns repeated over a master of ``shape``."""
    n = int(np.prod(shape))
    p = np.array(patterns, dtype=np.uint32)
    return np.resize(p, n).reshape(shape).view(np.float32)
