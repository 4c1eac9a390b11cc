"""The case table of tests/test_train_guard_gpu.py and tests/test_train_guard_cpu.py: one ``Row`` for every entry point of the
training section of include/cotr_hip.h that launches a kernel (the CPU test parses the header and fails when the two sets differ;
the pure host entry points - the size queries and the two salt calls - are ``HOST_ONLY``).  DESIGN.md 3h-20.

A row gives the class of its comparison, its cases - the smallest shapes that put something on an edge of the kernel - and
``build(params, mode)``: the call as a list of arguments in the order of the C prototype (the argument kinds and ``place`` of
tests/scratch_guard_cases.py) with ``expect(outs, fill)``.  Every buffer has exactly the size the header or the size query
gives and is placed at the least alignment the header documents: ``'a16'`` where it says 16 bytes, ``'f32'`` where it says 4.

The three classes of comparison (each per element, never a norm of the tensor):
* ``bits``: moves, bit for bit with the float32 restatement (``check_bits``);
* ``sum``: sums of products, run twice - ``mode == 'int'``: integer-valued inputs in [-3, 3], every partial sum an integer below
  2^24 (asserted on the reference's sum of absolute terms) and the result equal to the int64 reference; ``mode == 'rand'``:
  |got - ref| <= (n + 2) 2^-24 sum |terms|, the bound of any summation order (``check_sum``);
* ``yard``: everything with a rsqrt, exp2 or division, held to ``FACTOR`` = 8 times the worst per-element ratio |err| / scale
  of the same formula in torch float32 on the CPU against the float64 restatement (``YARD``, ``check_yard``).
Every element an op must not write holds the fill byte (``check_fill``)."""
import collections
import ctypes
import functools

import numpy as np

from tests import dropout_oracle as do
from tests import train_kernel_oracle as ko
from tests.guard_arena import is_fill
from tests.scratch_guard_cases import NULL, STREAM, Aux, AuxOut, In, Out, Ref, Table, filled

F32 = np.float32
ERR_ARG = -1
A16, F4, A8 = 'a16', 'f32', 'a8'
MODES = {'bits': ('rand',), 'sum': ('int', 'rand'), 'yard': ('rand',)}

# rc: the expected return value; init: {output name: array} written into an in/out buffer before the call; knobs: process-wide knobs
# for the call; twin: (entry point, TCall) whose outputs ``expect`` receives as a third argument; yard(): the yardstick's own ratios
TCall = collections.namedtuple('TCall', 'args expect rc init knobs twin yard', defaults=(0, None, None, None, None))
Case = collections.namedtuple('Case', 'id params')
# query: the size query of part / scratch, or None; early: (case id, buffer) of the early-band control, or None
Row = collections.namedtuple('Row', 'name cls query cases build early')

# ---- the yardstick figures -----------------------------------------------------------------------------------------------------
# YARD[key]: the worst per-element ratio |torch float32 on the CPU - float64 restatement| / scale over the cases of the table,
# measured when the table was written (rounded up to two digits) and reproduced by tests/test_train_guard_cpu.py.  A kernel is allowed
# FACTOR times that: exp2 in the log2 domain, rcp and another summation order - not a wrong term.
# KERNEL_WORST[key]: the kernels' own worst ratio in the first run on an MI355X, for the record.
FACTOR = 8.0
YARD = {
    'ln_fwd.y': 1.9e-7, 'ln_fwd.mean': 6.5e-9, 'ln_fwd.rstd': 1.1e-7,
    'ln_bwd.ds': 1.6e-7, 'ln_bwd.dgamma': 1.2e-7,
    'head_fwd.y': 1.9e-7,
    'adam.p': 9.6e-5, 'adam.m': 5.7e-8, 'adam.v': 1.1e-7,
    'attention_fwd.o': 4.4e-7, 'attention_fwd.lse': 1.4e-7,
    'attention_bwd.delta': 1.1e-7, 'attention_bwd.dq': 1.4e-7, 'attention_bwd.dk': 3.6e-7, 'attention_bwd.dv': 1.3e-6,
}
KERNEL_WORST = {
    'ln_fwd.y': 1.71e-7, 'ln_fwd.mean': 3.14e-9, 'ln_fwd.rstd': 6.92e-8,
    'ln_bwd.ds': 1.09e-7, 'ln_bwd.dgamma': 1.19e-7,
    'head_fwd.y': 5.17e-8,
    'adam.p': 9.58e-5, 'adam.m': 5.18e-8, 'adam.v': 1.01e-7,
    'attention_fwd.o': 4.74e-7, 'attention_fwd.lse': 1.12e-7,
    'attention_bwd.delta': 8.43e-8, 'attention_bwd.dq': 1.48e-7, 'attention_bwd.dk': 5.11e-7, 'attention_bwd.dv': 1.17e-6,
}
WORST = {}                                             # filled by check_yard while a test session runs


def bound(key):
    return FACTOR * YARD[key]


# ---- the comparison functions --------------------------------------------------------------------------------------------------
def _first(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def check_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want, dtype=got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} elements differ in their bits, first at {_first(bad)}: got {got[_first(bad)]!r}, want {want[_first(bad)]!r}'


def check_sum(got, ref, sumabs, n, mode, what):
    """n: the largest number of terms of one element"""
    got, ref, sumabs = np.asarray(got), np.asarray(ref, dtype=np.float64), np.asarray(sumabs, dtype=np.float64)
    assert got.shape == ref.shape == sumabs.shape, (what, got.shape, ref.shape)
    if mode == 'int':
        assert sumabs.max(initial=0) < 2 ** 24 and np.array_equal(ref, np.rint(ref)), what     # a condition, not a hope
        bad = got.astype(np.float64) != ref
        assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} integer sums are wrong, first at {_first(bad)}: got {got[_first(bad)]!r}, want {ref[_first(bad)]!r}'
    else:
        err = np.abs(got.astype(np.float64) - ref)
        bad = ~(err <= (n + 2) * 2.0 ** -24 * sumabs)
        assert not bad.any(), (f'{what}: {int(bad.sum())} of {bad.size} elements are outside (n + 2) 2^-24 sum|terms| with n = {n}, first at {_first(bad)}: '
                               f'got {got[_first(bad)]!r}, want {ref[_first(bad)]!r}, sum|terms| {sumabs[_first(bad)]!r}')


def yard_ratio(got, ref, scale):
    """the worst per-element |got - ref| / scale (NaN or inf in got: inf)"""
    r = np.abs(np.asarray(got, dtype=np.float64) - ref) / scale
    r = np.where(np.isfinite(r), r, np.inf)
    return float(r.max(initial=0.0)), r


def check_yard(got, ref, scale, key, what):
    assert np.asarray(got).shape == np.asarray(ref).shape, (what, np.asarray(got).shape, np.asarray(ref).shape)
    worst, r = yard_ratio(got, ref, scale)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    bad = r > bound(key)
    assert not bad.any(), (f'{what}: {int(bad.sum())} of {bad.size} elements are more than {FACTOR:g} x the yardstick {YARD[key]:.3g} off ({key}), worst ratio '
                           f'{worst:.3g} at {_first(r == r.max())}, first at {_first(bad)}: got {np.asarray(got)[_first(bad)]!r}, want {np.asarray(ref)[_first(bad)]!r}')


def check_fill(a, fill, what):
    assert filled(a, fill), f'{what}: {int((~is_fill(a, fill)).sum())} elements that must not be written are not the fill 0x{fill:02X}'


def untouched(outs, fill, *_):
    for name, a in outs.items():
        check_fill(a, fill, name)


# ---- data ----------------------------------------------------------------------------------------------------------------------
def data(mode, seed, *shape):
    rng = np.random.default_rng(seed)
    if mode == 'int':
        return rng.integers(-3, 4, shape).astype(F32)
    return rng.standard_normal(shape).astype(F32)


def opt(present, arg):
    return arg if present else NULL


# ---- cotr_train_add_rowmod: 4 rows a workgroup ----------------------------------------------------------------------------------
def add_rowmod_build(params, mode):
    rows, mod = params
    x, x2 = data(mode, 1, rows, 256), data(mode, 2, mod if mod else rows, 256)

    def expect(outs, fill):
        check_bits(outs['y'], ko.add_rowmod(x, x2, mod), 'y')
    return TCall([In('x', x, A16), In('x2', x2, A16), mod, Out('y', F32, (rows, 256), A16), rows, STREAM], expect)


ADD_ROWMOD = Row('cotr_train_add_rowmod', 'bits', None,
                 [Case('rows1-mod0', (1, 0)), Case('rows3-mod2', (3, 2)), Case('rows4-mod3', (4, 3)), Case('rows5-mod0', (5, 0)), Case('rows5-mod3', (5, 3))],
                 add_rowmod_build, None)


# ---- cotr_train_add_drop_ln_fwd: 4 rows a workgroup, a wavefront a row ------------------------------------------------------------
def _ln_inputs(rows, with_x, p, seed):
    a, x = data('rand', 3 + rows, rows, 256), (data('rand', 4 + rows, rows, 256) if with_x else None)
    w, b = (1 + 0.3 * data('rand', 5, 256)).astype(F32), (0.2 * data('rand', 6, 256)).astype(F32)
    return a, x, w, b, ko.ln_s(x, a, p, seed)


def ln_fwd_build(params, mode):
    rows, with_x, with_s, p = params
    seed = 0x1234ABCD + rows
    a, x, w, b, s = _ln_inputs(rows, with_x, p, seed)
    (y, ys), (mean, ms), (rstd, rs) = ko.ln_fwd(s, w, b)

    def expect(outs, fill):
        if with_s:
            check_bits(outs['s_out'], s, 's_out: x + dropout(a), the zeros and the kept elements of the mask')
            assert p == 0 or (s == (x if with_x else 0)).any(), 'no element was dropped'
        check_yard(outs['y'], y, ys, 'ln_fwd.y', 'y')
        check_yard(outs['stats'][:, 0], mean, ms, 'ln_fwd.mean', 'stats mean')
        check_yard(outs['stats'][:, 1], rstd, rs, 'ln_fwd.rstd', 'stats rstd')

    def yard():
        y32, m32, r32 = ko.ln_fwd_f32(s, w, b)
        return {'ln_fwd.y': yard_ratio(y32, y, ys)[0], 'ln_fwd.mean': yard_ratio(m32, mean, ms)[0], 'ln_fwd.rstd': yard_ratio(r32, rstd, rs)[0]}
    return TCall([In('x', x, A16) if with_x else NULL, In('a', a, A16), In('w', w, A16), In('b', b, A16), opt(with_s, Out('s_out', F32, (rows, 256), A16)),
                  Out('y', F32, (rows, 256), A16), Out('stats', F32, (rows, 2), F4), rows, ctypes.c_float(p), seed, STREAM], expect, yard=yard)


LN_FWD = Row('cotr_train_add_drop_ln_fwd', 'yard', None,
             [Case('rows1-x-s-p0.1', (1, True, True, 0.1)), Case('rows3-noX-s-p0', (3, False, True, 0.0)), Case('rows4-x-noS-p0.1', (4, True, False, 0.1)),
              Case('rows5-x-s-p0.1', (5, True, True, 0.1)), Case('rows5-noX-noS-p0', (5, False, False, 0.0)), Case('rows4-noX-s-p0.1', (4, False, True, 0.1))],
             ln_fwd_build, None)


# ---- cotr_train_ln_bwd: rows a workgroup a multiple of 4, at most 512 parts -------------------------------------------------------
def ln_bwd_build(params, mode):
    rows, with_da, p, with_dwb = params
    seed = 0x0BADF00D + rows
    dy = data(mode, 7 + rows, rows, 256)
    _, _, w, b, s = _ln_inputs(rows, True, 0.0, 0)
    (_, _), (mean, _), (rstd, _) = ko.ln_fwd(s, w, b)
    stats = np.stack([mean, rstd], 1).astype(F32)
    ref = ko.ln_bwd(dy, s, stats, w)
    parts = ko.ln_bwd_parts(rows)
    per = ko.ln_bwd_per(rows)

    def expect(outs, fill):
        part = outs['part']
        check_sum(part[:, 256:], *ref['beta_part'], per, mode, 'part: dbeta of every workgroup')
        if with_dwb:
            check_sum(outs['dwb'][256:], *ref['beta'], rows, mode, 'dwb: dbeta')
        if mode == 'int':
            return
        check_sum(part[:, :256], *ref['gamma_part'], 2 * per, mode, 'part: dgamma of every workgroup')      # (a product and its xhat: two roundings a term)
        check_yard(outs['ds'], *ref['ds'], 'ln_bwd.ds', 'ds')
        if with_dwb:
            check_yard(outs['dwb'][:256], ref['gamma'][0], np.maximum(ref['gamma'][1], np.finfo(F32).tiny), 'ln_bwd.dgamma', 'dwb: dgamma')
        if with_da:                                             # a move of the kernel's own ds: its mask's zeros, the kept elements one multiply
            keep = do.flat_mask(seed, rows, 256, p)
            check_bits(outs['da'], ko.dropped(outs['ds'], keep, p), 'da = ds * mask / (1 - p)')
            assert p == 0 or not keep.all()

    def yard():
        ds32, g32 = ko.ln_bwd_f32(dy, s, stats, w)
        return {'ln_bwd.ds': yard_ratio(ds32, *ref['ds'])[0], 'ln_bwd.dgamma': yard_ratio(g32, ref['gamma'][0], np.maximum(ref['gamma'][1], np.finfo(F32).tiny))[0]}
    return TCall([In('dy', dy, A16), In('s_in', s, A16), In('stats', stats, F4), In('w', w, A16), Out('ds', F32, (rows, 256), A16),
                  opt(with_da, Out('da', F32, (rows, 256), A16)), Out('part', F32, (parts, 512), F4), opt(with_dwb, Out('dwb', F32, (512,), F4)),
                  rows, ctypes.c_float(p), seed, STREAM], expect, yard=yard if mode == 'rand' else None)


LN_BWD = Row('cotr_train_ln_bwd', 'sum', 'cotr_train_ln_bwd_parts',
             [Case('rows1-da-p0.1-dwb', (1, True, 0.1, True)), Case('rows4-noDa-p0-dwb', (4, False, 0.0, True)), Case('rows5-da-p0-noDwb', (5, True, 0.0, False)),
              Case('rows2047-da-p0.1-noDwb', (2047, True, 0.1, False)), Case('rows2048-noDa-p0-dwb', (2048, False, 0.0, True)),
              Case('rows2049-da-p0.1-dwb', (2049, True, 0.1, True))],
             ln_bwd_build, ('rows2048-noDa-p0-dwb', 'part'))


# ---- cotr_train_head_fwd / cotr_train_head_bwd: a wavefront a row, a part is 514 floats ------------------------------------------
HEAD_ROWS = [(1, 1), (1, 3), (1, 255), (2, 128), (1, 257), (5, 205)]          # rows 1, 3, 255, 256, 257, 1025


def head_fwd_build(params, mode):
    nb, nq = params
    rows = nb * nq
    x, w, b = data(mode, 11 + rows, rows, 256), data(mode, 12, 512), data(mode, 13, 2)
    y, ys = ko.head_fwd(x, w, b)

    def expect(outs, fill):
        check_yard(outs['y'].reshape(rows, 2), y, ys, 'head_fwd.y', 'y')
    return TCall([In('x', x, A16), In('w', w, A16), In('b', b, F4), Out('y', F32, (nb, nq, 2), F4), nb, nq, STREAM], expect,
                 yard=lambda: {'head_fwd.y': yard_ratio(ko.head_fwd_f32(x, w, b), y, ys)[0]})


HEAD_FWD = Row('cotr_train_head_fwd', 'yard', None, [Case(f'rows{nb * nq}', (nb, nq)) for nb, nq in HEAD_ROWS], head_fwd_build, None)


def head_bwd_build(params, mode):
    rows, with_dwb = params
    dy, h, w2 = data(mode, 14 + rows, rows, 2), data(mode, 15 + rows, rows, 256), data(mode, 16, 512)
    parts, per = ko.head_bwd_parts(rows), ko.head_bwd_per(rows)
    dh, part, dwb = ko.head_bwd(dy, h, w2)

    def expect(outs, fill):
        check_sum(outs['dh'], *dh, 2, mode, 'dh')
        check_sum(outs['part'], *part, per, mode, 'part')
        if with_dwb:
            check_sum(outs['dwb'], *dwb, rows, mode, 'dwb')
    return TCall([In('dy', dy, F4), In('h', h, A16), In('w2', w2, A16), Out('dh', F32, (rows, 256), A16), Out('part', F32, (parts, 514), F4),
                  opt(with_dwb, Out('dwb', F32, (514,), F4)), rows, STREAM], expect)


HEAD_BWD = Row('cotr_train_head_bwd', 'sum', 'cotr_train_head_bwd_parts',
               [Case(f'rows{nb * nq}-{"dwb" if i % 2 == 0 else "noDwb"}', (nb * nq, i % 2 == 0)) for i, (nb, nq) in enumerate(HEAD_ROWS)] +
               [Case('rows1025-dwb', (1025, True)), Case('rows256-dwb', (256, True))],
               head_bwd_build, ('rows256-dwb', 'part'))


# ---- cotr_train_dropout_fwd / cotr_train_relu_drop_bwd: 1024 elements a workgroup -------------------------------------------------
def dropout_fwd_build(params, mode):
    n, p = params
    seed = 0x5EED0000 + n
    x = data(mode, 17 + n, n)

    def expect(outs, fill):
        want = ko.dropout_fwd(x, p, seed)
        check_bits(outs['x'], want, 'x *= mask / (1 - p)')
        assert p == 0 or n < 64 or ((want == 0).any() and (want != 0).any())
    return TCall([Out('x', F32, (n,), A16), n, ctypes.c_float(p), seed, STREAM], expect, init={'x': x})


DROPOUT_FWD = Row('cotr_train_dropout_fwd', 'bits', None,
                  [Case(f'n{n}-p{p}', (n, p)) for n, p in ((4, 0.1), (1020, 0.1), (1024, 0.1), (1028, 0.1), (1028, 0.0), (1024, 0.5))], dropout_fwd_build, None)


def relu_drop_bwd_build(params, mode):
    n, p = params
    dy = data(mode, 18 + n, n)
    y = np.maximum(data(mode, 19 + n, n), 0).astype(F32)
    y[::7] = -0.0

    def expect(outs, fill):
        check_bits(outs['dx'], ko.relu_drop_bwd(dy, y, p), 'dx = y > 0 ? dy / (1 - p) : 0')
    return TCall([In('dy', dy, A16), In('y', y, A16), Out('dx', F32, (n,), A16), n, ctypes.c_float(p), STREAM], expect)


RELU_DROP_BWD = Row('cotr_train_relu_drop_bwd', 'bits', None,
                    [Case(f'n{n}-p{p}', (n, p)) for n, p in ((4, 0.1), (1020, 0.0), (1024, 0.1), (1028, 0.1), (1028, 0.0), (1020, 0.1))], relu_drop_bwd_build, None)


# ---- cotr_train_colsum / cotr_train_sum_parts ------------------------------------------------------------------------------------
def colsum_build(params, mode):
    M, N = params
    x = data(mode, 20 + M + N, M, N)
    parts = ko.colsum_parts(M)
    out, part = ko.colsum(x)

    def expect(outs, fill):
        check_sum(outs['part'], *part, ko.colsum_per(M), mode, 'part')
        check_sum(outs['out'], *out, M, mode, 'out')
    return TCall([In('x', x, A16), Out('part', F32, (parts, N), A16), Out('out', F32, (N,), F4), M, N, STREAM], expect)


COLSUM = Row('cotr_train_colsum', 'sum', 'cotr_train_colsum_parts',
             [Case(f'M{M}-N{N}', (M, N)) for M, N in ((1, 4), (255, 1020), (256, 1024), (257, 1028), (513, 4096), (513, 4), (1, 4096), (257, 1024))],
             colsum_build, ('M256-N1024', 'part'))


def sum_parts_build(params, mode):
    nparts, n = params
    part = data(mode, 21 + nparts + n, nparts, n)

    def expect(outs, fill):
        check_sum(outs['out'], *ko.sum_parts(part), nparts, mode, 'out')
    return TCall([In('part', part, F4), nparts, n, Out('out', F32, (n,), F4), STREAM], expect)


SUM_PARTS = Row('cotr_train_sum_parts', 'sum', None,
                [Case(f'parts{p}-n{n}', (p, n)) for p, n in ((1, 1), (7, 255), (8, 256), (9, 257), (9, 1), (1, 257), (8, 255), (7, 256))], sum_parts_build, None)


# ---- cotr_train_transpose / _batched / cotr_train_perm_jobs: 32 x 32 tiles -------------------------------------------------------
def transpose_build(params, mode):
    R, C = params
    src = data(mode, 22 + 40 * R + C, R, C)

    def expect(outs, fill):
        check_bits(outs['dst'], ko.transpose(src), 'dst')
    return TCall([In('src', src, F4), Out('dst', F32, (C, R), F4), R, C, STREAM], expect)


TRANSPOSE = Row('cotr_train_transpose', 'bits', None,
                [Case(f'{R}x{C}', (R, C)) for R, C in ((1, 1), (31, 33), (32, 32), (33, 31), (1, 33), (33, 1), (32, 31), (33, 33))], transpose_build, None)


def transpose_batched_build(params, mode):
    Z, R, C = params
    src = data(mode, 23 + 40 * R + C + Z, Z, R, C)

    def expect(outs, fill):
        check_bits(outs['dst'], ko.transpose(src), 'dst')
    return TCall([In('src', src, F4), Out('dst', F32, (Z, C, R), F4), Z, R, C, STREAM], expect)


TRANSPOSE_BATCHED = Row('cotr_train_transpose_batched', 'bits', None,
                        [Case(f'{Z}x{R}x{C}', (Z, R, C)) for Z, R, C in ((1, 31, 33), (3, 32, 32), (3, 33, 1), (3, 1, 33), (1, 33, 32), (3, 33, 31))],
                        transpose_batched_build, None)

PERM_JOB = np.dtype([('src', np.uint64), ('dst', np.uint64), ('scale', np.uint64), ('Z', np.uint32), ('R', np.uint32), ('C', np.uint32),
                     ('sz', np.uint32), ('sr', np.uint32), ('sc', np.uint32), ('dz', np.uint32), ('dc', np.uint32),
                     ('tile0', np.uint32), ('tiles_r', np.uint32), ('tiles_c', np.uint32), ('pad', np.uint32)])
PERM_LD, PERM_OFF = 40, 3                       # job A writes [Z][C] rows of R = 33 into rows of 40, from element 3 of a larger buffer


def perm_jobs_build(params, mode):
    with_scale, reverse = params
    ZA, RA, CA = 2, 33, 31                      # job A: contiguous source, tiles 2 x 1 x 2 batches; destination a sub-block
    ZB, RB, CB = 1, 32, 64                      # job B: the source stored [C][R] (sr = 1, sc = R), tiles 1 x 2; destination contiguous
    src_a, src_b, scale = data(mode, 24, ZA * RA * CA), data(mode, 25, CB * RB), data(mode, 26, RA)
    big = PERM_OFF + ZA * CA * PERM_LD + 5

    def make(addr):
        j = np.zeros(2, PERM_JOB)
        j[0] = (addr('src_a'), addr('dst_a') + 4 * PERM_OFF, addr('scale') if with_scale else 0, ZA, RA, CA, RA * CA, CA, 1, CA * PERM_LD, PERM_LD, 0, 2, 1, 1 if reverse else 0)
        j[1] = (addr('src_b'), addr('dst_b'), 0, ZB, RB, CB, 0, 1, RB, 0, RB, 4, 1, 2, 0)
        return j

    def expect(outs, fill):
        a = outs['dst_a']
        block = a[PERM_OFF:PERM_OFF + ZA * CA * PERM_LD].reshape(ZA, CA, PERM_LD)
        check_bits(block[:, :, :RA], ko.perm_job(src_a, ZA, RA, CA, RA * CA, CA, 1, scale if with_scale else None, reverse), 'job A')
        check_fill(block[:, :, RA:], fill, 'job A: the columns between R and the row stride')
        check_fill(a[:PERM_OFF], fill, 'job A: before the sub-block')
        check_fill(a[PERM_OFF + ZA * CA * PERM_LD:], fill, 'job A: after the sub-block')
        check_bits(outs['dst_b'].reshape(ZB, CB, RB), ko.perm_job(src_b, ZB, RB, CB, 0, 1, RB, None, False), 'job B')
    return TCall([Table('jobs', PERM_JOB, (2,), make, A8), In('tile_job', np.array([0, 0, 0, 0, 1, 1], np.uint32), F4), 2, 6, STREAM,
                  Aux('src_a', src_a, F4), Aux('src_b', src_b, F4), Aux('scale', scale, F4), AuxOut('dst_a', F32, (big,), F4),
                  AuxOut('dst_b', F32, (ZB * CB * RB,), F4)], expect)


PERM_JOBS = Row('cotr_train_perm_jobs', 'bits', None,
                [Case('plain', (False, False)), Case('scale', (True, False)), Case('reverse', (False, True)), Case('scale-reverse', (True, True))],
                perm_jobs_build, None)


# ---- cotr_train_scale_rows ---------------------------------------------------------------------------------------------------
def scale_rows_build(params, mode):
    rows, cols, in_place = params
    w, scale = data(mode, 27 + rows + cols, rows, cols), data(mode, 28 + rows, rows)

    def expect(outs, fill):
        check_bits(outs['out'], ko.scale_rows(w, scale), 'out')
    if in_place:
        return TCall([Ref('out'), In('scale', scale, F4), Out('out', F32, (rows, cols), A16), rows, cols, STREAM], expect, init={'out': w})
    return TCall([In('w', w, A16), In('scale', scale, F4), Out('out', F32, (rows, cols), A16), rows, cols, STREAM], expect)


SCALE_ROWS = Row('cotr_train_scale_rows', 'bits', None,
                 [Case(f'{r}x{c}{"-inplace" if ip else ""}', (r, c, ip)) for r, c, ip in ((1, 4, False), (65, 36, False), (65, 4, True), (1, 36, True), (65, 36, True))],
                 scale_rows_build, None)


# ---- cotr_train_im2col / cotr_train_col2im: side-by-side halves -------------------------------------------------------------------
CONV_SHAPES = [(1, 1, 1, 4, 1, 1), (1, 1, 1, 4, 3, 1), (2, 2, 3, 8, 3, 1), (1, 2, 3, 4, 3, 2), (2, 5, 4, 4, 3, 2), (1, 5, 4, 8, 1, 2), (1, 5, 4, 8, 3, 1),
               (2, 2, 3, 4, 1, 1), (1, 1, 1, 8, 3, 2)]            # B, Hin, Win, Cin, ksize, stride


def _conv_id(p):
    return 'B{}-{}x{}-c{}-k{}-s{}'.format(*p)


def im2col_build(params, mode):
    B, Hin, Win, Cin, k, s = params
    x = data(mode, 29 + sum(params), B, Hin, 2 * Win, Cin)
    x[x == 0] = 1.0                                              # a zero in the output is then a pad, not a pixel
    idx, Hout, Wout = ko.im2col_index(*params)
    M = B * Hout * 2 * Wout

    def expect(outs, fill):
        col = outs['col']
        check_bits(col, ko.im2col(x, *params), 'col')
        if k == 3:           # the seam: the last column of the left half under its right-hand taps reads zeros, not the right half's pixels
            c = col.reshape(B, Hout, 2, Wout, k, k, Cin)
            if (Wout - 1) * s - 1 + 2 >= Win:
                assert (c[:, :, 0, Wout - 1, :, 2, :] == 0).all(), 'the left half reads across the seam'
            assert (c[:, :, 1, 0, :, 0, :] == 0).all(), 'the right half reads across the seam'
    return TCall([In('x', x, A16), Out('col', F32, (M, k * k * Cin), A16), B, Hin, Win, Cin, k, s, STREAM], expect)


IM2COL = Row('cotr_train_im2col', 'bits', None, [Case(_conv_id(p), p) for p in CONV_SHAPES], im2col_build, None)


def col2im_build(params, mode):
    B, Hin, Win, Cin, k, s = params
    Hout, Wout = ko.conv_out(Hin, k, s), ko.conv_out(Win, k, s)
    dcol = data(mode, 30 + sum(params), B * Hout * 2 * Wout, k * k * Cin)

    def expect(outs, fill):
        val, sab, n = ko.col2im(dcol, *params)
        check_sum(outs['dx'], val, sab, n, mode, 'dx')
    return TCall([In('dcol', dcol, A16), Out('dx', F32, (B, Hin, 2 * Win, Cin), A16), B, Hin, Win, Cin, k, s, STREAM], expect)


COL2IM = Row('cotr_train_col2im', 'sum', None, [Case(_conv_id(p), p) for p in CONV_SHAPES], col2im_build, None)


# ---- cotr_train_gemm_tn_parts / cotr_train_gemm_tn: 64 x 64 kernel (32 rows a step) and 128 x 128 kernel --------------------------
def _gemm_check_parts(part, A, B, with_colsum, mode, fill):
    M, N = A.shape
    K = B.shape[1]
    ref, sab, per = ko.gemm_tn_parts(A, B, with_colsum)
    nsplit = ref.shape[0]
    check_sum(part[:nsplit], ref, sab, per, mode, 'part')
    check_fill(part[nsplit:], fill, 'part: the partials past the count written')


@functools.lru_cache(maxsize=8)
def _gemm_data(mode, M, N, K):
    return data(mode, 31 + M + N, M, N), data(mode, 32 + M + K, M, K)


def gemm_tn_parts_build(params, mode):
    M, N, K, with_colsum = params
    A, B = _gemm_data(mode, M, N, K)
    splits = ko.gemm_tn_splits(M, N, K)
    width = N * K + (N if with_colsum else 0)

    def expect(outs, fill):
        if M == 0:
            return check_fill(outs['part'], fill, 'part')
        _gemm_check_parts(outs['part'], A, B, with_colsum, mode, fill)
    return TCall([In('A', A, A16), In('B', B, A16), Out('part', F32, (splits, width), F4), M, N, K, with_colsum, STREAM], expect,
                 rc=ko.gemm_tn_plan(M, N, K)[1])


_NK = [(64, 64), (64, 128), (128, 64), (128, 128)]
GEMM_SMALL = [(M, *_NK[i % 4], i % 2) for i, M in enumerate((1, 31, 32, 33, 63, 64, 65, 129, 256))] + [(33, 64, 64, 1), (65, 128, 128, 0), (256, 64, 64, 1)]
GEMM_BIG = [(2048, 512, 256, 1), (2049, 512, 256, 0), (2079, 128, 1024, 1), (2049, 128, 1024, 1), (2048, 128, 1024, 0)]
GEMM_FEWER = (4100, 256, 256, 1)                # 26 partials written of the 32 the query allows


def _gemm_id(p):
    return 'M{}-N{}-K{}-{}'.format(*p[:3], 'colsum' if p[3] else 'plain')


GEMM_TN_PARTS = Row('cotr_train_gemm_tn_parts', 'sum', 'cotr_train_gemm_tn_splits',
                    [Case(_gemm_id(p), p) for p in GEMM_SMALL + GEMM_BIG + [GEMM_FEWER]], gemm_tn_parts_build, ('M256-N64-K64-colsum', 'part'))


def gemm_tn_build(params, mode):
    M, N, K, with_colsum = params
    A, B = _gemm_data(mode, M, N, K)
    splits = ko.gemm_tn_splits(M, N, K)
    width = N * K + (N if with_colsum else 0)

    def expect(outs, fill):
        if M == 0:                                               # zeroes out (and colsum), leaves part alone
            assert not outs['out'].view(np.uint32).any(), 'out is not zeroed'
            return check_fill(outs['part'], fill, 'part')
        check_sum(outs['out'], *ko.gemm_tn(A, B, with_colsum), M, mode, 'out | colsum')
        part = outs['part']                                      # the header's size: a partial is N K + N floats wide with or without colsum
        nsplit = ko.gemm_tn_plan(M, N, K)[1]
        flat = part.reshape(-1)
        _gemm_check_parts(flat[:splits * width].reshape(splits, width), A, B, with_colsum, mode, fill)
        check_fill(flat[splits * width:], fill, 'part: past the partials')
        assert nsplit <= splits
    return TCall([In('A', A, A16), In('B', B, A16), Out('part', F32, (splits, N * K + N), F4), Out('out', F32, (width,), F4),
                  Ref('out', 4 * N * K) if with_colsum else NULL, M, N, K, STREAM], expect)


GEMM_TN = Row('cotr_train_gemm_tn', 'sum', 'cotr_train_gemm_tn_splits',
              [Case(_gemm_id(p), p) for p in [(0, 64, 64, 1), (0, 64, 128, 0), (1, 64, 64, 1), (33, 128, 64, 0), (129, 64, 128, 1), (256, 128, 128, 0),
                                              (2049, 512, 256, 1), (2079, 128, 1024, 0), GEMM_FEWER]], gemm_tn_build, ('M129-N64-K128-colsum', 'part'))


# ---- cotr_train_conv_wgrad_parts: the 128 x 128 kernel gathering its second operand ---------------------------------------------
def conv_wgrad_build(params, mode):
    B, Hin, Win, Cin, Cout, k, s = params
    Hout, Wout = ko.conv_out(Hin, k, s), ko.conv_out(Win, k, s)
    M, N, K = B * Hout * 2 * Wout, Cout, k * k * Cin
    applies = Cin % 128 == 0 and ko.gemm_tn_big(M, N, K)
    dz, x = data(mode, 33 + M, M, Cout), data(mode, 34 + M, B, Hin, 2 * Win, Cin)
    splits = ko.gemm_tn_splits(M, N, K)
    if not applies:
        return TCall([In('dz', dz, A16), In('x', x, A16), Out('part', F32, (splits, N * K), F4), B, Hin, Win, Cin, Cout, k, s, STREAM], untouched, rc=-1)
    col = ko.im2col(x, B, Hin, Win, Cin, k, s)

    def expect(outs, fill, twin):
        _gemm_check_parts(outs['part'], dz, col, 0, mode, fill)
        check_bits(outs['part'], twin['part'], 'part against cotr_train_im2col + cotr_train_gemm_tn_parts')
    twin = ('cotr_train_gemm_tn_parts', TCall([In('A', dz, A16), In('B', col, A16), Out('part', F32, (splits, N * K), F4), M, N, K, 0, STREAM], None,
                                              rc=ko.gemm_tn_plan(M, N, K)[1]))
    return TCall([In('dz', dz, A16), In('x', x, A16), Out('part', F32, (splits, N * K), F4), B, Hin, Win, Cin, Cout, k, s, STREAM], expect,
                 rc=ko.gemm_tn_plan(M, N, K)[1], twin=twin)


CONV_WGRAD = Row('cotr_train_conv_wgrad_parts', 'sum', 'cotr_train_gemm_tn_splits',
                 [Case('32x32-s1', (1, 32, 32, 128, 128, 3, 1)), Case('64x64-s2', (1, 64, 64, 128, 128, 3, 2)), Case('33x32-s1-ragged', (1, 33, 32, 128, 128, 3, 1)),
                  Case('cin64-returns-minus1', (1, 32, 32, 64, 128, 3, 1)), Case('16x16-small-returns-minus1', (1, 16, 16, 128, 128, 3, 1))],
                 conv_wgrad_build, ('32x32-s1', 'part'))


# ---- cotr_train_reduce_jobs / cotr_train_adam: 1024-element chunks, one job per destination ------------------------------------------
REDUCE_SRC = np.dtype([('part', np.uint64), ('pstride', np.uint64), ('nparts', np.uint32), ('pad_', np.uint32)])
REDUCE_JOB = np.dtype([('dst', np.uint64), ('scale', np.uint64), ('numel', np.uint32), ('first_src', np.uint32), ('n_src', np.uint32), ('chunk0', np.uint32),
                       ('row_len', np.uint32), ('cin', np.uint32), ('taps', np.uint32), ('vec', np.uint32)])
# numel, vec, row_len, cin, taps, scale present, nparts of each source
REDUCE_JOBS_SPEC = [(1, 0, 0, 0, 1, False, (3,)), (1023, 0, 33, 0, 1, True, (33,)), (1024, 1, 0, 0, 1, False, (8, 9)), (1025, 0, 0, 0, 1, False, (41,)),
                    (2049, 0, 0, 0, 1, False, (2,)), (2052, 1, 36, 4, 9, True, (40,)), (108, 0, 36, 4, 9, False, (7, 1))]


def reduce_jobs_build(params, mode):
    with_scale, = params
    args, jobs, srcs, chunk_job, checks = [], [], [], [], []
    chunk0 = 0
    for j, (numel, vec, row_len, cin, taps, sc, nps) in enumerate(REDUCE_JOBS_SPEC):
        kind = A16 if vec else F4
        dst0 = data(mode, 40 + j, numel)
        scale = data(mode, 50 + j, numel // row_len) if sc and with_scale else None
        parts = []
        for i, nparts in enumerate(nps):
            pstride = numel + (4 if vec else 1)                  # a stride that is not the count; vec keeps it a multiple of 4
            buf = data(mode, 60 + 10 * j + i, (nparts - 1) * pstride + numel)
            args.append(Aux(f'part{j}_{i}', buf, kind))
            srcs.append((f'part{j}_{i}', pstride, nparts))
            parts.append(np.stack([buf[q * pstride:q * pstride + numel] for q in range(nparts)]))
        args.append(AuxOut(f'dst{j}', F32, (numel,), kind))
        if scale is not None:
            args.append(Aux(f'scale{j}', scale, F4))
        jobs.append((f'dst{j}', f'scale{j}' if scale is not None else None, numel, len(srcs) - len(nps), len(nps), chunk0, row_len, cin, taps, vec))
        nchunk = ko.cdiv(numel, 1024)
        chunk_job += [j] * nchunk
        chunk0 += nchunk
        checks.append((f'dst{j}', dst0, parts, scale, row_len, cin, taps, sum(nps) + 2 * len(nps) + 1))

    def make_jobs(addr):
        t = np.zeros(len(jobs), REDUCE_JOB)
        for i, (d, s, *rest) in enumerate(jobs):
            t[i] = (addr(d), addr(s) if s else 0, *rest)
        return t

    def make_srcs(addr):
        t = np.zeros(len(srcs), REDUCE_SRC)
        for i, (p, stride, n) in enumerate(srcs):
            t[i] = (addr(p), stride, n, 0)
        return t

    def expect(outs, fill):
        for name, dst0, parts, scale, row_len, cin, taps, n in checks:
            check_sum(outs[name], *ko.reduce_job(dst0, parts, scale, row_len, cin, taps), n, mode, name)
    return TCall([Table('jobs', REDUCE_JOB, (len(jobs),), make_jobs, A8), Table('srcs', REDUCE_SRC, (len(srcs),), make_srcs, A8),
                  In('chunk_job', np.array(chunk_job, np.uint32), F4), len(jobs), chunk0, STREAM] + args, expect, init={c[0]: c[1] for c in checks})


REDUCE_JOBS = Row('cotr_train_reduce_jobs', 'sum', None, [Case('scale', (True,)), Case('no-scale', (False,))], reduce_jobs_build, None)

ADAM_JOB = np.dtype([('p', np.uint64), ('off', np.uint64), ('numel', np.uint32), ('chunk0', np.uint32), ('group', np.uint32), ('vec', np.uint32)])
# numel, offset in the flat buffers, vec, lr group: the second job's offset is odd with vec 0; the fourth has a scalar tail under vec 1
ADAM_JOBS_SPEC = [(1, 0, 0, 0), (1023, 1, 0, 1), (1024, 1024, 1, 0), (1025, 2048, 1, 1), (2049, 3075, 0, 0)]
ADAM_TOTAL = 3075 + 2049
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = (1e-4, 1e-5), 0.9, 0.999, 1e-8


def adam_build(params, mode):
    step, = params                                               # None: the corrections as given (t = 3); a float: the device step count
    t = 3.0
    bc1, bc2s = 1.0 - ADAM_B1 ** t, float(np.sqrt(1.0 - ADAM_B2 ** t))
    g = (0.01 * data(mode, 70, ADAM_TOTAL)).astype(F32)
    r = data(mode, 71, ADAM_TOTAL)                               # |m| stays away from 0 and p is small: the update, not the rounding unit of p, sets the scale
    m0, v0 = (0.01 * np.sign(r) * (1 + np.abs(r))).astype(F32), (1e-4 * data(mode, 72, ADAM_TOTAL) ** 2).astype(F32)
    args, jobs, chunk_job, ps = [], [], [], []
    chunk0 = 0
    for j, (numel, off, vec, group) in enumerate(ADAM_JOBS_SPEC):
        p0 = (1e-3 * data(mode, 73 + j, numel)).astype(F32)
        args.append(AuxOut(f'p{j}', F32, (numel,), A16 if vec else F4))
        jobs.append((f'p{j}', off, numel, chunk0, group, vec))
        nchunk = ko.cdiv(numel, 1024)
        chunk_job += [j] * nchunk
        chunk0 += nchunk
        ps.append(p0)

    def make(addr):
        tb = np.zeros(len(jobs), ADAM_JOB)
        for i, (p, *rest) in enumerate(jobs):
            tb[i] = (addr(p), *rest)
        return tb

    def refs():
        for j, (numel, off, vec, group) in enumerate(ADAM_JOBS_SPEC):
            sl = slice(off, off + numel)
            yield j, sl, (ps[j], g[sl], m0[sl], v0[sl], ADAM_LR[group], ADAM_B1, ADAM_B2, ADAM_EPS, bc1, bc2s, step)

    def expect(outs, fill):
        seen = np.zeros(ADAM_TOTAL, bool)
        for j, sl, a in refs():
            pr, mr, vr = ko.adam(*a)
            check_yard(outs[f'p{j}'], *pr, 'adam.p', f'p{j}')
            check_yard(outs['m'][sl], *mr, 'adam.m', f'm of job {j}')
            check_yard(outs['v'][sl], *vr, 'adam.v', f'v of job {j}')
            seen[sl] = True
        check_bits(outs['m'][~seen], m0[~seen], 'm between the jobs')
        check_bits(outs['v'][~seen], v0[~seen], 'v between the jobs')

    def yard():
        out = {'adam.p': 0.0, 'adam.m': 0.0, 'adam.v': 0.0}
        for j, sl, a in refs():
            for key, got, (ref, scale) in zip(('adam.p', 'adam.m', 'adam.v'), ko.adam_f32(*a), ko.adam(*a)):
                out[key] = max(out[key], yard_ratio(got, ref, scale)[0])
        return out
    lr = (ctypes.c_float * 2)(*ADAM_LR)
    return TCall([Table('jobs', ADAM_JOB, (len(jobs),), make, A8), In('chunk_job', np.array(chunk_job, np.uint32), F4), chunk0, In('g', g, A16),
                  Out('m', F32, (ADAM_TOTAL,), A16), Out('v', F32, (ADAM_TOTAL,), A16), lr, 2, ADAM_B1, ADAM_B2, ADAM_EPS, bc1, bc2s,
                  NULL if step is None else In('step', np.array([step], F32), F4), STREAM] + args, expect,
                 init=dict({f'p{j}': p for j, p in enumerate(ps)}, m=m0, v=v0), yard=yard)


ADAM = Row('cotr_train_adam', 'yard', None, [Case('host-corrections', (None,)), Case('device-step3', (3.0,))], adam_build, None)


# ---- cotr_train_attention_fwd / _bwd: 512 keys, 8 heads of 32, 32-query tiles in groups of 4 ------------------------------------
KNOB_FORM = 'train_attention_form'
QSCALE = float(F32(32 ** -0.5))
LDO_WIDE, LDV_WIDE = 320, 288
ATT = ko.ATT_KEYS


@functools.lru_cache(maxsize=4)
def _attn_data(nb, nq, p, packed, wide):
    """q|k (packed: one [nb*512][512] buffer, q in its first nb*nq rows), v, and the float32 forward of the restatement"""
    seed = 0xA77E0000 + 16 * nq + nb
    qk = data('rand', 80 + nq, nb * ATT, 512)
    q, k = (qk[:nb * nq, :256], qk[:, 256:]) if packed else (np.ascontiguousarray(qk[:nb * nq, :256]), np.ascontiguousarray(qk[:, 256:]))
    v = data('rand', 81 + nq, nb * ATT, LDV_WIDE if wide else 256)
    (o, so), (lse, sl) = ko.attention_fwd(q, k, v, nb, nq, QSCALE, p, seed)
    return seed, qk, q, k, v, (o, so), (lse, sl)


def _qk_args(packed, qk, q, k):
    if packed:
        return [In('qk', qk, A16), 512, Ref('qk', 4 * 256), 512]
    return [In('q', q, A16), 256, In('k', k, A16), 256]


def attention_fwd_build(params, mode):
    form, nb, nq, p, packed, wide = params
    seed, qk, q, k, v, (o, so), (lse, sl) = _attn_data(nb, nq, p, packed, wide)
    ldo, ldv = (LDO_WIDE, LDV_WIDE) if wide else (256, 256)

    def expect(outs, fill):
        check_yard(outs['o'][:, :256], o, so, 'attention_fwd.o', 'o')
        check_fill(outs['o'][:, 256:], fill, 'o: the columns between 256 and ldo')
        check_yard(outs['lse'], lse, sl, 'attention_fwd.lse', 'lse')

    def yard():
        o32, l32 = ko.attention_fwd_f32(q, k, v, nb, nq, QSCALE, p, seed)
        return {'attention_fwd.o': yard_ratio(o32, o, so)[0], 'attention_fwd.lse': yard_ratio(l32, lse, sl)[0]}
    return TCall(_qk_args(packed, qk, q, k) + [In('v', v, A16), ldv, Out('o', F32, (nb * nq, ldo), A16), ldo, Out('lse', F32, (nb * nq, 8), F4), nb, nq,
                                              ctypes.c_float(QSCALE), ctypes.c_float(p), seed, STREAM], expect, knobs={KNOB_FORM: form}, yard=yard)


def _attn_id(p):
    return 'form{}-nb{}-nq{}-p{}{}{}'.format(*p[:4], '-packed' if p[4] else '', '-wide' if p[5] else '') + ('-scratch' if len(p) > 6 and p[6] else '')


ATTENTION_FWD = Row('cotr_train_attention_fwd', 'yard', None,
                    [Case(_attn_id(p), p) for p in ((1, 1, 1, 0.1, False, False), (1, 2, 33, 0.0, True, True), (2, 1, 31, 0.1, False, True), (2, 2, 127, 0.1, True, False),
                                                    (3, 1, 128, 0.0, False, False), (0, 1, 129, 0.1, True, True), (2, 1, 32, 0.0, False, False), (1, 1, 129, 0.1, False, False))],
                    attention_fwd_build, None)


def attention_bwd_build(params, mode):
    form, nb, nq, p, packed, wide, with_scratch = params
    seed, qk, q, k, v, (o64, _), (lse64, _) = _attn_data(nb, nq, p, packed, wide)
    ldo, ldv = (LDO_WIDE, LDV_WIDE) if wide else (256, 256)
    o = np.zeros((nb * nq, ldo), F32)
    o[:, :256] = o64
    d_o = data('rand', 82 + nq, nb * nq, ldo)
    lse = lse64.astype(F32)
    ref = ko.attention_bwd(q, k, v, o, d_o, lse, nb, nq, QSCALE, p, seed)
    nscratch = ko.attention_bwd_scratch(nb, nq)

    def expect(outs, fill):
        check_yard(outs['delta'], *ref['delta'], 'attention_bwd.delta', 'delta')
        if packed:
            dqk = outs['dqk']
            dq, dk = dqk[:nb * nq, :256], dqk[:, 256:]
            check_fill(dqk[nb * nq:, :256], fill, 'dq|dk: the rows of dq past nb * nq')
        else:
            dq, dk = outs['dq'], outs['dk']
        check_yard(dq, *ref['dq'], 'attention_bwd.dq', 'dq')
        check_yard(dk, *ref['dk'], 'attention_bwd.dk', 'dk')
        check_yard(outs['dv'][:, :256], *ref['dv'], 'attention_bwd.dv', 'dv')
        check_fill(outs['dv'][:, 256:], fill, 'dv: the columns between 256 and lddv')

    def yard():
        got = ko.attention_bwd_f32(q, k, v, o, d_o, lse, nb, nq, QSCALE, p, seed)
        return {f'attention_bwd.{n}': yard_ratio(got[n], *ref[n])[0] for n in ('delta', 'dq', 'dk', 'dv')}
    grads = ([Out('dqk', F32, (nb * ATT, 512), A16), 512, Ref('dqk', 4 * 256), 512] if packed
             else [Out('dq', F32, (nb * nq, 256), A16), 256, Out('dk', F32, (nb * ATT, 256), A16), 256])
    return TCall(_qk_args(packed, qk, q, k) + [In('v', v, A16), ldv, In('o', o, A16), In('d_o', d_o, A16), ldo, In('lse', lse, F4), Out('delta', F32, (nb * nq, 8), F4)] +
                 grads + [Out('dv', F32, (nb * ATT, ldv), A16), ldv, nb, nq, ctypes.c_float(QSCALE), ctypes.c_float(p), seed,
                          opt(with_scratch, Out('scratch_f', F32, (nscratch,), A16)), STREAM], expect, knobs={KNOB_FORM: form}, yard=yard)


# form 3, nb 1: no scratch -> one workgroup a (pair, head) (4 key tiles a wavefront); scratch -> the keys split over 4 workgroups (1 key tile), all four
# dQ partials = the whole scratch written; form 0, nb 12 with scratch: split over 2 (2 key tiles), half the scratch; form 0, nb 1: the two-kernel form
ATTENTION_BWD = Row('cotr_train_attention_bwd', 'yard', 'cotr_train_attention_bwd_scratch',
                    [Case(_attn_id(p), p) for p in ((1, 1, 1, 0.1, False, False, False), (1, 2, 33, 0.0, True, True, False), (2, 1, 31, 0.1, False, True, False),
                                                    (2, 2, 127, 0.1, True, False, True), (3, 1, 128, 0.0, False, False, False), (3, 1, 129, 0.1, False, False, True),
                                                    (0, 12, 32, 0.1, False, False, True), (0, 1, 129, 0.1, True, True, True), (3, 1, 32, 0.0, False, False, True),
                                                    (3, 2, 127, 0.1, True, False, True))],
                    attention_bwd_build, ('form3-nb1-nq129-p0.1-scratch', 'scratch_f'))


ROWS = [ADD_ROWMOD, LN_FWD, LN_BWD, DROPOUT_FWD, RELU_DROP_BWD, COLSUM, TRANSPOSE, IM2COL, COL2IM, SCALE_ROWS, TRANSPOSE_BATCHED, GEMM_TN, GEMM_TN_PARTS,
        CONV_WGRAD, SUM_PARTS, REDUCE_JOBS, ADAM, PERM_JOBS, HEAD_FWD, HEAD_BWD, ATTENTION_FWD, ATTENTION_BWD]
BY_NAME = {r.name: r for r in ROWS}
HOST_ONLY = ['cotr_train_ln_bwd_parts', 'cotr_train_colsum_parts', 'cotr_train_gemm_tn_splits', 'cotr_train_head_bwd_parts',
             'cotr_train_attention_bwd_scratch', 'cotr_train_set_dropout_salt', 'cotr_train_clear_dropout_salt']


def all_cases():
    return [(r, c, mode) for r in ROWS for c in r.cases for mode in MODES[r.cls]]


# ---- refusals (COTR_ERR_ARG, nothing written) and empty calls (0, nothing written) -----------------------------------------------
def _swap(call, changes, rc):
    """the call with some plain arguments replaced (position -> value): nothing may be written"""
    args = list(call.args)
    for i, v in changes.items():
        args[i] = v
    return call._replace(args=args, expect=untouched, rc=rc, twin=None, init=None, yard=None)


def special_calls():
    """-> [(id, entry point, TCall)]"""
    out = []
    add = lambda ident, row, call: out.append((ident, row.name, call))   # noqa: E731
    g = gemm_tn_parts_build((64, 64, 64, 1), 'rand')
    add('gemm_tn_parts-N-not-64', GEMM_TN_PARTS, _swap(g, {4: 96}, ERR_ARG))
    add('gemm_tn_parts-K-not-64', GEMM_TN_PARTS, _swap(g, {5: 32}, ERR_ARG))
    add('gemm_tn_parts-M0-empty', GEMM_TN_PARTS, _swap(g, {3: 0}, 0))
    t = gemm_tn_build((33, 128, 64, 1), 'rand')
    add('gemm_tn-K-not-64', GEMM_TN, _swap(t, {7: 48}, ERR_ARG))
    add('gemm_tn-colsum-not-out-plus-NK', GEMM_TN, _swap(t, {4: Ref('out', 0)}, ERR_ARG))
    add('dropout_fwd-n-not-4', DROPOUT_FWD, _swap(dropout_fwd_build((1028, 0.1), 'rand'), {1: 1026}, ERR_ARG))
    add('dropout_fwd-n0-empty', DROPOUT_FWD, _swap(dropout_fwd_build((1028, 0.1), 'rand'), {1: 0}, 0))
    add('relu_drop_bwd-n-not-4', RELU_DROP_BWD, _swap(relu_drop_bwd_build((1028, 0.1), 'rand'), {3: 1027}, ERR_ARG))
    add('relu_drop_bwd-n0-empty', RELU_DROP_BWD, _swap(relu_drop_bwd_build((1028, 0.1), 'rand'), {3: 0}, 0))
    add('im2col-Cin-not-4', IM2COL, _swap(im2col_build((1, 2, 3, 4, 3, 2), 'rand'), {5: 2}, ERR_ARG))
    add('col2im-Cin-not-4', COL2IM, _swap(col2im_build((1, 2, 3, 4, 3, 2), 'rand'), {5: 2}, ERR_ARG))
    add('scale_rows-cols-not-4', SCALE_ROWS, _swap(scale_rows_build((65, 36, False), 'rand'), {4: 34}, ERR_ARG))
    af = attention_fwd_build((2, 1, 31, 0.1, False, True), 'rand')
    for pos, what in ((1, 'ldq'), (3, 'ldk'), (5, 'ldv'), (7, 'ldo')):
        add(f'attention_fwd-{what}-not-4', ATTENTION_FWD, _swap(af, {pos: af.args[pos] + 2}, ERR_ARG))
    add('attention_fwd-nb0-empty', ATTENTION_FWD, _swap(af, {9: 0}, 0))
    ab = attention_bwd_build((2, 1, 31, 0.1, False, True, False), 'rand')
    for pos, what in ((1, 'ldq'), (3, 'ldk'), (5, 'ldv'), (8, 'ldo'), (12, 'lddq'), (14, 'lddk'), (16, 'lddv')):
        add(f'attention_bwd-{what}-not-4', ATTENTION_BWD, _swap(ab, {pos: ab.args[pos] + 2}, ERR_ARG))
    add('attention_bwd-nb0-empty', ATTENTION_BWD, _swap(ab, {17: 0}, 0))
    c = colsum_build((257, 1028), 'rand')
    add('colsum-N-not-4', COLSUM, _swap(c, {4: 1026}, ERR_ARG))
    add('colsum-N-above-4096', COLSUM, _swap(colsum_build((1, 4096), 'rand'), {4: 4100}, ERR_ARG))
    add('transpose_batched-batch-above-65535', TRANSPOSE_BATCHED, _swap(transpose_batched_build((3, 1, 33), 'rand'), {2: 65536}, ERR_ARG))
    a = adam_build((None,), 'rand')
    add('adam-ngroups0', ADAM, _swap(a, {7: 0}, ERR_ARG))
    add('adam-ngroups9', ADAM, _swap(a, {7: 9}, ERR_ARG))
    add('adam-lr-null', ADAM, _swap(a, {6: None}, ERR_ARG))
    add('add_rowmod-rows0-empty', ADD_ROWMOD, _swap(add_rowmod_build((5, 3), 'rand'), {4: 0}, 0))
    add('ln_fwd-rows0-empty', LN_FWD, _swap(ln_fwd_build((5, True, True, 0.1), 'rand'), {7: 0}, 0))
    add('ln_bwd-rows0-empty', LN_BWD, _swap(ln_bwd_build((5, True, 0.0, False), 'rand'), {8: 0}, 0))
    add('head_bwd-rows0-empty', HEAD_BWD, _swap(head_bwd_build((3, True), 'rand'), {6: 0}, 0))
    add('head_fwd-nb0-empty', HEAD_FWD, _swap(head_fwd_build((1, 3), 'rand'), {4: 0}, 0))
    add('reduce_jobs-njobs0-empty', REDUCE_JOBS, _swap(reduce_jobs_build((True,), 'rand'), {3: 0}, 0))
    add('perm_jobs-njobs0-empty', PERM_JOBS, _swap(perm_jobs_build((True, False), 'rand'), {2: 0}, 0))
    return out
