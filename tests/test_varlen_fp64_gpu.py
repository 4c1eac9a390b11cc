"""Varlen decode (cotr_forward_varlen / cotr_decode_varlen) against float64, at the tile, pass and form edges of its planner.

Each pattern of PATTERNS is a list of per-pair query counts over pairs of the float64 pool of tests/test_stages_fp64_gpu.py (images
from pool pairs, seeded queries with about 5 % in [-0.5, 1.5]).  test_every_pair_of_a_varlen_call_against_float64 runs it with the
default knobs and checks, for every pair with rows: pred_corrs against the float64 oracle decode of that pair alone (px error <=
max(PX_BAR, 3 x the float32 oracle's px gap)); then, from a second run with debug taps on, query_pos and hs of the LAST pass's rows
(the taps hold one pass; those rows may begin in the middle of a pair) with err <= max(FLOOR[s], 4 * gap32), the bar rule of the
stage test.  Every row of every pattern is checked against float64: rows are independent, so the oracle decodes each pair's own
queries once per module (_oracle).

Every pattern states the passes it is built for - (R, form) per pass, read back from the per-launch profile (passes_of: a pass ends
in its head2 launch, its attention launch names the form, the M of its linear launches is its R) - so a planner change that stops
reaching an edge fails here instead of quietly testing something easier.  The forms are decided by the fill rules on the 256 CUs of
an MI355X.  The batch_split prefix cut depends on those rules too: prefix_pattern() finds it from the handle's own launch list.

Then: poisoned scratch (a caller workspace of exactly the queried size, filled with NaN, and a guard row behind the output); varlen
against the uniform call bit for bit where their launch lists agree; every knob value of tests/knob_cases.py on varlen calls, with
the varlen planner's reach (VL_REACH); the staging ring growing a slot with a copy in flight; and the dispatch coverage of varlen
calls (the ' vl' launch keys) against a seeded grid of count patterns.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from oracle import cotr_oracle as O
from tests import gpu_helpers as G
from tests import raw_abi
from tests.knob_cases import KNOB_CASES, case_runs
from tests.test_parity_gpu import PX_BAR, SHAPE_NOISE_PX, hip_model
from tests.test_stages_fp64_gpu import COVERAGE_Q, FLOOR, POOL, _rel, launch_key, pool
from tests.test_varlen_gpu import FORMS

pytestmark = pytest.mark.gpu

EDGES = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129]   # around 1, 2, 3, 4 32-row tiles = 1, 2 64-row tiles
FUSED, ROWS, PLAIN = 'qproj+attention+oproj dec', 'att_rows dec', 'attention dec'
FORM_OF = {FUSED: 'fused', ROWS: 'rows', PLAIN: 'plain'}
BIG70 = [1900 + (i * 37) % 97 for i in range(70)]

# name: (counts, [(R, form) of each pass] under the default knobs, what it is for)
PATTERNS = {
    # tile edges: every count of EDGES in one call, under each form the default fill rules pick
    'edges_fused': ([97, 1, 64, 129, 31, 96, 33, 128, 63, 0, 32, 127, 65, 95], [(961, 'fused')],
                    'R <= 1024: the fused few-rows attention on 32-row tiles'),
    'edges_plain': (EDGES * 5, [(4805, 'plain')], '4096 < R < 8192: above both fusion thresholds, below att_rows_min_rows'),
    'edges_rows': ([1024, 1, 1024, 31, 1024, 32, 1024, 33, 1024, 63, 1024, 64, 1024, 65, 1024, 95, 1024, 96, 1024, 97, 1024, 127,
                    1024, 128, 129], [(13249, 'rows')],
                   '213 64-row tiles (one round of 256 CUs >= 75 %), 13249 rows >= 7/8 of them: att_rows on 64-row tiles'),
    # empty pairs first, last, adjacent; all but one; fewer rows than pairs (vl_tile_cap's R < B)
    'empty_pairs': ([0, 0, 33, 0, 0, 97, 64, 0, 1, 0, 0], [(195, 'fused')], 'empty pairs first, last and adjacent'),
    'all_but_one_empty': ([0] * 6 + [129] + [0] * 5, [(129, 'fused')], 'one pair with rows among 12'),
    'rows_below_pairs': ([1 if i in (0, 7, 8, 20, 33, 34, 50, 61, 68, 69) else 0 for i in range(70)], [(10, 'fused')],
                         '10 rows over 70 pairs: R < B'),
    # the 32768-row cut falls inside pair 1 (no prefix of whole pairs reaches 8192 rows), the next pass starts there
    'cut_inside_a_pair': ([5000, 30000, 3000, 17], [(32768, 'plain'), (5249, 'plain')],
                          'a pass cut 27768 rows into pair 1 (a partial tile on both sides), pairs 2, 3 behind it'),
    # five passes: four cut by batch_split's prefix rule below 32768 rows (pairs whole), the 5th the remainder; 2346 tiles
    'many_passes': (BIG70, [(31154, 'rows'), (31120, 'rows'), (31183, 'rows'), (31149, 'rows'), (11710, 'plain')],
                    '70 pairs of 1900 ... 1996 rows: 5 passes'),
    # what test_varlen_patterns_launch_every_kernel_the_varlen_dispatch_can_launch asked for: the decoder GEMMs pick their tuned
    # configuration by the pass's M (csrc/gemm_tuned.inc, nearest M), so each of these is a pass of the R that reaches it
    'cov_510': ([17, 16, 18] * 10, [(510, 'fused')], 'the MLP linear 256x256 on cfg33'),
    'cov_1116': ([1000, 33, 0, 83], [(1116, 'plain')], 'linear 1024x256 cfg4, 256x1024 cfg25, 256x256 cfg36, 256x256 cfg3 +pos'),
    'cov_1313': ([1290, 23], [(1313, 'plain')], 'linear 1024x256 cfg41'),
    'cov_1427': ([196, 40, 324, 267, 0, 600], [(1427, 'plain')], 'linear 256x256 cfg25, and cfg25 +pos'),
    'cov_3000': ([1000, 999, 1001], [(3000, 'plain')], 'linear 256x1024 cfg4, 256x256 cfg4'),
    'cov_3136': ([686, 24, 1235, 89, 1102], [(3136, 'plain')], 'linear 256x1024 cfg12'),
    'cov_3598': ([250, 264] * 7, [(3598, 'plain')], 'linear 256x1024 cfg9'),
    'cov_16448': ([257] * 64, [(16448, 'plain')], 'linear 256x1024 cfg40 (257 rows: 7/8 of 5 64-row tiles fails, no rows form)'),
    'cov_19595': ([19393, 31, 7, 12, 152], [(19595, 'plain')], 'linear 256x1024 cfg27'),
}
PREFIX_CANDIDATES = [[q] * n + [s] * 3 for q in (1000, 1024, 900, 500) for n in range(8, 33) for s in (1, 17)]

_oracle = {}     # pattern name -> per pair: float64 / float32 pred_corrs, and query_pos / hs of the rows the taps hold
_worst = {}
_prefix = []


def pattern_pairs(name, b):
    offset = (29 * sorted(PATTERNS).index(name) + 5) % POOL if name in PATTERNS else 11
    return [(offset + j) % POOL for j in range(b)]


def pattern_queries(name, n):
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 7919 + n)
    qs = torch.rand(n, 2, generator=g)
    wide = torch.rand(n, 1, generator=g) < 0.05
    return torch.where(wide, torch.rand(n, 2, generator=g) * 2 - 0.5, qs)


def counts_of(name):
    return _prefix[0] if name == 'prefix_cut' else PATTERNS[name][0]


def inputs(name):
    counts = counts_of(name)
    P = pool()
    idx = pattern_pairs(name, len(counts))
    img = torch.stack([P['pairs'][i]['img'] for i in idx])
    return idx, img, pattern_queries(name, sum(counts))


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def profiled(m, fn):
    """(result of fn(), the per-launch names of its decoder: from its first posenc launch on; every decode pass starts with one)"""
    m.set_profiling(2)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = m.profile_names()
        assert 0 < len(names)
    finally:
        m.set_profiling(0)
    return out, names[names.index('posenc'):]


def passes_of(names):
    """[(R, form, attention launch name)] of one decode: a pass runs from its posenc launch to its head2 launch"""
    out, cur = [], []
    for n in names:
        assert (n == 'posenc') == (not cur), (n, cur)
        cur.append(n)
        if n == 'head2':
            att = [x for x in cur if x.startswith((FUSED, ROWS, PLAIN))]
            rs = {int(mm.group(1)) for x in cur for mm in [re.match(r'linear (\d+)x', x)] if mm}
            assert len(rs) == 1 and att, cur
            forms = {FORM_OF[k] for x in att for k in FORM_OF if x.startswith(k)}
            assert len(forms) == 1 and len(att) == 6, att                  # one attention launch per decoder layer, one form
            out.append((rs.pop(), forms.pop(), att[0]))
            cur = []
    assert not cur, cur
    return out


def pass_tiles(counts, rs, rows_per_tile):
    """tile-table entries of each pass of rows rs (every pair's rows inside the pass in tiles of rows_per_tile, as the kernels read)"""
    off, r0, out = offsets(counts), 0, []
    for r in rs:
        lo, hi = np.maximum(off[:-1], r0), np.minimum(off[1:], r0 + r)
        out.append(int(np.sum(np.where(hi > lo, (hi - lo + rows_per_tile - 1) // rows_per_tile, 0))))
        r0 += r
    return out


def run(m, name, **kw):
    _, img, q = inputs(name)
    return m.forward_varlen(img.cuda(), q.cuda(), counts_of(name), **kw).cpu()


def prefix_pattern(m):
    """A pass that vl_next_pass ends at a pair boundary below 32768 rows (batch_split's prefix rule), under the default knobs - the first
    candidate whose launch list shows it (the fill rules read the CU count)"""
    if not _prefix:
        P = pool()
        for counts in PREFIX_CANDIDATES:
            n = sum(counts)
            img = torch.stack([P['pairs'][i]['img'] for i in range(len(counts))]).cuda()
            _, names = profiled(m, lambda: m.forward_varlen(img, torch.rand(n, 2, device='cuda'), counts))
            ps = passes_of(names)
            if len(ps) == 2 and ps[0][0] == sum(counts[:-3]) and n <= 32768:
                _prefix.append(counts)
                _prefix.append([(r, f) for r, f, _ in ps])
                break
    assert _prefix, 'no candidate whose decode batch_split cuts at a pair boundary'
    return _prefix[0], _prefix[1]


def expected_passes(m, name):
    return prefix_pattern(m)[1] if name == 'prefix_cut' else PATTERNS[name][1]


def oracle(m, name):
    """per pair j with rows: float64 / float32 pred_corrs of its rows, and query_pos / hs of its rows inside the last pass (the rows the
    debug taps hold)"""
    if name not in _oracle:
        P = pool()
        idx, _, q = inputs(name)
        off = offsets(counts_of(name))
        tap_rows = (int(off[-1]) - expected_passes(m, name)[-1][0], int(off[-1]))
        per = {}
        with torch.no_grad():
            for j, i in enumerate(idx):
                a, b = int(off[j]), int(off[j + 1])
                if a == b:
                    continue
                t64, t32 = {}, {}
                d64 = O.cotr_decode(P['sd64'], P['pairs'][i]['mem64'], P['pos64'], q[a:b][None], torch.float64, taps=t64)
                d32 = O.cotr_decode(P['sd'], P['pairs'][i]['mem32'], P['pos32'], q[a:b][None], torch.float32, taps=t32)
                e = dict(rows=(a, b), p64=d64['pred_corrs'][0], p32=d32['pred_corrs'][0])
                lo, hi = max(a, tap_rows[0]), min(b, tap_rows[1])
                if lo < hi:
                    sl = slice(lo - a, hi - a)
                    e['tap_rows'] = (lo, hi)
                    e['query_pos'] = (t64['query_pos'][sl, 0], t32['query_pos'][sl, 0])
                    e['hs'] = (d64['hs'][sl, 0], d32['hs'][sl, 0])
                per[j] = e
        _oracle[name] = per
    return _oracle[name]


def px_bars(m, name):
    """per pair: (rows, float64 pred_corrs, bar)"""
    per = oracle(m, name)
    return {j: (e['rows'], e['p64'], max(PX_BAR, 3 * O.px_err(e['p32'], e['p64']))) for j, e in per.items()}


def record(rows, label):
    worst_here = {}
    for s, p, e, bar in rows:
        if e / bar > worst_here.get(s, (-1.0,))[0]:
            worst_here[s] = (e / bar, e, bar, p)
        if e / bar > _worst.get(s, (-1.0,))[0]:
            _worst[s] = (e / bar, label, p)
    print(f'\n{label}: ' + '  '.join(f'{s} {r:.3f} ({e:.2e}/{bar:.1e})' for s, (r, e, bar, _) in worst_here.items()))
    print('worst err/bar so far: ' + '  '.join(f'{s} {r:.3f} @{lb}' for s, (r, lb, _) in _worst.items()))
    return worst_here


# ---- 1 + 2: every stage of every pair against float64, the passes from the profile ------------------------------------------------
@pytest.mark.parametrize('name', list(PATTERNS) + ['prefix_cut'])
def test_every_pair_of_a_varlen_call_against_float64(name):
    m = hip_model()
    want = expected_passes(m, name)
    counts = counts_of(name)
    n = sum(counts)
    out = run(m, name)
    assert out.shape == (n, 2) and torch.isfinite(out).all()
    prof_out, names = profiled(m, lambda: run(m, name))
    assert torch.equal(prof_out, out)
    got = passes_of(names)
    assert [(r, f) for r, f, _ in got] == want, f'{name}: passes {[(r, f) for r, f, _ in got]}, built for {want}'
    assert all(a.endswith(' vl') or f == 'rows' for _, f, a in got), got
    last = want[-1][0]
    m.set_debug_taps(True)
    try:
        run(m, name)
        taps = {s: m.debug_tap(s).view(last, 256).cpu() for s in ('query_pos', 'hs')}
    finally:
        m.set_debug_taps(False)

    per = oracle(m, name)
    idx = pattern_pairs(name, len(counts))
    rows = []
    for j, e in per.items():
        a, b = e['rows']
        rows.append(('pred_corrs', idx[j], O.px_err(out[a:b], e['p64']), max(PX_BAR, 3 * O.px_err(e['p32'], e['p64']))))
        if 'tap_rows' in e:
            lo, hi = e['tap_rows']
            for s in ('query_pos', 'hs'):
                r64, r32 = e[s]
                rows.append((s, idx[j], _rel(taps[s][lo - (n - last):hi - (n - last)], r64), max(FLOOR[s], 4 * _rel(r32, r64))))
    worst = record(rows, name)
    assert {'pred_corrs', 'query_pos', 'hs'} <= set(worst)
    bad = [(s, p, f'{e:.3e} > {bar:.3e}') for s, p, e, bar in rows if not e <= bar]
    assert not bad, f'{len(bad)} (stage, pool pair) over the bar in {name}: {bad[:20]}'


def test_the_patterns_reach_every_planner_branch():
    """what the patterns are for, in one place: the three default-knob forms, the prefix cut, a cut inside a pair among other pairs,
    R < B; then the plain form of many_passes needs more than 4096 tile entries (the staging slot grows: test_ring_slot_grows_...)"""
    m = hip_model()
    forms = {f for name in PATTERNS for _, f in PATTERNS[name][1]}
    assert forms == {'fused', 'rows', 'plain'}
    counts, ps = prefix_pattern(m)
    assert len(ps) == 2 and ps[0][0] < 32768 and ps[0][0] in offsets(counts)
    c, ps = PATTERNS['cut_inside_a_pair'][:2]
    assert ps[0][0] not in offsets(c) and len([x for x in c if x]) > 2
    c, ps = PATTERNS['rows_below_pairs'][:2]
    assert ps[0][0] < len(c)


# ---- 3: poisoned scratch and a guard row ------------------------------------------------------------------------------------------
GUARD = -7.25


def raw_call(m, nbytes, fill, call, n):
    """call(out_ptr) on a caller workspace of exactly nbytes (cotr_set_workspace, keep_encode 0) filled with `fill`; out: n + 1 rows
    of NaN, the last one a guard.  The model's own workspace is dropped afterwards (its next call sizes and hands over a new one)."""
    out = torch.full((n + 1, 2), float('nan'), device='cuda')
    out[n] = GUARD
    with raw_abi.caller_workspace(m, nbytes, fill):
        rc = call(out.data_ptr())
        assert rc == 0, _lib.load_library().cotr_last_error(m._handle)
    return out.cpu()


def varlen_in_workspace(m, img, q, counts, fill):
    lib = _lib.load_library()
    arr = (ctypes.c_int * (len(counts) + 1))(*offsets(counts).tolist())
    imgd, qd = img.cuda().contiguous(), q.cuda().contiguous()
    return raw_call(m, raw_abi.scratch_bytes_varlen(m, arr), fill,
                    lambda o: lib.cotr_forward_varlen(m._handle, imgd.data_ptr(), qd.data_ptr(), arr, len(counts), o,
                                                      _lib.current_stream_ptr()), sum(counts))


def uniform_in_workspace(m, img, q, fill):
    lib = _lib.load_library()
    b, nq = q.shape[:2]
    imgd, qd = img.cuda().contiguous(), q.cuda().contiguous()
    return raw_call(m, raw_abi.scratch_bytes(m, b, nq), fill,
                    lambda o: lib.cotr_forward(m._handle, imgd.data_ptr(), qd.data_ptr(), b, nq, o, _lib.current_stream_ptr()), b * nq)


def check_poisoned(nan, zero, n):
    assert torch.isfinite(nan[:n]).all(), f'{int((~torch.isfinite(nan[:n])).any(1).sum())} rows read poisoned scratch'
    assert (nan[n] == GUARD).all() and (zero[n] == GUARD).all(), 'the guard row behind the output was written'
    assert torch.equal(nan[:n], zero[:n])


POISON_PATTERNS = ['edges_fused', 'edges_plain', 'edges_rows', 'empty_pairs', 'rows_below_pairs', 'cut_inside_a_pair', 'prefix_cut']
VL_FORMS = ['fused', 'rows', 'plain']


@pytest.mark.parametrize('form', VL_FORMS)
@pytest.mark.parametrize('name', POISON_PATTERNS)
def test_varlen_on_poisoned_scratch(name, form):
    """The whole workspace is scratch or the encode cache (include/cotr_hip.h; the positional table and weights live in the handle), and
    cotr_forward_varlen rewrites the encode cache: a row no tile covers shows up as NaN, a stale row as a difference to the zero fill."""
    m = hip_model()
    if name == 'prefix_cut':
        prefix_pattern(m)
    _, img, q = inputs(name)
    counts = counts_of(name)
    with G.model_knobs(m, **FORMS[form][0]):
        nan = varlen_in_workspace(m, img, q, counts, float('nan'))
        zero = varlen_in_workspace(m, img, q, counts, 0.0)
    check_poisoned(nan, zero, sum(counts))


@pytest.mark.parametrize('b,nq', [(3, 333), (17, 1000)])
def test_uniform_on_poisoned_scratch(b, nq):
    m = hip_model()
    P = pool()
    img = torch.stack([P['pairs'][i]['img'] for i in range(b)])
    q = pattern_queries(f'uniform{b}', b * nq).view(b, nq, 2)
    nan = uniform_in_workspace(m, img, q, float('nan'))
    zero = uniform_in_workspace(m, img, q, 0.0)
    check_poisoned(nan, zero, b * nq)
    assert torch.equal(nan[:-1].view(b, nq, 2), m(img.cuda(), q.cuda())['pred_corrs'].cpu())


# ---- 4: varlen == uniform, bit for bit, where the launches are the same -------------------------------------------------------------
UNIFORM_SHAPES = [(4, 300), (8, 512), (24, 100), (1, 1000)]
_uniform_report = {}


@pytest.mark.parametrize('form', VL_FORMS)
@pytest.mark.parametrize('b,nq', UNIFORM_SHAPES, ids=[f'{b}x{q}' for b, q in UNIFORM_SHAPES])
def test_varlen_equals_the_uniform_call_where_the_launches_agree(b, nq, form):
    """include/cotr_hip.h: "the result of every row is that of a uniform call on its pair".  With equal counts the varlen kernels do
    the uniform kernels' per-row arithmetic (tile placement and xcd_mapping change neither): where the decoder launch lists agree
    (' vl' dropped) the outputs are equal bit for bit; elsewhere within SHAPE_NOISE_PX, and the launch that differs is named."""
    m = hip_model()
    P = pool()
    img = torch.stack([P['pairs'][i]['img'] for i in range(b)]).cuda()
    q = pattern_queries(f'uniform{b}', b * nq).cuda()
    with G.model_knobs(m, **FORMS[form][0]):
        uni, un = profiled(m, lambda: m(img, q.view(b, nq, 2))['pred_corrs'].cpu())
        vl, vn = profiled(m, lambda: m.forward_varlen(img, q, [nq] * b).cpu())
    vn = [re.sub(r' vl$', '', x) for x in vn]
    vl = vl.view(b, nq, 2)
    if un == vn:
        assert torch.equal(vl, uni), f'same launches, {O.px_err(vl, uni):.3e} px apart'
        _uniform_report[(b, nq, form)] = 'bit-identical'
    else:
        diff = sorted(set(un) ^ set(vn))
        _uniform_report[(b, nq, form)] = diff
        print(f'\n{b} x {nq} {form}: launch lists differ: {diff}')
        assert O.px_err(vl, uni) < SHAPE_NOISE_PX, diff


# ---- 5: every knob value on varlen calls ------------------------------------------------------------------------------------------
# the varlen planner's reach, for the knobs it reads: value -> 'changes' (the decoder launch list differs from the base knobs' one at
# some pattern of REACH_PATTERNS), 'default' (it is the same at every one, and why), or ('has', regex) for a knob that acts inside a
# kernel (a launch of it runs).  Values not listed: not read by the varlen decoder (encoder only).
def S_VL(form, splits):
    return '^' + re.escape(f'{form} s{splits} vl') + '$'


VL_REACH = {
    'attention_splits': {0: 'default', 4: 'default', **{v: ('changes', S_VL(PLAIN, v)) for v in (1, 2, 8, 16)}},   # 0 means 4
    'attention_fused_splits': {0: 'default', 4: 'default', 8: ('changes', S_VL(FUSED, 8)), 48: ('changes', S_VL(FUSED, 8)),
                               84: ('default', S_VL(FUSED, 4))},                  # 48 / 84: 8 / 4 splits in the decoder
    'xcd_mapping': {v: 'default' for v in (0, 1, 2, 1 | 4, 1 | 16, 1 | 32)} | {1 | 8: ('default', r' dec s\d+ vl$')},   # placement only
    'att_rows_min_rows': {0: 'changes', 1 << 30: 'changes'},       # 0 with rows_min_fill 0: mid_rows takes att_rows
    'ffn_rows_min_rows': {0: 'changes', 1 << 30: 'changes'},
    'rows_min_fill': {0: 'changes', 100: 'changes'},               # 0: fill9 takes the rows kernels; 100: edges_rows does not
    'attention_fusion_max_rows': {0: 'changes', 1 << 30: 'default'},   # above 4096 rows the FFN fusion refuses the fused form anyway
    'ffn_fusion_max_rows': {0: 'changes', 1 << 30: 'changes'},     # mid_rows' 7424 rows fill the fused FFN's two rounds
    'ffn_fused_max_chunks': {2: 'changes', 4: 'changes', 8: 'changes', 16: 'default'},
    'batch_split': {0: 'changes', 1: 'default'},                    # prefix_cut in one pass
}
REACH_EXTRA = {'mid_rows': [1024] * 7 + [256], 'fill9': [1024] * 9}     # plain under the defaults: 7424 rows, 9216 rows in 144 tiles
SWEEP = ['edges_fused', 'edges_rows']     # the fused form, and the rows form (plain under some knobs)
_default_vl, _reach_base = {}, {}


def reach_counts(m):
    return {'edges_fused': counts_of('edges_fused'), 'edges_rows': counts_of('edges_rows'), 'edges_plain': counts_of('edges_plain'),
            'prefix_cut': prefix_pattern(m)[0], **REACH_EXTRA}


def decoder_names(m, counts):
    P = pool()
    img = torch.stack([P['pairs'][i % POOL]['img'] for i in range(len(counts))]).cuda()
    q = pattern_queries('reach', sum(counts)).cuda()
    return profiled(m, lambda: m.forward_varlen(img, q, counts))[1]


def _sweep_ids():
    seen, out = set(), []
    for k, v, _, _, base in case_runs():
        if (k, v) not in seen:
            seen.add((k, v))
            out.append((k, v, base))
    return out


@pytest.mark.parametrize('knob,value,base', _sweep_ids(), ids=[f'{k}={v}' for k, v, _ in _sweep_ids()])
def test_knob_value_on_varlen_calls(knob, value, base):
    m = hip_model()
    for name in SWEEP:
        if name not in _default_vl:
            _default_vl[name] = run(m, name)
    with G.model_knobs(m, **base, **{knob: value}):
        for name in SWEEP:
            out = run(m, name)
            assert torch.isfinite(out).all(), name
            assert torch.equal(out, run(m, name)), f'{name}: not bit-repeatable'
            _, img, q = inputs(name)
            assert torch.equal(varlen_in_workspace(m, img, q, counts_of(name), 0.0)[:-1], out), \
                f'{name}: another result in a workspace of cotr_scratch_bytes_varlen'
            ref = _default_vl[name]
            if KNOB_CASES[knob]['bits'] == 'same':
                assert torch.equal(out, ref), (name, O.px_err(out, ref))
            assert O.px_err(out, ref) < SHAPE_NOISE_PX, name
            bad = [j for j, ((a, b), p64, bar) in px_bars(m, name).items() if not O.px_err(out[a:b], p64) <= bar]
            assert not bad, f'{name}: pairs {bad} over the float64 bar'
        reach = VL_REACH.get(knob, {}).get(value)
        if reach is None:
            return
        assert value in VL_REACH[knob]
        kind, pattern = (reach, None) if isinstance(reach, str) else reach
        names = {p: decoder_names(m, c) for p, c in reach_counts(m).items()}
    bkey = tuple(sorted(base.items()))
    if bkey not in _reach_base:
        with G.model_knobs(m, **base):
            _reach_base[bkey] = {p: decoder_names(m, c) for p, c in reach_counts(m).items()}
    ref = _reach_base[bkey]
    changed = [p for p in names if names[p] != ref[p]]
    if kind == 'changes':
        assert changed, f'{knob}={value} changes no varlen launch list'
    else:
        assert not changed, f'{knob}={value} changes the launches at {changed}'
    if pattern:
        assert any(re.search(pattern, x) for v in names.values() for x in v), f'no launch matching {pattern!r}'


def test_every_varlen_knob_value_of_the_table_is_in_the_sweep():
    values = {(k, v) for k, v, _ in _sweep_ids()}
    for knob, vals in VL_REACH.items():
        assert set(vals) == {v for k, v in values if k == knob}, f'{knob}: VL_REACH and knob_cases.py list other values'


# ---- the staging ring -------------------------------------------------------------------------------------------------------------
def test_ring_slot_grows_with_its_copy_in_flight():
    """A fresh handle: four small decode_varlen calls (each takes a ring slot of 4096 entries), then - no host synchronisation in
    between - many_passes under the plain form: 5 passes, more than 4096 tile entries, in the slot of the first small call, whose copy
    may still be in flight.  Every output against float64 (the small calls decode prefixes of many_passes' rows of each pair)."""
    import cotr_amd
    from cotr_amd.models import build_model
    from cotr_amd.utils.synth import synth_state_dict
    m = build_model(cotr_amd.default_args()).cuda().eval()
    m.load_state_dict(synth_state_dict(0))
    name = 'many_passes'
    counts = counts_of(name)
    _, img, q = inputs(name)
    off = offsets(counts)
    for k, v in FORMS['plain'][0].items():
        m.set_knob(k, v)
    m.encode(img.cuda())
    qd = q.cuda()
    smalls = [[(3 * j + k) % 7 * (j % 5) for j in range(70)] for k in range(4)]
    outs = []
    for c in smalls:
        outs.append(m.decode_varlen(torch.cat([qd[off[j]:off[j] + c[j]] for j in range(70)]), c))
    big, names = profiled(m, lambda: m.decode_varlen(qd, counts))
    rs = [r for r, _, _ in passes_of(names)]
    assert len(rs) == 5 and sum(rs) == sum(counts)
    assert sum(pass_tiles(counts, rs, 32)) > 4096
    bars = px_bars(hip_model(), name)
    for c, o in zip(smalls + [counts], outs + [big]):
        o, r0 = o.cpu(), 0
        for j, n in enumerate(c):
            if n:
                (a, _), p64, bar = bars[j]
                assert O.px_err(o[r0:r0 + n], p64[:n]) <= bar, (c, j)
            r0 += n
    m.set_profiling(0)


# ---- 6: dispatch coverage of varlen calls -----------------------------------------------------------------------------------------
def coverage_grid():
    """B = 1 ... 70 (the pairs behind B empty): all-equal counts at each COVERAGE_Q, uniform-random counts in [0, 2Q], one heavy pair
    plus light ones"""
    rng = np.random.Generator(np.random.PCG64(17))
    for b in range(1, POOL + 1):
        for q in COVERAGE_Q:
            yield [q] * b + [0] * (POOL - b)
            yield [int(x) for x in rng.integers(0, 2 * q + 1, b)] + [0] * (POOL - b)
        yield [int(rng.integers(1000, 20000))] + [int(x) for x in rng.integers(0, 40, b - 1)] + [0] * (POOL - b)


def test_varlen_patterns_launch_every_kernel_the_varlen_dispatch_can_launch():
    m = hip_model()
    checked = set()
    for name in list(PATTERNS) + ['prefix_cut']:
        if name == 'prefix_cut':
            prefix_pattern(m)
        _, img, q = inputs(name)
        checked |= {launch_key(x) for x in profiled(m, lambda: m.forward_varlen(img.cuda(), q.cuda(), counts_of(name)))[1]}
    g = torch.Generator(device='cuda').manual_seed(3)
    img = torch.randn(POOL, 3, 256, 512, device='cuda', generator=g)     # the dispatch does not look at the data
    qs = torch.rand(POOL * 2000 + 20000, 2, device='cuda', generator=g)
    m.encode(img)
    first = {}
    for counts in coverage_grid():
        for k in {launch_key(x) for x in profiled(m, lambda: m.decode_varlen(qs[:sum(counts)], counts))[1]} - checked:
            first.setdefault(k, (len([c for c in counts if c]), sum(counts), counts[:4]))
    assert not first, 'varlen launch keys no pattern reaches (key <- first grid pattern: pairs with rows, rows, first counts):\n' + \
        '\n'.join(f'  {k}  <- {v}' for k, v in sorted(first.items()))
