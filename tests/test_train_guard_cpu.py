"""What tests/test_train_guard_gpu.py stands on, without a GPU: the case table of tests/train_guard_cases.py against the training
section of include/cotr_hip.h (every entry point that launches a kernel has a row, the rest are the listed host-only calls), every
case laid out in a guarded arena on ``device='cpu'`` with the prototype's arguments, the host size queries against closed forms,
the float64 restatement (tests/train_kernel_oracle.py) against torch float64 autograd, the yardstick figures, and three doctored
references that the comparison functions must refuse."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dropout_oracle as do
from tests import train_guard_cases as tg
from tests import train_kernel_oracle as ko
from tests.guard_arena import KINDS
from tests.scratch_guard_cases import AuxOut, In, Out, Table, place

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cotr_hip.h')
F32 = np.float32


@pytest.fixture(scope='module')
def lib():
    from cotr_amd import _lib
    from cotr_amd.build import build_library
    build_library()
    return _lib.load_library()


# ---- the table against the header -----------------------------------------------------------------------------------------------
def training_section():
    text = open(HEADER).read()
    start = text.index('/* ---- training step')
    return text[start:text.index('\n/* ----', start + 1)]


def training_entry_points():
    text = re.sub(r'/\*.*?\*/', '', training_section(), flags=re.S)
    return {m.group(1): ' '.join(m.group(2).split()) for m in re.finditer(r'\b(?:int|size_t)\s+(cotr_\w+)\s*\(([^;{]*?)\)\s*;', text, flags=re.S)}


def test_every_training_entry_point_has_a_row_or_is_host_only():
    header = set(training_entry_points())
    rows, host = {r.name for r in tg.ROWS}, set(tg.HOST_ONLY)
    assert len(header) == 29 and all(n.startswith('cotr_train_') for n in header)
    assert len(rows) == len(tg.ROWS) and not rows & host
    assert header - host == rows, f'without a row: {sorted(header - host - rows)}; rows without an entry point: {sorted(rows - header)}'
    assert host == header - rows and all(n.endswith(('_parts', '_splits', '_scratch', '_dropout_salt')) for n in host)
    for r in tg.ROWS:
        ids = [c.id for c in r.cases]
        assert len(set(ids)) == len(ids), r.name
        assert r.early is None or r.early[0] in ids, r.name
        assert (r.query is None) == (r.early is None), r.name                              # every op with a part or scratch has its control
    ids = [i for i, _, _ in tg.special_calls()]
    assert len(set(ids)) == len(ids)


def test_the_header_states_the_alignment_of_every_training_pointer():
    text = training_section()
    assert '16-byte aligned' in text and '4-byte aligned' in text
    for name, args in training_entry_points().items():
        if name in tg.HOST_ONLY:
            continue
        pointers = re.findall(r'(?:float|unsigned|cotr_\w+_job|cotr_reduce_src)\s*\*\s*(\w+)', args)
        assert pointers, name
        m = re.search(r'/\* alignment of ' + name + r': (.*?)\*/', text, flags=re.S)
        assert m, f'{name}: no alignment line in the header'
        for ptr in pointers:
            assert re.search(r'\b' + ptr + r'\b', m.group(1)), f'{name}: the alignment of `{ptr}` is not stated'


def test_no_case_is_heavier_than_the_issue_allows():
    for r, c, mode in tg.all_cases():
        call = r.build(c.params, mode)
        for a in call.args:
            nbytes = a.array.nbytes if hasattr(a, 'array') else (int(np.prod(a.shape)) * np.dtype(a.dtype).itemsize if isinstance(a, (Out, AuxOut, Table)) else 0)
            assert nbytes <= 32 << 20, (r.name, c.id, a.name, nbytes)
        if r.name.startswith('cotr_train_gemm_tn'):
            assert c.params[0] <= 4100
        if r.name.startswith('cotr_train_attention'):
            assert c.params[1] <= 12 and c.params[2] <= 129
        if r.name == 'cotr_train_conv_wgrad_parts':
            B, Hin, Win, _, _, k, s = c.params
            assert B * ko.conv_out(Hin, k, s) * 2 * ko.conv_out(Win, k, s) <= 4100


# ---- every case can be laid out, with the prototype's arguments -----------------------------------------------------------------
@pytest.mark.parametrize('row', tg.ROWS, ids=lambda r: r.name[11:])
def test_every_case_can_be_laid_out(lib, row):
    calls = [(c.id, row.build(c.params, mode)) for c in row.cases for mode in tg.MODES[row.cls]]
    calls += [(i, call) for i, name, call in tg.special_calls() if name == row.name]
    fn = getattr(lib, row.name)
    for ident, call in calls:
        arena, argv, outs = place(call, 0, 'cpu', 0xA5)
        assert len(fn.argtypes) == len(argv), (ident, len(fn.argtypes), len(argv))
        for t, a in zip(fn.argtypes, argv):
            t.from_param(a)
        for a in call.args:
            if isinstance(a, (In, Out, AuxOut, Table)) or hasattr(a, 'array'):
                kind = a.kind
                assert kind in ('a16', 'f32', 'a8'), (ident, a.name)                        # the least the header documents, and no more
                res, mod = KINDS[kind]
                assert arena.addr(a.name) % mod == res, (ident, a.name)
        for name, array in (call.init or {}).items():
            assert arena.nbytes(name) == np.asarray(array).nbytes, (ident, name)
        arena.check()
        assert all(arena.all_fill(name) for name in outs)


# ---- the host queries against closed forms ----------------------------------------------------------------------------------------
def test_size_queries_at_every_case_and_over_a_sweep(lib):
    rows_seen = set(range(0, 5001))
    for r, c, _ in tg.all_cases():
        if r.name in ('cotr_train_ln_bwd', 'cotr_train_head_bwd'):
            rows_seen.add(c.params[0])
        if r.name == 'cotr_train_colsum':
            rows_seen.add(c.params[0])
        if r.name in ('cotr_train_gemm_tn', 'cotr_train_gemm_tn_parts'):
            M, N, K, _ = c.params
            assert lib.cotr_train_gemm_tn_splits(M, N, K) == ko.gemm_tn_splits(M, N, K), c.id
        if r.name == 'cotr_train_attention_bwd':
            assert lib.cotr_train_attention_bwd_scratch(c.params[1], c.params[2]) == 4 * c.params[1] * c.params[2] * 256
    for n in sorted(rows_seen):
        for query, closed, per, most in ((lib.cotr_train_ln_bwd_parts, ko.ln_bwd_parts, ko.ln_bwd_per, 512),
                                         (lib.cotr_train_head_bwd_parts, ko.head_bwd_parts, ko.head_bwd_per, 256),
                                         (lib.cotr_train_colsum_parts, ko.colsum_parts, ko.colsum_per, 256)):
            if n == 0:
                assert query(0) == 0 and query(-3) == 0                                      # (no partials; these used to divide by zero)
                continue
            parts = query(n)
            assert parts == closed(n) and 1 <= parts <= most, (n, parts)
            assert parts * per(n) >= n > (parts - 1) * per(n), n                              # the parts cover the rows and the last is not empty
            assert per is ko.colsum_per or per(n) % 4 == 0
        for N, K in ((64, 64), (128, 64), (256, 256), (512, 256), (128, 1024), (1024, 256)):
            splits = lib.cotr_train_gemm_tn_splits(n, N, K)
            assert splits == ko.gemm_tn_splits(n, N, K) and splits >= 1, (n, N, K)
            if n:
                per, nsplit = ko.gemm_tn_plan(n, N, K)
                assert per % 32 == 0 and splits >= -(-n // per) == nsplit >= 1, (n, N, K)      # the partials written fit what the query sizes
    assert ko.gemm_tn_plan(4100, 256, 256) == (160, 26) and lib.cotr_train_gemm_tn_splits(4100, 256, 256) == 32
    assert ko.gemm_tn_plan(2049, 512, 256) == (256, 9) and ko.gemm_tn_plan(256, 64, 64) == (128, 2)
    assert lib.cotr_train_attention_bwd_scratch(0, 5) == 0 and lib.cotr_train_attention_bwd_scratch(12, 129) == 4 * 12 * 129 * 256
    assert ko.ln_bwd_per(2047) == ko.ln_bwd_per(2048) == 4 and ko.ln_bwd_per(2049) == 8


# ---- the restatement against torch float64 autograd -----------------------------------------------------------------------------
def t64(a, grad=False):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).clone().requires_grad_(grad)


def close(a, b, tol=1e-11):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b.detach() if torch.is_tensor(b) else b, dtype=np.float64)
    assert a.shape == b.shape and np.abs(a - b).max(initial=0) <= tol * max(1.0, np.abs(b).max(initial=0)), np.abs(a - b).max(initial=0)


@pytest.mark.parametrize('rows,p', [(3, 0.0), (70, 0.1)])
def test_restatement_layernorm(rows, p):
    seed = 77
    a, x, w, b, s = tg._ln_inputs(rows, True, p, seed)
    keep = do.flat_mask(seed, rows, 256, p)
    at, xt, wt, bt = t64(a, True), t64(x, True), t64(w, True), t64(b, True)
    st = xt + at * t64(np.where(keep, float(F32(do.inv_keep(p))), 0.0) if p else np.ones_like(a))
    close(s, st, 1e-6)                                                                      # (s is the float32 sum)
    s_in = t64(s, True)
    y = F.layer_norm(s_in, (256,), wt, bt, 1e-5)
    (yr, _), (mean, _), (rstd, _) = ko.ln_fwd(s, w, b)
    close(yr, y)
    dy = tg.data('rand', 5, rows, 256)
    y.backward(t64(dy))
    ref = ko.ln_bwd(dy, s, np.stack([mean, rstd], 1), w)
    close(ref['ds'][0], s_in.grad)
    close(ref['gamma'][0], wt.grad)
    close(ref['beta'][0], bt.grad)
    close(ref['gamma_part'][0].sum(0), wt.grad)
    close(ref['beta_part'][0].sum(0), bt.grad)
    assert ref['gamma_part'][0].shape == (ko.ln_bwd_parts(rows), 256)


@pytest.mark.parametrize('nb,nq,p', [(1, 5, 0.0), (2, 33, 0.1)])
def test_restatement_attention(nb, nq, p):
    seed = 1234
    q, k, v = tg.data('rand', 1, nb * nq, 256), tg.data('rand', 2, nb * 512, 256), tg.data('rand', 3, nb * 512, 256)
    d_o = tg.data('rand', 4, nb * nq, 256)
    qt, kt, vt = t64(q, True), t64(k, True), t64(v, True)
    heads = lambda x, n: x.reshape(nb, n, 8, 32).permute(0, 2, 1, 3)   # noqa: E731
    s = heads(qt, nq) @ heads(kt, 512).transpose(-1, -2) * float(F32(tg.QSCALE))
    pd = torch.softmax(s, -1)
    if p:
        pd = pd * t64(np.where(do.attention_mask(seed, nb, nq, p), float(F32(do.inv_keep(p))), 0.0))
    o = (pd @ heads(vt, 512)).permute(0, 2, 1, 3).reshape(nb * nq, 256)
    (oref, _), (lse, _) = ko.attention_fwd(q, k, v, nb, nq, tg.QSCALE, p, seed)
    close(oref, o)
    close(lse, (torch.logsumexp(s, -1) / np.log(2.0)).permute(0, 2, 1).reshape(nb * nq, 8))
    o.backward(t64(d_o))
    ref = ko.attention_bwd(q, k, v, oref, d_o, lse, nb, nq, tg.QSCALE, p, seed)             # (o and lse in float64: no rounding to account for)
    close(ref['dq'][0], qt.grad, 1e-10)
    close(ref['dk'][0], kt.grad, 1e-10)
    close(ref['dv'][0], vt.grad, 1e-10)
    close(ref['delta'][0], (o.detach() * t64(d_o)).reshape(nb * nq, 8, 32).sum(-1))


@pytest.mark.parametrize('rows', [3, 300])
def test_restatement_head_and_relu(rows):
    x, w, b, dy = tg.data('rand', 1, rows, 256), tg.data('rand', 2, 512), tg.data('rand', 3, 2), tg.data('rand', 4, rows, 2)
    xt, wt, bt = t64(x, True), t64(w.reshape(2, 256), True), t64(b, True)
    y = xt @ wt.T + bt
    close(ko.head_fwd(x, w, b)[0], y)
    y.backward(t64(dy))
    dh, part, dwb = ko.head_bwd(dy, x, w)
    close(dh[0], xt.grad)
    close(dwb[0], torch.cat([wt.grad.reshape(-1), bt.grad]))
    close(part[0].sum(0), dwb[0])
    assert part[0].shape == (ko.head_bwd_parts(rows), 514)
    ht = t64(x, True)
    torch.relu(ht).backward(t64(tg.data('rand', 5, rows, 256)))
    close(ko.relu_drop_bwd(tg.data('rand', 5, rows, 256), np.maximum(x, 0), 0.0), ht.grad, 1e-7)


@pytest.mark.parametrize('params', [(2, 5, 4, 4, 3, 2), (1, 2, 3, 8, 3, 1), (2, 5, 4, 4, 1, 2)])
def test_restatement_im2col_col2im_against_unfold(params):
    B, Hin, Win, Cin, k, s = params
    x = tg.data('rand', 9, B, Hin, 2 * Win, Cin)
    xt = t64(x, True)
    halves = xt.reshape(B, Hin, 2, Win, Cin).permute(0, 2, 4, 1, 3).reshape(B * 2, Cin, Hin, Win)     # each half on its own, NCHW
    u = F.unfold(halves, k, padding=k // 2, stride=s)                                                  # [B*2][Cin*k*k][Hout*Wout]
    Hout, Wout = ko.conv_out(Hin, k, s), ko.conv_out(Win, k, s)
    col = u.reshape(B, 2, Cin, k * k, Hout, Wout).permute(0, 4, 1, 5, 3, 2).reshape(B * Hout * 2 * Wout, k * k * Cin)
    close(ko.im2col(x, *params), col)
    dcol = tg.data('rand', 10, *col.shape)
    col.backward(t64(dcol))
    close(ko.col2im(dcol, *params)[0], xt.grad)


@pytest.mark.parametrize('M,N,K', [(33, 64, 64), (2049, 512, 256)])
def test_restatement_gemm_colsum_sum_parts(M, N, K):
    A, B = tg.data('rand', 1, M, N), tg.data('rand', 2, M, K)
    want = torch.cat([(t64(A).T @ t64(B)).reshape(-1), t64(A).sum(0)])
    close(ko.gemm_tn(A, B, 1)[0], want)
    part, sab, per = ko.gemm_tn_parts(A, B, 1)
    close(part.sum(0), want)
    assert part.shape[0] == ko.gemm_tn_plan(M, N, K)[1] and (sab >= np.abs(part)).all()
    (out, _), (cpart, _) = ko.colsum(A)
    close(out, t64(A).sum(0))
    close(cpart.sum(0), out)
    close(ko.sum_parts(part.astype(F32))[0], t64(part.astype(F32)).sum(0))


@pytest.mark.parametrize('taps,cin,rows', [(1, 0, 5), (9, 4, 3)])
def test_restatement_reduce_job_and_moves(taps, cin, rows):
    row_len = 36
    dst, scale = tg.data('rand', 1, rows * row_len), tg.data('rand', 2, rows)
    srcs = [tg.data('rand', 3, 4, rows * row_len), tg.data('rand', 4, 2, rows * row_len)]
    tot = sum(t64(s).sum(0) for s in srcs).reshape(rows, row_len) * t64(scale)[:, None]
    if taps > 1:
        tot = tot.reshape(rows, taps, cin).transpose(1, 2)                                  # [row][tap][cin] -> torch's [row][cin][tap]
    close(ko.reduce_job(dst, srcs, scale, row_len, cin, taps)[0], t64(dst) + tot.reshape(-1))
    w = tg.data('rand', 5, rows, row_len)
    close(ko.scale_rows(w, scale), t64(w) * t64(scale)[:, None], 1e-7)
    close(ko.transpose(w.reshape(1, rows, row_len)), t64(w).T[None])
    src = tg.data('rand', 6, 2 * rows * row_len)
    want = torch.flip(t64(src).reshape(2, rows, row_len), (0,)).transpose(1, 2) * t64(scale)[None, None, :]
    close(ko.perm_job(src, 2, rows, row_len, rows * row_len, row_len, 1, scale, True), want, 1e-7)
    close(ko.add_rowmod(w, w[:2], 2), t64(w) + t64(w[:2]).repeat(rows, 1)[:rows], 1e-7)


@pytest.mark.parametrize('steps', [1, 3])
def test_restatement_adam_against_torch_optim(steps):
    p0 = tg.data('rand', 1, 50)
    param = torch.nn.Parameter(t64(p0))
    opt = torch.optim.Adam([param], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    p, m, v = p0.astype(np.float64), np.zeros(50), np.zeros(50)
    for t in range(1, steps + 1):
        g = tg.data('rand', 10 + t, 50)
        param.grad = t64(g)
        opt.step()
        # (the restatement rounds the constants to float32 as the launcher does: compare at that precision)
        (p, _), (m, _), (v, _) = ko.adam(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1 - 0.9 ** t, np.sqrt(1 - 0.999 ** t))
        (p2, _), _, _ = ko.adam(p0, g, m * 0, v * 0, 1e-3, 0.9, 0.999, 1e-8, 0, 0, step=1.0) if t == 1 else ((None, None), 0, 0)
    close(p, param, 1e-6)
    if steps == 1:
        close(p2, param, 1e-6)


# ---- the yardstick --------------------------------------------------------------------------------------------------------------
def test_the_yardstick_figures_reproduce_the_constants():
    worst = {}
    for r, c, mode in tg.all_cases():
        call = r.build(c.params, mode)
        if call.yard is not None:
            for key, ratio in call.yard().items():
                worst[key] = max(worst.get(key, 0.0), ratio)
    assert set(worst) == set(tg.YARD)
    for key, ratio in worst.items():
        assert tg.YARD[key] / 1.5 <= ratio <= tg.YARD[key] * 1.5, (key, ratio, tg.YARD[key])     # (another BLAS may sum in another order)
        assert ratio < 1e-3 and tg.bound(key) == 8 * tg.YARD[key]
    for key, ratio in tg.KERNEL_WORST.items():
        assert ratio <= tg.bound(key), key


# ---- doctored references: the comparison of each class refuses a subtly wrong result --------------------------------------------------
def test_a_dropped_last_row_fails_the_sum_comparison():
    M, N = 1000, 64
    for mode in ('int', 'rand'):
        x = tg.data(mode, 3, M, N)
        (out, sab), _ = ko.colsum(x)
        tg.check_sum(x.astype(np.float64).sum(0).astype(F32), out, sab, M, mode, 'out')
        short = x[:-1].astype(np.float64).sum(0).astype(F32)                               # what a kernel that drops row M - 1 returns
        with pytest.raises(AssertionError, match='out'):
            tg.check_sum(short, out, sab, M, mode, 'out')
    # the measure the older tests use does not see it
    assert np.abs(short - out).max() / np.abs(out).max() < 0.2


def test_a_tile_edge_off_by_one_fails_the_move_comparison():
    R, C = 33, 31
    src = tg.data('rand', 4, R, C)
    want = ko.transpose(src)
    tg.check_bits(want.copy(), want, 'dst')
    wrong = want.copy()
    wrong[:, 32] = 0.0                                                                      # the second row tile (r = 32) never written
    with pytest.raises(AssertionError, match=r'31 of 1023 elements differ'):
        tg.check_bits(wrong, want, 'dst')


def test_a_mask_index_shifted_by_one_fails_the_attention_comparison():
    nb, nq, p, seed = 1, 33, 0.1, 99
    q, k, v = tg.data('rand', 1, nq, 256), tg.data('rand', 2, 512, 256), tg.data('rand', 3, 512, 256)
    (o, so), _ = ko.attention_fwd(q, k, v, nb, nq, tg.QSCALE, p, seed)
    o32, _ = ko.attention_fwd_f32(q, k, v, nb, nq, tg.QSCALE, p, seed)
    saved = dict(tg.WORST)                                                                 # (the record of a session's real comparisons)
    try:
        tg.check_yard(o32, o, so, 'attention_fwd.o', 'o')
        (shifted, _), _ = ko.attention_fwd(q, k, v, nb, nq, tg.QSCALE, p, seed, mask_shift=1)
        with pytest.raises(AssertionError, match='attention_fwd.o'):
            tg.check_yard(shifted.astype(F32), o, so, 'attention_fwd.o', 'o')
    finally:
        tg.WORST.clear()
        tg.WORST.update(saved)
