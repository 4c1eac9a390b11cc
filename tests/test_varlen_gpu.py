"""Varlen decode (cotr_decode_varlen / cotr_forward_varlen, model.forward_varlen / decode_varlen): B pairs with a different number
of queries each, packed [N, 2], against the CPU oracle run per pair on that pair's own queries, against the zero-padded uniform
call, and through FasterSparseEngine(varlen=True)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cotr_amd
from cotr_amd import _lib
from cotr_amd.inference import FasterSparseEngine
from cotr_amd.models import build_model
from cotr_amd.utils.synth import synth_state_dict, synth_inputs
from oracle import cotr_oracle
from tests import gpu_helpers as G
from tests import raw_abi
from tests.engine_fixtures import ids, synthetic_pair

pytestmark = pytest.mark.gpu

PX_BAR = 1e-3
SHAPE_NOISE_PX = 3e-4  # same math, different fp32 summation order between launch configurations

_models = {}


def hip_model():
    if 'm' not in _models:
        m = build_model(cotr_amd.default_args()).cuda().eval()
        m.load_state_dict(synth_state_dict(0))
        _models['m'] = m
    return _models['m']


def inputs(counts, seed):
    """img [B,3,256,512] (every pair its own image), packed queries [N,2] and the per-pair split of them."""
    img, _ = synth_inputs(len(counts), 1, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    q = torch.from_numpy(rng.random((int(sum(counts)), 2)).astype(np.float32))
    return img, q


def oracle_varlen(img, q, counts):
    """The oracle per pair: encode (in chunks of pairs), then each pair's decode on its own queries only."""
    sd = synth_state_dict(0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    out = torch.zeros(q.shape[0], 2)
    ends = np.cumsum(counts)
    with torch.no_grad():
        for c0 in range(0, len(counts), 8):
            idx = [b for b in range(c0, min(c0 + 8, len(counts))) if counts[b] > 0]
            if not idx:
                continue
            enc = cotr_oracle.cotr_encode(sd, img[idx])
            for k, b in enumerate(idx):
                rows = slice(int(ends[b] - counts[b]), int(ends[b]))
                out[rows] = cotr_oracle.cotr_decode(sd, enc['memory'][:, k:k + 1], enc['pos'][:, k:k + 1], q[rows][None])['pred_corrs'][0]
    return out


def random_counts(n, hi, seed):
    return [int(c) for c in np.random.Generator(np.random.PCG64(seed)).integers(1, hi + 1, n)]


PATTERNS = {
    'squads_257_31x8': [257] + [8] * 31,
    'empty_pair': [0, 5, 1000, 3],
    'one_each_32': [1] * 32,
    'one_pair_two_passes': [40000],
    'random_17x1200': random_counts(17, 1200, 7),
    'random_70': random_counts(70, 600, 8),
}


@pytest.mark.parametrize('name', list(PATTERNS))
def test_varlen_matches_the_oracle_per_pair(name):
    counts = PATTERNS[name]
    img, q = inputs(counts, seed=300 + len(counts))
    m = hip_model()
    out = m.forward_varlen(img.cuda(), q.cuda(), counts).cpu()
    assert out.shape == (sum(counts), 2) and torch.isfinite(out).all()
    ref = oracle_varlen(img, q, counts)
    ends = np.cumsum(counts)
    for b, c in enumerate(counts):
        if c:
            rows = slice(int(ends[b] - c), int(ends[b]))
            assert cotr_oracle.px_err(out[rows], ref[rows]) < PX_BAR, (name, b, c)


# each decoder attention form with a varlen mode, forced through the per-model knobs; the profile names say which one ran
FORMS = {
    'fused': (dict(), 'qproj+attention+oproj dec s4 vl'),
    'fused_s8': (dict(attention_fused_splits=8), 'qproj+attention+oproj dec s8 vl'),
    'rows': (dict(attention_fusion_max_rows=0, att_rows_min_rows=0, rows_min_fill=0), 'att_rows dec'),
    'plain': (dict(attention_fusion_max_rows=0, att_rows_min_rows=1 << 30), 'attention dec s4 vl'),
    'plain_s2': (dict(attention_fusion_max_rows=0, att_rows_min_rows=1 << 30, attention_splits=2), 'attention dec s2 vl'),
}


@pytest.mark.parametrize('form', list(FORMS))
def test_every_varlen_attention_form_matches_the_oracle(form):
    knobs, launch = FORMS[form]
    counts = [64, 0, 128, 192, 63, 1]        # 448 rows in 8 tiles of 64: the rows form's 7/8 fill rule holds once it is allowed
    img, q = inputs(counts, seed=41)
    m = hip_model()
    with G.model_knobs(m, **knobs):
        m.set_profiling(2)
        try:
            out = m.forward_varlen(img.cuda(), q.cuda(), counts).cpu()
            names = m.profile_names()
        finally:
            m.set_profiling(0)
    assert any(n.startswith(launch) for n in names), (form, sorted(set(names)))
    assert cotr_oracle.px_err(out, oracle_varlen(img, q, counts)) < PX_BAR, form


def test_varlen_matches_the_zero_padded_call():
    counts = [257] + [8] * 31
    img, q = inputs(counts, seed=51)
    m = hip_model()
    out = m.forward_varlen(img.cuda(), q.cuda(), counts).cpu()
    pad = torch.zeros(len(counts), max(counts), 2)
    ends = np.cumsum(counts)
    for b, c in enumerate(counts):
        pad[b, :c] = q[ends[b] - c:ends[b]]
    padded = m(img.cuda(), pad.cuda())['pred_corrs'].cpu()
    real = torch.cat([padded[b, :c] for b, c in enumerate(counts)])
    assert cotr_oracle.px_err(out, real) < SHAPE_NOISE_PX
    # uniform counts: varlen == the uniform call
    img4, q4 = synth_inputs(4, 300, seed=52)
    uni = m(img4.cuda(), q4.cuda())['pred_corrs'].cpu()
    vl = m.forward_varlen(img4.cuda(), q4.reshape(-1, 2).cuda(), [300] * 4).cpu()
    assert cotr_oracle.px_err(vl.reshape(4, 300, 2), uni) < SHAPE_NOISE_PX


def test_varlen_is_repeatable():
    counts = random_counts(9, 900, 53)
    img, q = inputs(counts, seed=53)
    m = hip_model()
    a = m.forward_varlen(img.cuda(), q.cuda(), counts)
    b = m.forward_varlen(img.cuda(), q.cuda(), counts)
    assert torch.equal(a, b)


def test_decode_varlen_against_one_cached_encode():
    """encode once; decode_varlen twice with different counts; then the uniform decode: all against the oracle."""
    m = hip_model()
    img, q = synth_inputs(3, 40, seed=54)
    m.encode(img.cuda())
    c1, c2 = [40, 0, 17], [5, 40, 40]
    q1 = torch.cat([q[b, :c] for b, c in enumerate(c1)])
    q2 = torch.cat([q[b, :c] for b, c in enumerate(c2)])
    o1 = m.decode_varlen(q1.cuda(), c1).cpu()
    o2 = m.decode_varlen(q2.cuda(), c2).cpu()
    o3 = m.decode(q.cuda()).cpu()
    ref = cotr_oracle.cotr_forward(synth_state_dict(0), img, q)
    assert cotr_oracle.px_err(o3, ref) < PX_BAR
    assert cotr_oracle.px_err(o1, torch.cat([ref[b, :c] for b, c in enumerate(c1)])) < PX_BAR
    assert cotr_oracle.px_err(o2, torch.cat([ref[b, :c] for b, c in enumerate(c2)])) < PX_BAR


def test_back_to_back_varlen_calls_with_different_offsets():
    """Six varlen calls with different offsets enqueued with no host synchronisation in between (more than the handle's staging
    ring of 4 slots; each offsets array is gone once its call returns): every one is right."""
    m = hip_model()
    img, q = synth_inputs(4, 300, seed=55)
    m.encode(img.cuda())
    qd = q.cuda()
    patterns = [[300, 1, 0, 77], [3, 300, 300, 2], [0, 0, 0, 9], [120, 120, 120, 120], [1, 2, 3, 4], [299, 0, 150, 300]]
    outs = []
    for counts in patterns:
        packed = torch.cat([qd[b, :c] for b, c in enumerate(counts)])
        outs.append(m.decode_varlen(packed, list(counts)))
    torch.cuda.synchronize()
    ref = cotr_oracle.cotr_forward(synth_state_dict(0), img, q)
    for counts, o in zip(patterns, outs):
        want = torch.cat([ref[b, :c] for b, c in enumerate(counts)])
        assert cotr_oracle.px_err(o.cpu(), want) < PX_BAR, counts


def test_caller_workspace_from_cotr_scratch_bytes_varlen():
    """A workspace of exactly cotr_scratch_bytes_varlen bytes serves the call: the library never allocates with a workspace set (a
    region that does not fit is a 'workspace too small' error instead), so success is the proof."""
    lib = _lib.load_library()
    m = build_model(cotr_amd.default_args()).cuda().eval()
    m.load_state_dict(synth_state_dict(0))
    counts = [257] + [8] * 31
    img, q = inputs(counts, seed=56)
    ref = m.forward_varlen(img.cuda(), q.cuda(), counts)       # the binding's own workspace
    offsets = (ctypes.c_int * (len(counts) + 1))(*np.concatenate([[0], np.cumsum(counts)]).tolist())
    out = torch.empty(sum(counts), 2, device='cuda')
    imgd, qd = img.cuda(), q.cuda()
    with raw_abi.caller_workspace(m, raw_abi.scratch_bytes_varlen(m, offsets)):
        rc = lib.cotr_forward_varlen(m._handle, imgd.data_ptr(), qd.data_ptr(), offsets, len(counts), out.data_ptr(),
                                     _lib.current_stream_ptr())
        assert rc == 0, lib.cotr_last_error(m._handle)
        assert torch.equal(out, ref)
        # and the varlen decode against that encode, same workspace
        rc = lib.cotr_decode_varlen(m._handle, qd.data_ptr(), offsets, len(counts), out.data_ptr(), _lib.current_stream_ptr())
        assert rc == 0 and torch.equal(out, ref)
        assert raw_abi.set_workspace(m, None, 0) == 0


def test_malformed_offsets_on_a_real_handle():
    lib = _lib.load_library()
    m = hip_model()
    img, q = synth_inputs(2, 8, seed=57)
    m.encode(img.cuda())
    qd = q.reshape(-1, 2).cuda()
    out = torch.empty(16, 2, device='cuda')
    s = _lib.current_stream_ptr()
    cases = [([1, 8, 16], 2, b'offsets[0]'), ([0, 9, 8], 2, b'decrease'), ([0, 8, 16], 0, b'B <= 0'), ([0, 8, 16], -1, b'B <= 0')]
    for offs, b, msg in cases:
        arr = (ctypes.c_int * 3)(*offs)
        assert lib.cotr_decode_varlen(m._handle, qd.data_ptr(), arr, b, out.data_ptr(), s) == -1, (offs, b)
        assert msg in lib.cotr_last_error(m._handle), (offs, b, lib.cotr_last_error(m._handle))
        assert lib.cotr_forward_varlen(m._handle, img.cuda().data_ptr(), qd.data_ptr(), arr, b, out.data_ptr(), s) == -1
    arr = (ctypes.c_int * 4)(0, 8, 16, 16)
    assert lib.cotr_decode_varlen(m._handle, qd.data_ptr(), arr, 3, out.data_ptr(), s) == -3     # COTR_ERR_STATE: the cache holds 2 pairs
    assert b'no cached encode' in lib.cotr_last_error(m._handle)
    arr = (ctypes.c_int * 3)(0, 8, 16)
    assert lib.cotr_decode_varlen(m._handle, None, arr, 2, out.data_ptr(), s) == -1
    assert lib.cotr_decode_varlen(m._handle, qd.data_ptr(), arr, 2, out.data_ptr(), s) == 0


def _run_faster_engine(golden_dir, model, varlen):
    g = np.load(os.path.join(golden_dir, 'e2e_faster_known.npz'))
    seed, nq, conv, cycle, bs, load = (int(v) for v in g['meta'])
    img_a, img_b = synthetic_pair(seed)
    eng = FasterSparseEngine(model, bs, mode='tile', max_load=load, varlen=varlen)
    np.random.seed(seed)
    corrs, idx = eng.cotr_corr_multiscale(img_a, img_b, np.linspace(0.5, 0.0625, 4), conv, max_corrs=nq,
                                          queries_a=g['queries'].copy(), return_idx=True, force=True, areas=[1.0, 1.0])
    return g, np.asarray(corrs, dtype=np.float64).reshape(-1, 4), ids(idx), eng.decoded_rows


def test_faster_sparse_engine_varlen_reproduces_the_reference_engine(golden_dir):
    model = hip_model()
    g, corrs, idx, rows_vl = _run_faster_engine(golden_dir, model, varlen=True)
    assert np.array_equal(idx, g['idx'])
    assert np.array_equal(corrs[:, :2], g['corrs'][:, :2])
    err = np.abs(corrs[:, 2:] - g['corrs'][:, 2:]).max()
    assert err < 0.02, f'{err:.3e} px from the reference engine'
    _, _, _, rows_pad = _run_faster_engine(golden_dir, model, varlen=False)
    assert 0 < rows_vl <= rows_pad, (rows_vl, rows_pad)        # (this golden's squads are all of one task: nothing to save)


def test_faster_sparse_engine_grouped_call_decodes_only_the_real_rows():
    """A grouped call with squads of 6, 1, 3 and 1 tasks: the padded call decodes 4 x 6 rows, the varlen call 11 - and the real
    rows agree."""
    model = hip_model()
    img_a, img_b = synthetic_pair(3)
    eng = FasterSparseEngine(model, 8, mode='tile', max_load=6, varlen=True)
    cropper = eng.make_cropper(img_a, img_b, torch.device('cuda'))
    boxes = np.array([[10, 20, 200, 30, 40, 250], [100, 50, 180, 60, 80, 200], [0, 0, 256, 0, 0, 300], [200, 90, 150, 120, 100, 160]],
                     dtype=np.int32)
    counts = [6, 1, 3, 1]
    rng = np.random.default_rng(5)
    queries = np.zeros((4, 6, 2), dtype=np.float32)
    for k, c in enumerate(counts):
        queries[k, :c] = rng.random((c, 2))
    vl = eng._forward_varlen(cropper, boxes, queries, counts, torch.device('cuda'))
    assert eng.decoded_rows == 11
    pad = eng._forward(cropper, boxes, queries, torch.device('cuda'), count=False)
    assert eng.decoded_rows == 11 + 24
    for k, c in enumerate(counts):
        assert cotr_oracle.px_err(torch.from_numpy(vl[k, :c]), torch.from_numpy(pad[k, :c])) < SHAPE_NOISE_PX, k
        assert not vl[k, c:].any()
