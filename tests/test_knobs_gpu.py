"""Every value of every forward tuning knob against the oracle (a knob changes which kernels run, never the
contract).  The table is tests/knob_cases.py; each (knob, value, shape) runs on ONE cached model object (the workspace is re-carved as
knobs change, cotr_model.py _Workspace.stale) and is checked for: finite and bit-repeatable output; every pair within SHAPE_NOISE_PX of the
default-knob output (bit for bit where the table says 'same'); three pairs within PX_BAR of the CPU oracle; and reach - the per-launch
profile (cotr_set_profiling 2) shows the value took its branch at that shape.  A case that does not reach its branch fails.
Then the interactions the dispatch code shows to matter.  Everything runs eagerly (no graph capture: a captured side stream is a
graph with parallel branches)."""
import re

import pytest
import torch

from cotr_amd import _lib
from cotr_amd.utils.synth import synth_state_dict, synth_inputs
from oracle import cotr_oracle
from tests import gpu_helpers as G
from tests import raw_abi
from tests.knob_cases import KNOB_CASES, case_runs
from tests.test_parity_gpu import PX_BAR, SHAPE_NOISE_PX, hip_model

pytestmark = pytest.mark.gpu

_inputs, _oracle, _default, _names = {}, {}, {}, {}
_sized_checked = set()


def inputs(b, q):
    if (b, q) not in _inputs:
        _inputs[(b, q)] = synth_inputs(b, q, seed=700 + b)
    return _inputs[(b, q)]


def pick(b):
    return sorted({0, b // 2, b - 1})


def oracle(b, q, idx):
    key = (b, q, tuple(idx))
    if key not in _oracle:
        img, qs = inputs(b, q)
        _oracle[key] = cotr_oracle.cotr_forward(synth_state_dict(0), img[idx], qs[idx])
    return _oracle[key]


def forward(m, b, q):
    img, qs = inputs(b, q)
    return m(img.cuda(), qs.cuda())['pred_corrs'].cpu()


def launch_names(m, b, q):
    """per-launch names of one forward (kernel, variant, GEMM shape and configuration)"""
    m.set_profiling(2)
    try:
        forward(m, b, q)
        torch.cuda.synchronize()
        return m.profile_names()
    finally:
        m.set_profiling(0)


def default_out(m, b, q):
    if (b, q) not in _default:
        _default[(b, q)] = forward(m, b, q)
    return _default[(b, q)]


def base_names(m, b, q, base):
    key = (b, q, tuple(sorted(base.items())))
    if key not in _names:
        with G.model_knobs(m, **base):
            _names[key] = launch_names(m, b, q)
    return _names[key]


def raw_forward_in_sized_workspace(m, b, q):
    """cotr_forward on a caller workspace of exactly cotr_scratch_bytes(h, B, Q) bytes, 256-aligned, under the handle's current knobs
    (cotr_scratch_bytes: "a knob never makes a sized workspace too small").  The model's own workspace is dropped afterwards."""
    lib = _lib.load_library()
    img, qs = inputs(b, q)
    img, qs = img.cuda().contiguous(), qs.cuda().contiguous()
    out = torch.empty(b, q, 2, device='cuda')
    with raw_abi.caller_workspace(m, raw_abi.scratch_bytes(m, b, q)):
        rc = lib.cotr_forward(m._handle, img.data_ptr(), qs.data_ptr(), b, q, out.data_ptr(), _lib.current_stream_ptr())
        assert rc == 0, lib.cotr_last_error(m._handle)
    return out.cpu()


def _ids():
    return [f'{k}={v}@{s[0]}x{s[1]}' for k, v, s, _, _ in case_runs()]


@pytest.mark.parametrize('knob,value,shape,reach,base', list(case_runs()), ids=_ids())
def test_knob_value_against_the_oracle(knob, value, shape, reach, base):
    b, q = shape
    m = hip_model()
    ref = default_out(m, b, q)
    ref_names = base_names(m, b, q, base)
    with G.model_knobs(m, **base, **{knob: value}):
        out = forward(m, b, q)
        assert torch.isfinite(out).all()
        assert torch.equal(out, forward(m, b, q)), 'not bit-repeatable'
        if (knob, value) not in _sized_checked:
            _sized_checked.add((knob, value))
            assert torch.equal(raw_forward_in_sized_workspace(m, b, q), out), 'another result in a workspace of cotr_scratch_bytes'
        if reach == 'side':
            chunk = m.knobs()['encode_chunk'][0]
            assert b <= chunk and b * q <= 8192 and m.batch_chunks(b, q, 0) == [b] and m.batch_chunks(b, q, 1) == [b], \
                'the side stream is not eligible at this shape (api.hip forward_impl)'
        else:
            names = launch_names(m, b, q)
            if reach == 'changes':
                assert names != ref_names, f'{knob}={value} does not change the launches at {b}x{q}'
            elif reach == 'default':
                assert names == ref_names, sorted(set(names) ^ set(ref_names))[:8]
            else:
                kind, pattern = reach
                assert kind == 'has'
                assert any(re.search(pattern, n) for n in names), f'no launch matching {pattern!r} at {b}x{q}'
    if KNOB_CASES[knob]['bits'] == 'same':
        assert torch.equal(out, ref), cotr_oracle.px_err(out, ref)
    err = cotr_oracle.px_err(out, ref)                  # every pair: a bug that touches only a later pass shows here
    assert err < SHAPE_NOISE_PX, err
    idx = pick(b)
    err = cotr_oracle.px_err(out[idx], oracle(b, q, idx))
    assert err < PX_BAR, err


# ---- interactions ------------------------------------------------------------------------------------------------------------------
ROWS_EVERYWHERE = dict(att_rows_min_rows=0, ffn_rows_min_rows=0, rows_min_fill=0)


def split_decode_shape(m):
    """A call whose decode is cut into passes while its encode is not, with B * Q <= 8192 (the side stream's row limit), under the rows
    kernels' lowest thresholds - found from the handle's own pass lists (the fill rules read the CU count); existing shapes first."""
    with G.model_knobs(m, **ROWS_EVERYWHERE):
        for b, q in [(8, 512), (3, 333), (24, 100), (16, 512), (4, 1000)] + [(b, 512) for b in range(2, 17)]:
            if b * q <= 8192 and m.batch_chunks(b, q, 0) == [b] and len(m.batch_chunks(b, q, 1)) > 1:
                return b, q
    return None


@pytest.mark.parametrize('side', [1, 2, 3])
def test_side_stream_on_a_call_whose_decode_splits(side):
    """side_stream applies to one decode pass only (include/cotr_hip.h): its query encoding is written once for all B x Q rows.  A call
    whose decode walks several passes must run without it - every pair against the oracle, not a sample (pair 7 of 8 x 512 used to be
    decoded with pair 0's query encodings)."""
    m = hip_model()
    shape = split_decode_shape(m)
    assert shape is not None, 'no shape with one encode pass and several decode passes under the rows kernels\' lowest thresholds'
    b, q = shape
    with G.model_knobs(m, **ROWS_EVERYWHERE):
        plain = forward(m, b, q)
    with G.model_knobs(m, **ROWS_EVERYWHERE, side_stream=side):
        out = forward(m, b, q)
        assert torch.equal(out, forward(m, b, q))
    idx = list(range(b))
    assert cotr_oracle.px_err(out, oracle(b, q, idx)) < PX_BAR, [cotr_oracle.px_err(out[i:i + 1], oracle(b, q, idx)[i:i + 1]) for i in idx]
    assert cotr_oracle.px_err(out, plain) < SHAPE_NOISE_PX


def test_side_stream_kv_without_the_pos_table():
    """side_stream bit 1 with pos_table_min_rows = 1 << 30: the K/V projection stays on the chain (no table), and decoder layer 1 must
    not wait on an event this call never recorded."""
    m = hip_model()
    b, q = 1, 1000
    ref = default_out(m, b, q)
    with G.model_knobs(m, side_stream=2, pos_table_min_rows=1 << 30):
        out = forward(m, b, q)
        assert torch.equal(out, forward(m, b, q))
    assert cotr_oracle.px_err(out, ref) < SHAPE_NOISE_PX
    assert cotr_oracle.px_err(out, oracle(b, q, [0])) < PX_BAR


@pytest.mark.parametrize('batch_split', [0, 1])
@pytest.mark.parametrize('b', [17, 29])
def test_odd_encode_chunk_across_the_conv23m_gap(b, batch_split):
    """encode_chunk 7: passes of 7 + 7 + 3 (17 pairs) and 7 x 4 + 1 (29) - every pass below conv23m's 16 pairs, the last one small -
    with and without batch_split; every pair against the oracle."""
    m = hip_model()
    q = 40
    ref = default_out(m, b, q)
    with G.model_knobs(m, encode_chunk=7, batch_split=batch_split):
        enc = m.batch_chunks(b, q, 0)
        assert sum(enc) == b and max(enc) <= 7
        out = forward(m, b, q)
        assert torch.equal(out, forward(m, b, q))
    assert cotr_oracle.px_err(out, ref) < SHAPE_NOISE_PX
    assert cotr_oracle.px_err(out, oracle(b, q, list(range(b)))) < PX_BAR
