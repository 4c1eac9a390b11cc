"""ffn_fused_pipe_kernel (csrc/ffn_pipe.hip): the few-rows fused FFN with phase 1 and phase 2 on separate wavefronts, overlapped across 32-unit
steps.  It runs ffn_fused_kernel's floating-point operations in ffn_fused_kernel's order, so cotr_op_ffn_block keeps the bits recorded on
the commit before it (tests/golden/ffn_pipeline_sha.json from tests/golden/make_ffn_pipeline_fixtures.py; tests/golden/ffn_fused_sha.json
for the row counts tests/test_ffn_fused_loads_gpu.py already pins).  What a pipeline can get wrong beyond a single launch's bits:
  * its edges - two and three row tiles with the last one full or nearly empty, at 2 steps (first and last adjacent), 4 steps, and 16
    steps (the three W1 stages and the W2 register ring wrap several times);
  * something stale or missing - a partial-slab element never written (scratch pre-filled with NaN), an LDS stage or Hs buffer read
    before this launch wrote it (the same call twice with another launch in between);
  * the knob forms - chunk-major workgroup order and plain stores are the same arithmetic."""
import json
import os

import pytest
import torch

from tests import ffn_pipeline_cases as FP
from tests import gpu_helpers as G
from tests import load_order_cases as C

pytestmark = pytest.mark.gpu


def _fixture(name):
    with open(os.path.join(os.path.dirname(__file__), 'golden', name)) as f:
        return json.load(f)


def _run(M, max_chunks, scratch_fill=None, xcd_mapping=None):
    """tests/load_order_cases.ffn_run with a chosen scratch content and knob -> y [M + 1][256] with the guard row"""
    from cotr_amd import _lib
    lib = _lib.load_library()
    _lib.set_knob('ffn_fused_max_chunks', max_chunks)
    if xcd_mapping is not None:
        _lib.set_knob('xcd_mapping', xcd_mapping)
    try:
        t = C.ffn_inputs_dev(M)
        nch = lib.cotr_op_ffn_chunks(M)
        scratch = torch.empty(nch * M * 256, device=G.dev())
        if scratch_fill is not None:
            scratch.fill_(scratch_fill)
        y = torch.full((M + 1, 256), float('nan'), device=G.dev())
        rc = lib.cotr_op_ffn_block(*[G.P(v) for v in t], G.P(scratch), G.P(y), M, G.sptr())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return y
    finally:
        _lib.reset_knobs()


@pytest.mark.parametrize('max_chunks', FP.EDGE_CHUNKS)
@pytest.mark.parametrize('M', FP.EDGE_ROWS)
def test_bits_at_the_pipeline_edges(M, max_chunks):
    y, nch = C.ffn_run(M, max_chunks)
    want = _fixture('ffn_pipeline_sha.json')[f'M{M} max_chunks{max_chunks}']
    assert nch == want['nch'] == max_chunks                                  # 1024 / nch / 32 = 2, 4, 16 steps
    assert torch.isnan(y[M]).all()                                           # the guard row
    assert torch.isnan(y[C.FFN_NAN_ROW]).all()
    finite = torch.ones(M, dtype=torch.bool)
    finite[C.FFN_NAN_ROW] = False
    assert torch.isfinite(y[:M][finite.to(y.device)]).all()                  # the NaN row stays in its row
    e = G.rel_err(y[:M][finite.to(y.device)], C.ffn_reference(M)[finite])
    print(f'M {M} max_chunks {max_chunks}: {nch} chunks, rel err against fp64 {e:.3g}')
    assert e < 2e-5, e                                                       # the bound of test_ops_gpu.test_fused_ffn_block
    assert C.sha(y) == want['sha256']


@pytest.mark.parametrize('max_chunks', [16, 2])
def test_nothing_stale_nothing_missing(max_chunks):
    want = _fixture('ffn_fused_sha.json')[f'M33 max_chunks{max_chunks}']['sha256']
    assert C.sha(_run(33, max_chunks, scratch_fill=float('nan'))) == want    # every element of every partial slab is written
    first = C.sha(C.ffn_run(33, max_chunks)[0])
    other = C.sha(C.ffn_run(1000, max_chunks)[0])                            # leaves its own X, W1 stages and H in the CUs' LDS
    again = C.sha(C.ffn_run(33, max_chunks)[0])
    assert first == again == want
    assert other == _fixture('ffn_fused_sha.json')[f'M1000 max_chunks{max_chunks}']['sha256']


@pytest.mark.parametrize('xcd_mapping', [1 | 4, 1 | 16], ids=['chunk_major', 'plain_stores'])
def test_knob_forms(xcd_mapping):
    want = _fixture('ffn_fused_sha.json')['M1000 max_chunks16']
    assert want['nch'] == 8
    assert C.sha(_run(1000, 16, xcd_mapping=xcd_mapping)) == want['sha256']
