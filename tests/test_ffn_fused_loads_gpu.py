"""ffn_fused_kernel (csrc/ffn.hip) pinned to the bits it produces today, for the next change that moves its loads or waits without touching
its arithmetic (the first such attempt - W2 / b1 requested in front of phase 1, the next W1 sub-chunk in flight across phase 2 - kept
these bits and gained nothing: docs/LABNOTES.md 4b).  cotr_op_ffn_block must give the recorded sha256 (tests/golden/ffn_fused_sha.json,
tests/golden/make_load_order_fixtures.py) at every copy of the sub-chunk loop body (1, 2, 4 and 8 sub-chunks per workgroup: knob
ffn_fused_max_chunks), at the partial row tile and at the one-pair row counts; and it is the block of transformer.py:156-158 (fp64, the
bound of test_ops_gpu.test_fused_ffn_block).  A wrong counted wait reads an operand before it has landed: wrong bits, not a fault - which
is what the hashes are for."""
import json
import os

import pytest
import torch

from tests import gpu_helpers as G
from tests import load_order_cases as C

pytestmark = pytest.mark.gpu


def _fixture():
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'ffn_fused_sha.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('max_chunks', C.FFN_CHUNKS)
@pytest.mark.parametrize('M', C.FFN_ROWS)
def test_ffn_fused_bits_and_fp64(M, max_chunks):
    y, nch = C.ffn_run(M, max_chunks)
    want = _fixture()[f'M{M} max_chunks{max_chunks}']
    assert nch == want['nch']
    if M == 33:
        assert 1024 // nch // 64 == {2: 8, 4: 4, 8: 2, 16: 1}[max_chunks]   # sub-chunks per workgroup: every copy of the body
    assert torch.isnan(y[M]).all()                                          # the guard row
    ref = C.ffn_reference(M)
    finite = torch.ones(M, dtype=torch.bool)
    if M > C.FFN_NAN_ROW:
        finite[C.FFN_NAN_ROW] = False
        assert torch.isnan(y[C.FFN_NAN_ROW]).all()
    assert torch.isfinite(y[:M][finite.to(y.device)]).all()                  # the NaN row stays in its row
    e = G.rel_err(y[:M][finite.to(y.device)], ref[finite])
    print(f'M {M} max_chunks {max_chunks}: {nch} chunks, rel err against fp64 {e:.3g}')
    assert e < 2e-5, e
    assert C.sha(y) == want['sha256']
