"""The epilogues of gemm_wp_body (csrc/gemm_wp.hip) and gemm_ks_body (csrc/gemm.hip) after their scale / bias / residual requests moved
in front of the K loop: the arithmetic and its order are unchanged, so every configuration must give the bits it gave before - the
sha256 recorded on the commit before the change (tests/golden/gemm_epilogue_sha.json, tests/golden/make_load_order_fixtures.py) - with
every combination of the epilogue operands the op-level entries take, at one row, at a ragged last tile (rows past M read a clamped row
and store nothing: the guard row behind the output is hashed with it) and at the one-pair query count, for a short and a long
contraction, and on a 3x3 and a strided 1x1 convolution of a 16 x 32 pair.  A configuration that refuses a case is recorded as
refusing."""
import json
import os

import pytest

from tests import load_order_cases as C

pytestmark = pytest.mark.gpu


def _fixture():
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'gemm_epilogue_sha.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('cfg', C.GEMM_CFGS)
def test_gemm_epilogue_bits(cfg):
    want = _fixture()[str(cfg)]
    got = C.gemm_run(cfg)
    assert sorted(got) == sorted(want)
    ran = [k for k, v in got.items() if v != 'refused']
    print(f'cfg {cfg}: {len(ran)} of {len(got)} cases ran')
    assert ran, 'the configuration took no case at all'
    wrong = [k for k in got if got[k] != want[k]]
    assert not wrong, wrong
