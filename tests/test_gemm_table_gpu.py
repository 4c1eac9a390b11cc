"""Every launch of a forward - each GEMM's shape and configuration, the dual launches, the ` dense` suffix - is the one recorded before
the launch configurations were described by rows (tests/golden/forward_launch_names.json, make_gemm_fixtures.py)."""
import json
import os

import pytest

from tests import gemm_table_cases as C

pytestmark = pytest.mark.gpu


def test_forward_launch_names_match_the_recorded_ones(golden_dir):
    with open(os.path.join(golden_dir, 'forward_launch_names.json')) as f:
        want = json.load(f)
    got = C.forward_launch_names()
    assert sorted(got) == sorted(want) == sorted(f'{b},{q}' for b, q in C.FORWARD_SHAPES)
    for key in want:
        assert len(want[key]) > 80
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(got[key], want[key])) if a != b]
        assert got[key] == want[key], (key, len(got[key]), len(want[key]), diff[:5])
    assert any('+conv1x1/1' in n for n in want['1,100']) and any(n.endswith(' dense') for n in want['8,100'])
