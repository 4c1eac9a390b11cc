"""How the library plans a call, pinned: cotr_scratch_bytes, cotr_workspace_bytes and the encode / decode passes of
cotr_batch_chunks over a grid of (pairs, queries) under the knob values that move them, against tests/golden/plan_sizes.json
(recorded on the MI355X by tests/golden/make_plan_golden.py).  The sizing and the pass walk are host code that the kernels'
bounds depend on: a change meant to keep behaviour keeps every number."""
import importlib.util
import json
import os

import pytest

from tests.test_parity_gpu import hip_model

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    'make_plan_golden', os.path.join(os.path.dirname(__file__), 'golden', 'make_plan_golden.py'))
make_plan_golden = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_plan_golden)


def test_plan_numbers_match_the_recorded_ones():
    with open(make_plan_golden.PATH) as f:
        want = json.load(f)
    assert sorted(want) == sorted(make_plan_golden.KNOB_SETS)
    m = hip_model()
    import torch
    m._ensure_ready(torch.device('cuda'))
    got = make_plan_golden.all_numbers(m._handle)
    for name in make_plan_golden.KNOB_SETS:
        diff = {shape: (got[name].get(shape), v) for shape, v in want[name].items() if got[name].get(shape) != v}
        assert not diff, f'{name}: {len(diff)} shapes differ (got, recorded), e.g. {dict(list(diff.items())[:3])}'
