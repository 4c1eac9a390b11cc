"""The refit frame (cotr_amd/csrc/refit.h) carries the Gauss-Newton refits of cotr_ransac_homography, cotr_ransac_pnp and
cotr_refine_pose with their arithmetic in their order, so every array these calls return keeps the bits of the commit before
the frame: tests/golden/refit_frame_sha.json, recorded there by tests/golden/make_refit_frame_fixtures.py over the calls of
tests/refit_frame_cases.py."""
import json
import os

import pytest

from tests import refit_frame_cases as C

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(__file__), 'golden', 'refit_frame_sha.json')) as _f:
    WANT = json.load(_f)


def test_the_fixture_holds_the_case_list():
    assert sorted(WANT) == sorted(C.CASES)


@pytest.mark.parametrize('name', list(C.CASES))
def test_same_bits_as_before_the_frame(name):
    got, want = C.hashes(name), WANT[name]
    assert sorted(got) == sorted(want)
    differ = [k for k in got if got[k] != want[k]]
    assert not differ, f'{name}: {differ[0]} differs from the recorded bits (all that differ: {differ})'
