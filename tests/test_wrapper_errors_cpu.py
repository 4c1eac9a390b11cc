"""What the geometry wrappers under cotr_amd/inference/ refuse, in which order and in which words, and which library calls
their chained functions make, against tests/golden/wrapper_errors.json: the table recorded on the commit before their argument
rules moved into inference/_args.py (tests/golden/make_wrapper_errors.py; the calls are tests/wrapper_error_cases.py).  The
type and the text of every exception are compared exactly.  No GPU and no built library: every check here runs before a device
is picked, and the call logs run on the CPU with a recorder in the library's place."""
import json
import os

import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import _args
from tests import wrapper_error_cases as C

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wrapper_errors.json')) as f:
    GOLDEN = json.load(f)
CASES = C.cases()


def test_the_table_and_the_cases_are_the_same_rows():
    assert [row[:2] for row in GOLDEN['errors']] == [list(c[:2]) for c in CASES]
    assert len({tuple(row[:2]) for row in GOLDEN['errors']}) == len(CASES)
    assert list(GOLDEN['calls']) == list(C.sequences())


def test_no_row_got_as_far_as_the_library():
    # a check behind load_library() is not an argument check: the generator would have recorded reached_library's AssertionError
    assert all(row[2] in ('ValueError', 'CotrHipError', 'DeviceReached', 'returned') for row in GOLDEN['errors'])


@pytest.mark.parametrize('case, row', list(zip(CASES, GOLDEN['errors'])), ids=[f'{c[0]}-{c[1]}' for c in CASES])
def test_every_call_raises_what_it_raised_before(case, row, monkeypatch):
    monkeypatch.setattr(_args, 'device', C.reached_device)
    monkeypatch.setattr(_lib, 'load_library', C.reached_library)
    path, cid, base, over = case
    assert C.outcome(path, base, over) == row[2:], (path, cid)


@pytest.mark.parametrize('name', list(GOLDEN['calls']))
def test_chained_calls_make_the_same_library_calls_with_the_same_scalars(name, monkeypatch):
    monkeypatch.setattr(_args, 'device', lambda device=None: torch.device('cpu'))
    monkeypatch.setattr(_args, 'no_cpu_tensors', lambda subject, *xs: None)   # (the chained tensors are CPU tensors here)
    rec = C.Recorder()
    C.cpu_patches(monkeypatch.setattr, rec)
    C.sequences()[name]()
    assert json.loads(json.dumps(rec.log)) == GOLDEN['calls'][name]
