"""Every kernel of the training step (the ``cotr_train_*`` entry points of include/cotr_hip.h) through the raw C ABI inside a guarded
arena (tests/guard_arena.py), at the shapes of tests/train_guard_cases.py: ``part``, ``scratch`` and ``delta`` of exactly the size
the query or the header gives, every buffer between two 64 KiB bands of a fill byte at the least alignment the header documents
(16 bytes where a kernel loads float4, 4 where it accesses by scalar).

Each case runs three times, with the fill 0x00, 0xA5 and 0xFF, from fresh arenas - a case of a sum of products once with integer
data and once with random data - and asserts
1. the return code is 0, or the documented count of partials for the ``*_parts`` calls; no band byte and no input changed;
2. the outputs are the float64 restatement's (tests/train_kernel_oracle.py) element by element: bit for bit for a move, exactly on
   integer data and within the any-order bound on random data for a sum of products, within 8 times the float32 yardstick for
   everything with a rsqrt, exp2 or division; every element the op must not write holds the fill;
3. the three runs wrote the same bytes: a read of ``part``, ``scratch``, ``delta``, of an output or of a query row past ``nq`` that
   reaches a result shows here.

The refusals return COTR_ERR_ARG and the empty calls 0, each with every output still the fill.  One control per op with a ``part`` or
``scratch`` moves that buffer's rear band into the buffer at the case where its last partial is written in full, and the check must
say so.  The knob a case sets is put back in ``finally``; no case registers a dropout salt."""
import json

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from tests import train_guard_cases as tg
from tests.guard_arena import GuardError
from tests.scratch_guard_cases import place, read_outputs, same_written_bytes

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xA5, 0xFF)
ERR_HIP = -2
CASES = tg.all_cases()
SPECIAL = tg.special_calls()
EARLY = [r for r in tg.ROWS if r.early is not None]


def enqueue(name, call, fill, early_outputs=None):
    """one call from a fresh arena -> (return value, arena, the outputs' (dtype, shape)), synchronized"""
    lib = _lib.load_library()
    arena, argv, outs = place(call, 0, 'cuda', fill, early_outputs=early_outputs)
    for buf, array in (call.init or {}).items():
        arena.raw(buf).copy_(torch.from_numpy(np.ascontiguousarray(array).reshape(-1).view(np.uint8)))
    saved = {k: _lib.knobs()[k][0] for k in (call.knobs or {})}
    try:
        for k, v in (call.knobs or {}).items():
            _lib.set_knob(k, v)
        try:
            torch.cuda.synchronize()
            rc = getattr(lib, name)(*argv)
            torch.cuda.synchronize()
        except RuntimeError as e:              # a device error is not one failed case: nothing more is started on this GPU
            pytest.exit(f'{name}: the device reported an error, the session ends here: {e}', returncode=3)
        if rc == ERR_HIP:
            pytest.exit(f'{name}: COTR_ERR_HIP ({lib.cotr_raster_last_error()}), the session ends here', returncode=3)
    finally:
        for k, v in saved.items():
            _lib.set_knob(k, v)
    return rc, arena, outs


def run(name, call, fill):
    """a clean run: the expected return value and the arena intact -> the outputs as host arrays"""
    rc, arena, outs = enqueue(name, call, fill)
    assert rc == call.rc, (rc, call.rc, _lib.load_library().cotr_raster_last_error())
    arena.check()
    return read_outputs(arena, outs)


def three_fills(name, call):
    twin = run(call.twin[0], call.twin[1], 0xA5) if call.twin is not None else None
    first = None
    for fill in FILLS:
        outs = run(name, call, fill)
        if twin is not None:
            call.expect(outs, fill, twin)
        else:
            call.expect(outs, fill)
        if first is None:
            first = (fill, outs)
        else:
            for buf in outs:
                same_written_bytes(first[1][buf], first[0], outs[buf], fill, buf)


@pytest.mark.parametrize('rcm', CASES, ids=lambda rcm: f'{rcm[0].name[11:]}-{rcm[1].id}-{rcm[2]}')
def test_inside_its_buffers_and_equal_to_the_restatement(rcm):
    row, case, mode = rcm
    three_fills(row.name, row.build(case.params, mode))


@pytest.mark.parametrize('special', SPECIAL, ids=lambda s: s[0])
def test_refusals_and_empty_calls_write_nothing(special):
    _, name, call = special
    three_fills(name, call)


@pytest.mark.parametrize('row', EARLY, ids=lambda r: r.name[11:])
def test_early_band_control(row):
    """the rear band of ``part`` / ``scratch`` starts 16 bytes before the buffer ends: the op's own kernel writes there, and the check says so"""
    case_id, buf = row.early
    case = next(c for c in row.cases if c.id == case_id)
    call = row.build(case.params, 'rand')
    rc, arena, _ = enqueue(row.name, call, 0xA5, early_outputs={buf: 16})
    assert rc == call.rc, _lib.load_library().cotr_raster_last_error()
    with pytest.raises(GuardError, match=rf"rear band of '{buf}'.*offsets -\d+ \.\. -\d+ from the buffer's end"):
        arena.check()


def test_zz_the_kernels_worst_ratios_are_inside_the_bounds(capsys):
    """runs last in this file: the worst per-element ratio of every yardstick output over the cases above, printed for the record"""
    with capsys.disabled():
        print('\ntrain guard: kernel worst ratios ' + json.dumps({k: float(f'{v:.3g}') for k, v in sorted(tg.WORST.items())}))
    for key, worst in tg.WORST.items():
        assert worst <= tg.bound(key), (key, worst, tg.bound(key))
