"""Every handle-less op that takes a scratch, through the raw C ABI inside a guarded arena (tests/guard_arena.py), at the shapes of
tests/scratch_guard_cases.py: scratch of exactly the size queried, every buffer between two 64 KiB bands of a fill byte at the
least alignment include/cotr_hip.h documents.  The GPU sanitizers are not available on shared machines; the bands, the exact
sizes and the documented alignments ask the same question without a tool.

Each case runs three times, with the fill 0x00, 0xA5 (a large negative float, a wild index) and 0xFF (NaN as a float, -1 as an
int), from fresh arenas, and asserts
1. the return code is 0, no band byte changed and no input changed;
2. the outputs are the numpy restatement's by the rule of that op's own GPU test, and every row the op must not write holds the
   fill;
3. the three runs wrote the same bytes: a read of scratch, of an output or of anything outside a buffer that reaches a result
   shows here;
4. a scratch one byte short, and a scratch 8 bytes off its 16-byte alignment, are refused with COTR_ERR_ARG before anything is
   launched: every output and the scratch still hold the fill.

Two controls show that the check sees what it should: with the scratch's rear band moved 256 bytes into the scratch (the library
is still told the true size, and the whole scratch stays inside the arena) a kernel that writes the end of its last region
trips the check; and one byte written into a band with a torch index assignment is found and named."""
import pytest
import torch

from cotr_amd import _lib
from tests import scratch_guard_cases as sg
from tests.guard_arena import BAND, GuardError

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xA5, 0xFF)
ERR_ARG = -1
CASES = sg.all_cases()
EARLY = [(e, c) for e, c in CASES if c.id == e.early]


def _id(ec):
    return f'{ec[0].name[5:]}-{ec[1].id}'


def enqueue(entry, call, nbytes, fill, **kw):
    """one call from a fresh arena -> (return code, arena, the outputs' (dtype, shape)), synchronized"""
    lib = _lib.load_library()
    arena, argv, outs = sg.place(call, nbytes, 'cuda', fill, **kw)
    torch.cuda.synchronize()
    rc = getattr(lib, entry.name)(*argv)
    torch.cuda.synchronize()
    return rc, arena, outs


def run(entry, params, fill):
    """a clean run: rc 0 and the arena intact -> the outputs as host arrays"""
    lib = _lib.load_library()
    call = entry.build(params)
    rc, arena, outs = enqueue(entry, call, entry.query(lib, params), fill)
    assert rc == 0, lib.cotr_raster_last_error()
    arena.check()
    return call, arena, sg.read_outputs(arena, outs)


same_written_bytes = sg.same_written_bytes


@pytest.mark.parametrize('ec', CASES, ids=_id)
def test_inside_its_buffers_and_equal_to_the_restatement(ec):
    entry, case = ec
    lib = _lib.load_library()
    twin_params = sg.twin_of(entry, case.params)
    twin = run(entry, twin_params, 0xA5)[2] if twin_params is not None else None
    first = None
    for fill in FILLS:
        call, arena, outs = run(entry, case.params, fill)
        if twin_params is not None:
            call.expect(outs, fill, twin)
        else:
            call.expect(outs, fill)
        if first is None:
            first = (fill, outs)
        else:
            for name in outs:
                same_written_bytes(first[1][name], first[0], outs[name], fill, name)
    # refusals: nothing is launched, so every output and the scratch keep the fill
    nbytes = entry.query(lib, case.params)
    attempts = []
    if case.refusal == 'both' and nbytes > 0:
        attempts.append(('one byte short', dict(scratch_bytes=nbytes - 1)))
    if case.refusal in ('both', 'align'):
        attempts.append(('8 bytes off 16-byte alignment', dict(scratch_shift=8)))
    for what, kw in attempts:
        rc, arena, outs = enqueue(entry, entry.build(case.params), nbytes, 0xA5, **kw)
        assert rc == ERR_ARG and lib.cotr_raster_last_error(), what
        arena.check()
        assert arena.all_fill('scratch') and all(arena.all_fill(name) for name in outs), what


@pytest.mark.parametrize('ec', EARLY, ids=_id)
def test_early_band_control(ec):
    """the rear band of the scratch starts 256 bytes before the scratch ends: the op's own kernels write there, and the check says so"""
    entry, case = ec
    lib = _lib.load_library()
    nbytes = entry.query(lib, case.params)
    assert nbytes >= 256
    rc, arena, _ = enqueue(entry, entry.build(case.params), nbytes, 0xA5, early_rear_band=256)
    assert rc == 0, lib.cotr_raster_last_error()
    with pytest.raises(GuardError, match=r"rear band of 'scratch'.*offsets -\d+ \.\. -\d+ from the buffer's end"):
        arena.check()


def test_harness_control_a_planted_byte_is_found_and_named():
    entry, case = sg.DELAUNAY, sg.DELAUNAY.cases[4]
    call, arena, _ = run(entry, case.params, 0xA5)
    b = arena.bufs['tris']
    arena.poke(b.rear + 37, 0x11)
    with pytest.raises(GuardError, match=r"rear band of 'tris'.*1 bytes are not fill 0xA5, offsets 37 \.\. 37 from the buffer's end"):
        arena.check()
    arena.poke(b.rear + 37, 0xA5)
    arena.check()
    arena.poke(arena.bufs['scratch'].start - 1, 0x00)
    with pytest.raises(GuardError, match=r"front band of 'scratch'.*offsets -1 \.\. -1 from the buffer's start"):
        arena.check()
    assert BAND == 64 * 1024
