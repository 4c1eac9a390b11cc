"""What tests/test_scratch_guard_gpu.py stands on, without a GPU: the guarded arena itself on ``device='cpu'`` (placement, both
bands, planted bytes, a modified input, the early rear band), the case table against the header (every entry point that takes a
scratch and no handle has a row), and every row's scratch-size query (host-only code) against what the header's text promises.

The arena (tests/guard_arena.py) places each buffer of a raw C-ABI call between two bands of one fill byte, at the least
alignment the header documents for that argument, and afterwards says which band byte or input byte changed.  The bands are
64 KiB: four times the 16 KiB that one workgroup of 1024 threads storing 16 bytes each can write past an end, so an overrun
by a whole workgroup still lands in a band and not in the next buffer."""
import os
import re

import numpy as np
import pytest

from tests import scratch_guard_cases as sg
from tests.guard_arena import BAND, KINDS, Arena, GuardError, fill_value, is_fill

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cotr_hip.h')


def small_arena(fill=0xA5, early=0):
    a = Arena('cpu', fill)
    a.add_input('points', np.arange(10, dtype=np.float64))
    a.add_input('flags', np.arange(7, dtype=np.uint8))
    a.add_output('out', np.float32, (5, 3))
    a.add_output('idx', np.int32, (0,))                       # an empty buffer still has its address and its bands
    a.add_output('rows', np.float64, (4, 4), kind='a16')
    a.add('scratch', 1024, 'scratch', early_rear_band=early)
    return a.build()


def test_band_width_is_four_workgroup_stores():
    assert BAND == 64 * 1024 == 4 * 1024 * 16


@pytest.mark.parametrize('fill', [0x00, 0xA5, 0xFF])
def test_placement_has_exactly_the_documented_residues(fill):
    a = small_arena(fill)
    base = a.mem.data_ptr()
    for name, kind in (('points', 'f64'), ('flags', 'u8'), ('out', 'f32'), ('idx', 'i32'), ('rows', 'a16'), ('scratch', 'scratch')):
        res, mod = KINDS[kind]
        assert a.addr(name) % mod == res, name               # that residue and no better: not a multiple of mod
        b = a.bufs[name]
        assert b.start - b.front >= BAND and b.start - b.front < BAND + mod            # the pad belongs to the front band
        assert b.rear == b.start + b.nbytes                                              # the buffer ends where the rear band begins
    order = list(a.bufs.values())
    for prev, nxt in zip(order, order[1:]):
        assert nxt.front == prev.rear + BAND
    assert a.addr('scratch') % 16 == 0 and a.addr('scratch') % 32 != 0 and a.addr('points') % 16 == 8 and a.addr('flags') % 2 == 1
    assert a.addr('out') % 8 == 4 and a.addr('rows') % 32 == 16
    assert base + a.used <= base + a.mem.numel()
    a.check()
    assert a.all_fill('out') and a.all_fill('scratch') and a.all_fill('rows')
    assert np.array_equal(a.view('points', np.float64, (10,)), np.arange(10.0)) and np.array_equal(a.view('flags', np.uint8, (7,)), np.arange(7))
    assert is_fill(a.view('out', np.float32, (5, 3)), fill).all()
    assert fill_value(0xFF, np.int32) == -1 and np.isnan(fill_value(0xFF, np.float64)) and fill_value(0xA5, np.float32) < -1e-20


def test_a_write_inside_a_buffer_is_not_reported():
    a = small_arena()
    for name in ('out', 'rows', 'scratch'):
        b = a.bufs[name]
        a.mem[b.start:b.start + b.nbytes] = 0x3C
    a.check()


@pytest.mark.parametrize('name,side,offset', [('out', 'front', -1), ('scratch', 'front', -1), ('scratch', 'front', -BAND), ('out', 'rear', 0),
                                              ('out', 'rear', BAND - 1), ('scratch', 'rear', 0), ('scratch', 'rear', BAND - 1),
                                              ('idx', 'rear', 0), ('idx', 'front', -1), ('flags', 'rear', 0)])
def test_a_planted_byte_is_reported_with_its_buffer_side_and_offset(name, side, offset):
    a = small_arena()
    b = a.bufs[name]
    at = (b.start if side == 'front' else b.start + b.nbytes) + offset
    a.poke(at, 0x5A)
    with pytest.raises(GuardError) as e:
        a.check()
    msg = str(e.value)
    assert f"{side} band of '{name}'" in msg and f'offsets {offset} .. {offset} from' in msg and '1 bytes are not fill 0xA5' in msg
    assert msg.count(' band of ') == 1                                                   # that band and no other
    a.poke(at, 0xA5)
    a.check()


def test_first_and_last_offending_offsets_of_a_run_of_bytes():
    a = small_arena()
    b = a.bufs['scratch']
    end = b.start + b.nbytes
    a.mem[end + 3:end + 4099] = 0
    with pytest.raises(GuardError, match=r"rear band of 'scratch' \(scratch, 1024 bytes\): 4096 bytes are not fill 0xA5, offsets 3 \.\. 4098 from the buffer's end"):
        a.check()


def test_a_pad_byte_in_front_of_a_buffer_belongs_to_the_front_band():
    a = small_arena()
    b = a.bufs['scratch']
    assert b.start - b.front > BAND                                                      # 16 (mod 256) needs a pad after 64 KiB
    a.poke(b.front + BAND, 0)                                                            # the first pad byte
    with pytest.raises(GuardError, match="front band of 'scratch'"):
        a.check()


def test_a_modified_input_is_reported():
    a = small_arena()
    b = a.bufs['points']
    a.poke(b.start + 17, 0xEE)
    with pytest.raises(GuardError, match=r"input 'points' was modified: 1 bytes differ, offsets 17 \.\. 17"):
        a.check()
    t = Arena('cpu', 0).add_input('table', np.zeros(4, np.uint64), 'a8').add_output('x', np.float32, (2,)).build()
    t.set_input('table', np.array([1, 2, t.addr('x'), 4], np.uint64))                   # a table of addresses, known after placement
    t.check()
    assert t.view('table', np.uint64, (4,))[2] == t.addr('x')
    t.poke(t.bufs['table'].start, 9)
    with pytest.raises(GuardError, match="input 'table' was modified"):
        t.check()


def test_early_rear_band_moves_the_band_into_the_buffer():
    a = small_arena(early=256)
    b = a.bufs['scratch']
    assert b.rear == b.start + b.nbytes - 256 and b.nbytes == 1024                       # the library is still told 1024 bytes
    assert b.rear + BAND <= a.mem.numel()                                                # the whole buffer lies inside the arena
    a.mem[b.start:b.start + b.nbytes - 256] = 1                                          # short of the moved band: clean
    a.check()
    a.mem[b.start:b.start + b.nbytes] = 1                                                # a kernel that writes its scratch in full
    with pytest.raises(GuardError, match=r"rear band of 'scratch'.*256 bytes are not fill 0xA5, offsets -256 \.\. -1 from the buffer's end"):
        a.check()


# ---- the table against the header --------------------------------------------------------------------------------------------
def scratch_taking_handleless_entry_points():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    found = set()
    for m in re.finditer(r'\b(?:int|size_t)\s+(cotr_\w+)\s*\(([^;{]*?)\)\s*;', text, flags=re.S):
        name, args = m.group(1), ' '.join(m.group(2).split())
        if re.search(r'void\s*\*\s*scratch\s*,\s*size_t\s+scratch_bytes', args) and not re.match(r'cotr_handle\b', args):
            found.add(name)
    return found


def test_every_scratch_taking_handleless_entry_point_has_a_row():
    header = scratch_taking_handleless_entry_points()
    table = {e.name for e in sg.ENTRIES}
    assert len(header) >= 17 and 'cotr_raster_mesh' in header and 'cotr_overlap_pairs' in header
    assert header == table, f'without a row: {sorted(header - table)}; rows without an entry point: {sorted(table - header)}'
    assert len(table) == len(sg.ENTRIES)
    for e in sg.ENTRIES:
        ids = [c.id for c in e.cases]
        assert len(set(ids)) == len(ids) and len(ids) >= 5, e.name
        # the early-band control: the case at which the last scratch region is written to its end, or the reason there is none
        assert e.early in ids or e.early.startswith(e.name[5:].split('_')[0]), e.name


def test_no_case_is_heavier_than_the_issue_allows():
    for e, c in sg.all_cases():
        if e.name == 'cotr_delaunay':
            assert c.params[0] <= 1024
        if e.name.startswith('cotr_ransac_'):
            assert c.params[0][-2] <= 64


# ---- the size queries (host-only code) ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from cotr_amd import _lib
    from cotr_amd.build import build_library
    build_library()
    return _lib.load_library()


@pytest.mark.parametrize('entry', sg.ENTRIES, ids=lambda e: e.name[5:])
def test_size_queries_of_every_case(lib, entry):
    for case in entry.cases:
        nbytes = entry.query(lib, case.params)
        need = entry.min_bytes(case.params)
        assert nbytes >= need, (case.id, nbytes, need)
        if entry.carver:
            assert nbytes % 256 == 0, (case.id, nbytes)
        else:
            assert nbytes % 16 == 0 and nbytes == need, (case.id, nbytes, need)        # the header states these sizes exactly
        # the call can be laid out: every buffer at its residue, scratch of exactly that size
        arena, argv, outs = sg.place(entry.build(case.params), nbytes, 'cpu', 0xA5)
        assert arena.nbytes('scratch') == nbytes and arena.addr('scratch') % 256 == 16
        fn = getattr(lib, entry.name)                                                   # the row's arguments are the prototype's
        assert len(fn.argtypes) == len(argv), (case.id, len(fn.argtypes), len(argv))
        for t, a in zip(fn.argtypes, argv):
            t.from_param(a)
        arena.check()
        assert all(arena.all_fill(name) for name in outs)


def test_the_exact_region_cases_are_exact(lib):
    """the shapes chosen so that a scratch region is a whole number of 256-byte units: one element more moves the size by 256"""
    q = lambda fn, *dims: sg.size_by_pointer(fn, lambda p: p)(lib, dims)   # noqa: E731
    assert q('cotr_delaunay_scratch_bytes', 64) + 5 * 256 == q('cotr_delaunay_scratch_bytes', 65)             # all five regions grow
    assert q('cotr_delaunay_scratch_bytes', 63) == q('cotr_delaunay_scratch_bytes', 64)
    assert q('cotr_tsdf_mesh_scratch_bytes', 32, 32, 16) == 2 * 16384 + 4 * 16384 + 256 + 256                  # 32 blocks: 256-byte totals and bases
    assert q('cotr_raster_mesh_scratch_bytes', 7936, 7, 13) + 3 * 256 == q('cotr_raster_mesh_scratch_bytes', 7937, 7, 13)             # recs, local, bsum
    assert q('cotr_nearest_mutual_scratch_bytes', 64, 64) == 128 * 8 + 128 * 4
    assert q('cotr_ransac_fundamental_scratch_bytes', 63, 64) == 192 * 72 + 192 * 4
    assert lib.cotr_depth_corrs_scratch(2, 64 * 128) == 64 * 36 and lib.cotr_overlap_scratch(1, 17 * 23) == 1568
