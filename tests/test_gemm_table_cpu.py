"""The launch-configuration table of the GEMM kernels (csrc/gemm.hip kCfgs, one row per configuration) against what the library
picked and reported before the configurations were described by rows: tests/golden/gemm_picks.json (make_gemm_fixtures.py).  No GPU:
cotr_gemm_pick_conv, cotr_gemm_pick_linear and cotr_gemm_config_info make no HIP call."""
import ctypes
import importlib.util
import json
import os

from cotr_amd import _lib
from cotr_amd.build import build_library
from tests import gemm_table_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_picks_match_the_recorded_ones():
    """every backbone convolution at 1 - 64 pairs and every dense row of gemm_tuned.inc at its own, a nearby and a far row count
    (exact hit, nearest M, cost model), plain / with the x + pos prologue / with a table residual, under the default knobs and with
    ks3 = conv_patch = 0"""
    build_library()
    with open(os.path.join(ROOT, 'tests', 'golden', 'gemm_picks.json')) as f:
        want = json.load(f)
    got = C.compute_picks()
    assert _lib.knobs() == {k: (v[1], v[1]) for k, v in _lib.knobs().items()}      # the process-wide set is back at its defaults
    assert [g['knobs'] for g in got] == [w['knobs'] for w in want] == list(C.PICK_KNOB_SETS)
    for g, w in zip(got, want):
        assert len(g['picks']) == len(w['picks']) > 2000
        assert {'conv', 'linear'} == {c.split()[0] for c in g['cases']}
        bad = [(c, a, b) for c, a, b in zip(g['cases'], g['picks'], w['picks']) if a != b]
        assert not bad, (g['knobs'], len(bad), bad[:8])
    assert got[0]['picks'] != got[1]['picks']                                         # the two knobs do reach the picks


def test_config_info_agrees_with_the_floor_table_and_the_dual_list():
    build_library()
    lib = _lib.load_library()
    spec = importlib.util.spec_from_file_location('floor_table', os.path.join(ROOT, 'tools', 'floor_table.py'))
    floor_table = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(floor_table)
    n = lib.cotr_gemm_num_configs()
    assert n == 42
    bm, bn, dual = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    info = {}
    for cfg in range(n):
        assert lib.cotr_gemm_config_info(cfg, ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(dual)) == 0
        info[cfg] = (bm.value, bn.value, dual.value)
    for cfg, tile in floor_table.TILE.items():
        assert info[cfg][:2] == tile, (cfg, info[cfg], tile)
    assert tuple(c for c in range(n) if info[c][2] == 1) == C.DUAL_CFGS
    assert all(info[c][2] in (0, 1) for c in range(n))
    assert info[28] == info[29] == (0, 0, 0)                                          # research-only indices: rows that never fit
    assert lib.cotr_gemm_config_info(-1, None, None, None) != 0 and lib.cotr_gemm_config_info(n, None, None, None) != 0
    assert lib.cotr_gemm_config_info(0, None, None, None) == 0
