"""Record how the library plans a call - its size queries and its pass walk - into tests/golden/plan_sizes.json.

Runs on the MI355X (the decode walk follows the rows kernels' dispatch predicates, which read the CU count).  For every knob set
of KNOB_SETS and every (pairs, queries) of the grid it stores cotr_scratch_bytes, cotr_workspace_bytes (weights loaded: the
weight arena is part of that number) and the encode / decode passes cotr_batch_chunks reports.  tests/test_plan_gpu.py asks the
library the same questions and expects the same answers: a change to the planning code that is meant to keep behaviour must
keep every number.

    python tests/golden/make_plan_golden.py [PATH]     # rewrites tests/golden/plan_sizes.json (or writes PATH)
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PAIRS = [1, 2, 3, 4, 7, 8, 16, 17, 29, 32, 33, 64, 65, 129]
QUERIES = [0, 1, 257, 1000, 8192, 20000, 32768, 131072]
BIG = 1 << 30
# the defaults, and every knob value that moves a pass boundary or an arena size
KNOB_SETS = {
    'default': {},
    'encode_chunk=1': {'encode_chunk': 1},
    'encode_chunk=7': {'encode_chunk': 7},
    'encode_chunk=128': {'encode_chunk': 128},
    'attention_fusion_max_rows=0': {'attention_fusion_max_rows': 0},
    'attention_fusion_max_rows=big': {'attention_fusion_max_rows': BIG},
    'ffn_fusion_max_rows=0': {'ffn_fusion_max_rows': 0},
    'ffn_fusion_max_rows=big': {'ffn_fusion_max_rows': BIG},
    'att_rows_min_rows=0': {'att_rows_min_rows': 0},
    'att_rows_min_rows=big': {'att_rows_min_rows': BIG},
    'ffn_rows_min_rows=0': {'ffn_rows_min_rows': 0},
    'ffn_rows_min_rows=big': {'ffn_rows_min_rows': BIG},
    'rows_min_fill=0': {'rows_min_fill': 0},
    'batch_split=0': {'batch_split': 0},
}
PATH = os.path.join(HERE, 'plan_sizes.json')


def loaded_handle():
    """A model's library handle with the seeded synthetic weights loaded (cotr_workspace_bytes counts the weight arena)."""
    import torch
    import cotr_amd
    from cotr_amd.models import build_model
    from cotr_amd.utils.synth import synth_state_dict
    m = build_model(cotr_amd.default_args()).cuda().eval()
    m.load_state_dict(synth_state_dict(0))
    m._ensure_ready(torch.device('cuda'))
    return m


def runs(sizes):
    """[3, 3, 3, 1] -> [[3, 3], [1, 1]]: (pass size, repeat) - a 129-pair walk of single pairs stays one entry"""
    out = []
    for c in sizes:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return out


def plan_numbers(handle, b, q):
    from cotr_amd import _lib
    lib = _lib.load_library()
    scratch, ws = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(lib.cotr_scratch_bytes(handle, b, q, ctypes.byref(scratch)), handle, 'cotr_scratch_bytes')
    _lib.check(lib.cotr_workspace_bytes(handle, b, q, ctypes.byref(ws)), handle, 'cotr_workspace_bytes')
    passes = []
    for which in (0, 1):
        sizes = (ctypes.c_int * 256)()
        n = lib.cotr_batch_chunks(handle, b, q, which, sizes, 256)
        assert 0 <= n <= 256, n
        passes.append(runs(sizes[:n]))
    return {'scratch_bytes': scratch.value, 'workspace_bytes': ws.value, 'encode_passes': passes[0], 'decode_passes': passes[1]}


def all_numbers(handle):
    """{knob set: {'BxQ': plan_numbers}}; the handle's knobs are back at their defaults afterwards"""
    from cotr_amd import _lib
    out = {}
    try:
        for name, knobs in KNOB_SETS.items():
            _lib.reset_knobs(handle)
            for k, v in knobs.items():
                _lib.set_knob(k, v, handle)
            out[name] = {f'{b}x{q}': plan_numbers(handle, b, q) for b in PAIRS for q in QUERIES}
    finally:
        _lib.reset_knobs(handle)
    return out


def main():
    m = loaded_handle()
    data = all_numbers(m._handle)
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(path, 'w') as f:
        json.dump(data, f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    print(f'{sum(len(v) for v in data.values())} shapes x knob sets -> {path}')


if __name__ == '__main__':
    main()
