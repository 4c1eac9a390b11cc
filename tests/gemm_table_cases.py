"""The cases behind tests/golden/gemm_picks.json and forward_launch_names.json, shared by the tests that compare against them
(tests/test_gemm_table_cpu.py, tests/test_gemm_table_gpu.py) and the script that recorded them (tests/golden/make_gemm_fixtures.py)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICK_BATCHES = (1, 2, 3, 4, 8, 16, 32, 64)
PICK_M_SCALES = (1.0, 0.6, 1.7, 3.5)          # exact hit, nearest measured M on either side, past it (cost model)
PICK_KNOB_SETS = ({}, {'ks3': 0, 'conv_patch': 0})
FORWARD_SHAPES = ((1, 100), (3, 100), (8, 100))   # dual launches everywhere; past layer1's 16384-row dual threshold; a batched pass
DUAL_CFGS = (3, 4, 10, 13, 14, 16, 26, 27, 32, 34, 35, 36)


def backbone_convs():
    """(Hin = Win per half, Cin, Cout, ksize, stride) of every convolution of torchvision's resnet50 from layer1 to layer3 as
    csrc/api.hip launches them on the 64 x 64 halves behind the stem (the stride of an entry block sits on conv2 and the downsample)."""
    out, H, cin = [], 64, 64
    for planes, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2)):
        for b in range(blocks):
            s = stride if b == 0 else 1
            if b == 0:
                out.append((H, cin, 4 * planes, 1, s))
            out += [(H, cin, planes, 1, 1), (H, planes, planes, 3, s), (H // s, planes, 4 * planes, 1, 1)]
            H, cin = H // s, 4 * planes
    return list(dict.fromkeys(out))


def tuned_dense_rows():
    """(M, N, K) of every dense row of csrc/gemm_tuned.inc"""
    rows = []
    for line in open(os.path.join(ROOT, 'cotr_amd', 'csrc', 'gemm_tuned.inc')):
        m = re.match(r'\{0, (\d+), (\d+), (\d+), \d+, \d+\}', line)
        if m:
            rows.append(tuple(int(v) for v in m.groups()))
    return list(dict.fromkeys(rows))


def compute_picks():
    """-> per knob set of PICK_KNOB_SETS {'knobs', 'cases': [name], 'picks': [configuration]} in one fixed case order (the fixture keeps
    the picks only); the process-wide knobs are back at their defaults afterwards"""
    from cotr_amd import _lib
    lib = _lib.load_library()
    out = []
    try:
        for knobs in PICK_KNOB_SETS:
            _lib.reset_knobs()
            for k, v in knobs.items():
                _lib.set_knob(k, v)
            picks = {}
            for (H, cin, cout, k, s) in backbone_convs():
                for B in PICK_BATCHES:
                    picks[f'conv {B},{H},{cin},{cout},{k},{s}'] = lib.cotr_gemm_pick_conv(B, H, H, cin, cout, k, s)
            for (M, N, K) in tuned_dense_rows():
                for f in PICK_M_SCALES:
                    m = int(round(M * f))
                    for flags in (0, 1, 2):
                        picks[f'linear {m},{N},{K},{flags}'] = lib.cotr_gemm_pick_linear(m, N, K, flags)
            out.append({'knobs': knobs, 'cases': list(picks), 'picks': list(picks.values())})
    finally:
        _lib.reset_knobs()
    return out


def forward_launch_names():
    """-> {"B,Q": profile_names() at level 2} of a synthetic-weight model's forward at FORWARD_SHAPES"""
    import cotr_amd
    from cotr_amd.models import build_model
    from cotr_amd.utils.synth import synth_state_dict, synth_inputs
    m = build_model(cotr_amd.default_args()).cuda().eval()
    m.load_state_dict(synth_state_dict(0))
    out = {}
    for B, Q in FORWARD_SHAPES:
        img, qs = synth_inputs(B, Q)
        m.set_profiling(2)
        m(img.cuda(), qs.cuda())
        out[f'{B},{Q}'] = m.profile_names()
        m.set_profiling(0)
    return out
