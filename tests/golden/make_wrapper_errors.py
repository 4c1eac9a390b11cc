"""Records wrapper_errors.json: what every call of tests/wrapper_error_cases.py raises, as THIS checkout of the wrappers under
cotr_amd/inference/ checks its arguments, and which library calls its chained functions make with which scalars.  It was
recorded on the commit before the wrappers' argument rules moved into inference/_args.py, where every module still bound its
own ``_device`` and ``_no_cpu_tensors``: the yardstick of tests/test_wrapper_errors_cpu.py is that commit, not the code under
test.  No GPU and no built library: a call that gets as far as picking its device is recorded as DeviceReached.

    python tests/golden/make_wrapper_errors.py [directory]
"""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

MODULES = ['_ransac', '_args', 'guided', 'homography', 'essential', 'pnp', 'structure', 'bundle', 'rigid3d', 'icp', 'triangulate', 'warp']


def replace_everywhere(names, value, undo):
    """the device rule and the CPU-tensor refusal, wherever a module binds one under one of ``names``"""
    for m in MODULES:
        try:
            mod = importlib.import_module('cotr_amd.inference.' + m)
        except ImportError:
            continue
        for name in names:
            if hasattr(mod, name):
                undo.append((mod, name, getattr(mod, name)))
                setattr(mod, name, value)


def patch(obj, name, value, undo):
    undo.append((obj, name, getattr(obj, name)))
    setattr(obj, name, value)


def main(where=HERE):
    import torch
    from cotr_amd import _lib
    from tests import wrapper_error_cases as C
    undo = []
    replace_everywhere(('_device', 'device'), C.reached_device, undo)
    patch(_lib, 'load_library', C.reached_library, undo)   # no row may show it: a check behind it is not an argument check
    errors = [[path, cid] + C.outcome(path, base, over) for path, cid, base, over in C.cases()]
    for mod, name, value in reversed(undo):
        setattr(mod, name, value)
    print(f'{len(errors)} calls, {sum(e[2] == "DeviceReached" for e in errors)} of them reach the device')

    undo, calls = [], {}
    replace_everywhere(('_device', 'device'), lambda device=None: torch.device('cpu'), undo)
    replace_everywhere(('_no_cpu_tensors', 'no_cpu_tensors'), lambda *xs: None, undo)
    for name, call in C.sequences().items():
        rec = C.Recorder()
        C.cpu_patches(lambda o, n, v: patch(o, n, v, undo), rec)
        call()
        calls[name] = rec.log
        print(f'{name}: {[c[0] for c in rec.log]}')
    for mod, name, value in reversed(undo):
        setattr(mod, name, value)

    os.makedirs(where, exist_ok=True)
    with open(os.path.join(where, 'wrapper_errors.json'), 'w') as f:
        json.dump(dict(errors=errors, calls=calls), f, indent=0, separators=(',', ':'))
        f.write('\n')


if __name__ == '__main__':
    main(*sys.argv[1:])
