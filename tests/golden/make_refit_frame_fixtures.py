"""Records refit_frame_sha.json: the sha256 of every array the calls of tests/refit_frame_cases.py return, as THIS build of the
library computes them.  It was recorded on the commit before the Gauss-Newton refits of homography.hip, pnp.hip and
essential.hip moved onto the one frame of csrc/refit.h, which runs their arithmetic in their order: the yardstick of
tests/test_refit_frame_gpu.py is that commit, not the code under test.

    python tests/golden/make_refit_frame_fixtures.py [directory]      # MI355X
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main(where=HERE):
    from tests import refit_frame_cases as C
    out = {}
    for name in C.CASES:
        out[name] = C.hashes(name)
        print(f'{name}: {len(out[name])} arrays', flush=True)
    os.makedirs(where, exist_ok=True)
    with open(os.path.join(where, 'refit_frame_sha.json'), 'w') as f:
        json.dump(out, f, sort_keys=True, indent=0, separators=(',', ':'))
        f.write('\n')
    print(f'{len(out)} cases, {sum(len(v) for v in out.values())} arrays')


if __name__ == '__main__':
    main(*sys.argv[1:])
