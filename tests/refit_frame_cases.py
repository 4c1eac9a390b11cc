"""The calls whose bits the refit frame (cotr_amd/csrc/refit.h) must leave as they were: one list for
tests/golden/make_refit_frame_fixtures.py, which recorded them on the commit before the frame, and for
tests/test_refit_frame_gpu.py, which compares.  The scenes are the oracle modules' own: n = 4, 5, 6, the wavefront (63, 64, 65),
the 256-thread block, the 2048-point chunk (2047, 2048, 2049: the first size at which a finish kernel adds two chunks) and
three chunks (4097, 5000)."""
import ctypes
import hashlib

import numpy as np
import torch

from tests import essential_oracle as eo
from tests import homography_oracle as ho
from tests import pnp_oracle as pn
from tests import pose_refit_oracle as po

REFINE_ITERS = (10, 0)
ROUNDS_ITERS = ((1, 0), (1, 10), (4, 10), (8, 3))


def _host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def homography(scene, refine_iters):
    from cotr_amd.inference import ransac_homography
    n, outl, noise, thr, conf, iters, seed = scene
    p1, p2, _, _ = ho.planar_scene(n, outl, seed, noise)
    return _host(ransac_homography(p1, p2, thr, conf, iters, seed, refine_iters, hypotheses=True))


def pnp(scene, refine_iters):
    from cotr_amd.inference import ransac_pnp
    n, outl, noise, thr, conf, iters, seed = scene
    obj, img, K, _, _, _ = pn.pnp_scene(n, outl, seed % (1 << 32), noise)
    return _host(ransac_pnp(obj, img, K, thr, conf, iters, seed, refine_iters=refine_iters, hypotheses=True))


def refine_pose(scene, rounds, refine_iters):
    """cotr_refine_pose through the C ABI from po.start(scene), the scratch filled with 0xA5 beforehand -> its five outputs and
    ``parts``: the per-chunk sums [chunks][22] the last accumulate left at the end of the scratch (256-byte aligned), read as
    tests/test_pose_refit_gpu.py::test_one_accumulation_against_the_restatement reads them"""
    from cotr_amd import _lib
    s = po.start(scene)
    n = scene[0]
    lib = _lib.load_library()
    nb = ctypes.c_size_t()
    assert lib.cotr_refine_pose_scratch_bytes(n, ctypes.byref(nb)) == 0
    chunks = (n + 2047) // 2048
    parts_at = nb.value - (chunks * 22 * 8 + 255) // 256 * 256
    K9 = ctypes.c_double * 9
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()   # noqa: E731
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    R, t, d1, d2 = dev(s['R0'].reshape(9), torch.float64), dev(s['t0'], torch.float64), dev(s['p1'], torch.float64), dev(s['p2'], torch.float64)
    m = dev(s['mask0'], torch.uint8)
    scratch = torch.full((nb.value,), 0xA5, dtype=torch.uint8, device='cuda')
    out = dict(R=torch.empty(9, dtype=torch.float64, device='cuda'), t=torch.empty(3, dtype=torch.float64, device='cuda'),
               E=torch.empty(9, dtype=torch.float64, device='cuda'), mask=torch.empty(n, dtype=torch.uint8, device='cuda'),
               info=torch.empty(8, dtype=torch.int32, device='cuda'))
    rc = lib.cotr_refine_pose(p(R), p(t), p(d1), p(d2), n, K9(*s['K1'].reshape(9)), K9(*s['K2'].reshape(9)), s['thr'], 50.0, rounds, refine_iters,
                              p(m), None, p(out['R']), p(out['t']), p(out['E']), p(out['mask']), p(out['info']), p(scratch), nb.value,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.cotr_raster_last_error()
    out['parts'] = scratch[parts_at:parts_at + chunks * 22 * 8]
    return _host(out)


def relative_pose(scene):
    from cotr_amd.inference.essential import relative_pose_tensors
    n, outl, noise, thr, conf, iters, seed = scene
    p1, p2, K1, K2, _, _, _ = eo.two_view_scene(n, outl, seed, noise)
    return _host(relative_pose_tensors(p1, p2, K1, K2, thr, conf, iters, seed, refine_rounds=4, refine_iters=10))


def _tag(scene):
    return f'n{scene[0]}-it{scene[5]}-seed{scene[6]}'


# name -> (function, arguments): the call returns a dict of numpy arrays
CASES = {}
for _s in ho.SCENES + ho.EDGES:
    for _it in REFINE_ITERS:
        CASES[f'homography {_tag(_s)} refine{_it}'] = (homography, (_s, _it))
for _s in pn.SCENES + pn.EDGES:
    for _it in REFINE_ITERS:
        CASES[f'pnp {_tag(_s)} refine{_it}'] = (pnp, (_s, _it))
for _s in po.SIZES:
    for _r, _it in ROUNDS_ITERS:
        CASES[f'refine_pose {_tag(_s)} rounds{_r} refine{_it}'] = (refine_pose, (_s, _r, _it))
for _s in po.QUALITY:
    CASES[f'relative_pose {_tag(_s)}'] = (relative_pose, (_s,))


def hashes(name):
    """the sha256 of the raw bytes (NaNs included) of every array the case returns"""
    fn, args = CASES[name]
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in fn(*args).items()}
