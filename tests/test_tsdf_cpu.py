"""The TSDF volume without a GPU: the numpy restatement (tests/tsdf_oracle.py) against a scalar loop and against scenes whose
answer is known - a plane's signed distance, the weight cap, one call against n calls, the raycast of a fused plane, the
back-face rule - and the argument checks of the C ABI (they run before any HIP call) and of the Python wrappers."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.build import declared_symbols
from cotr_amd.data import Capture
from cotr_amd.inference import TsdfVolume, fuse_captures, integrate_depths, raycast_volume, track_capture
from tests import icp_oracle as io
from tests import tsdf_oracle as to

NAMES = ['cotr_tsdf_integrate', 'cotr_tsdf_raycast']
F32 = 2.0 ** -24   # the relative rounding of a float32


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_restatement_against_a_scalar_loop_on_a_tiny_volume():
    dims, voxel, trunc = (4, 3, 5), 0.1, 0.3
    origin = to.small_origin(dims)
    depths, Ks, c2ws = to.captures(24, 32)
    r = to.integrate(*to.fresh(dims), origin, voxel, trunc, depths, Ks, c2ws, weights=[1.0, 2.5], max_weight=3.0)
    T, Wt = to.fresh(dims)
    for c in range(2):
        for k in range(dims[2]):
            for j in range(dims[1]):
                for i in range(dims[0]):
                    T[k, j, i], Wt[k, j, i] = to.integrate_voxel(T[k, j, i], Wt[k, j, i], i, j, k, origin, voxel, trunc, depths[c], Ks[c], c2ws[c],
                                                                 (1.0, 2.5)[c], 3.0)
    assert np.array_equal(r['tsdf'], T) and np.array_equal(r['weight'], Wt)
    assert (r['info'][:, 0] == 1).all() and (r['info'][:, 1] > 0).all() and (Wt == 3.0).any() and not r['near'].any()


def _plane_case(z0=2.0, H=24, W=32):
    """a fronto-parallel plane at depth z0 seen from the world's origin, and a 16 x 12 x 20 volume across it"""
    K = np.array([[40.0, 0.2, W / 2 - 0.3], [0.0, 41.0, H / 2 + 0.2], [0.0, 0.0, 1.0]])
    depth = np.full((H, W), z0, np.float32)
    dims, voxel, trunc = (16, 12, 20), 0.05, 0.15
    origin = (-0.371, -0.283, z0 - 0.4873)
    return depth, K, np.eye(4), dims, voxel, trunc, origin


def test_a_plane_from_one_camera_is_its_signed_distance_inside_the_band():
    depth, K, c2w, dims, voxel, trunc, origin = _plane_case()
    r = to.integrate(*to.fresh(dims), origin, voxel, trunc, depth[None], K[None], c2w[None])
    z = origin[2] + voxel * np.arange(dims[2])
    sd = np.broadcast_to((2.0 - z)[:, None, None], r['tsdf'].shape)
    seen = r['weight'] > 0
    assert seen.sum() == r['info'][0, 1] and 0 < seen.sum() < seen.size
    band = seen & (np.abs(sd) < trunc)
    assert band.sum() > 500 and np.abs(r['tsdf'][band].astype(np.float64) * trunc - sd[band]).max() <= trunc * F32 + 1e-15
    assert (r['tsdf'][seen & (sd >= trunc)] == 1).all() and not (seen & (sd < -trunc - 1e-12)).any()
    assert (r['tsdf'][~seen] == 1).all() and (r['weight'][seen] == 1).all()


def test_the_weight_stops_at_its_cap_and_the_value_stays_an_average():
    depth, K, c2w, dims, voxel, trunc, origin = _plane_case()
    vol = to.fresh(dims)
    one = to.integrate(*vol, origin, voxel, trunc, depth[None], K[None], c2w[None])
    r = to.integrate(*vol, origin, voxel, trunc, np.stack([depth] * 5), np.stack([K] * 5), np.stack([c2w] * 5), weights=[1, 1, 1, 1, 0.5], max_weight=3.0)
    seen = one['weight'] > 0
    assert (r['weight'][seen] == 3.0).all() and (r['weight'][~seen] == 0).all()
    assert np.abs(r['tsdf'].astype(np.float64) - one['tsdf']).max() <= 5 * F32   # the average of equal observations, rounded 5 times
    # a nearer plane afterwards pulls a capped voxel by w / (3 + w)
    near = to.integrate(r['tsdf'], r['weight'], origin, voxel, trunc, (depth - 0.05)[None], K[None], c2w[None], max_weight=3.0)
    both = seen & (near['weight'] == 3.0) & (np.abs(one['tsdf']) < 0.6)
    want = (3 * r['tsdf'][both].astype(np.float64) + (r['tsdf'][both] - 0.05 / trunc)) / 4
    assert both.sum() > 100 and np.abs(near['tsdf'][both] - want).max() <= 4 * F32


def test_n_captures_in_one_call_are_n_calls():
    depths, Ks, c2ws = to.captures(24, 32, 5)
    dims = (8, 8, 8)
    origin = to.small_origin(dims)
    found = [1, 0, 1, 1, 0]
    once = to.integrate(*to.fresh(dims), origin, 0.1, 0.3, depths, Ks, c2ws, found=found, weights=[1, 2, 3, 4, 5], max_weight=6.0)
    T, Wt = to.fresh(dims)
    for c in range(5):
        step = to.integrate(T, Wt, origin, 0.1, 0.3, depths[c:c + 1], Ks[c:c + 1], c2ws[c:c + 1], found=found[c:c + 1], weights=[c + 1], max_weight=6.0)
        T, Wt = step['tsdf'], step['weight']
        assert list(step['info'][0]) == list(once['info'][c]) and (step['info'][0, 0] == 1) == (found[c] == 1)
    assert np.array_equal(once['tsdf'], T) and np.array_equal(once['weight'], Wt) and (once['info'][[1, 4]] == 0).all()


def test_a_raycast_of_a_fused_plane_returns_its_depth():
    depth, K, c2w, dims, voxel, trunc, origin = _plane_case()
    r = to.integrate(*to.fresh(dims), origin, voxel, trunc, depth[None], K[None], c2w[None])
    # inside the band the stored value is linear in the position up to its float32 rounding, so the trilinear blend and the
    # crossing are exact up to that rounding at the two samples around it, and the float32 rounding of the depth written
    bound = 4 * trunc * F32 + 2.0 * F32
    for pose in (np.eye(4), io.po.pose_matrix((2.0, -3.0, 1.0), (0.05, -0.02, 0.3))):
        ray = to.raycast(r['tsdf'], r['weight'], origin, voxel, K, pose, depth.shape, 0.0, 3.0, trunc / 2, normals=True)
        hit = ray['depth'] > 0
        ref = io.render(*depth.shape, K, pose, (((0.0, 0.0, 1.0), 2.0),))
        err = np.abs(ray['depth'][hit].astype(np.float64) - ref[hit]).max()
        print(f'{hit.sum()} of {hit.size} pixels hit, depth within {err:.2e} (bound {bound:.2e})')
        # the volume spans 0.75 x 0.55 of the plane: 15 x 11 pixels at this focal length
        assert hit.sum() == ray['info'][1] > 100 and ray['info'][2] == 0 and err <= bound
        n = ray['normals'][hit]
        ok = ~np.isnan(n[:, 0])
        want = -pose[:3, :3].T @ np.array([0.0, 0.0, 1.0])   # the gradient points from behind the surface to its front
        assert ok.sum() > hit.sum() // 2 and np.abs(n[ok] - want).max() <= 1e-5 and np.isnan(ray['normals'][~hit]).all()


def test_a_crossing_from_behind_ends_the_ray_with_no_hit():
    c = to.crossings()
    tsdf, weight, origin, voxel, K = c['tsdf'], c['weight'], c['origin'], c['voxel'], c['K']
    front = to.raycast(tsdf, weight, origin, voxel, K, np.eye(4), (5, 5), 0.5, 3.8, 0.15)
    assert list(front['info']) == [1, 25, 0, 0] and np.abs(front['depth'] - 1.55).max() < 1e-6
    behind = to.raycast(tsdf, weight, origin, voxel, K, np.eye(4), (5, 5), 1.8, 3.8, 0.15)
    assert list(behind['info']) == [1, 0, 25, 0] and (behind['depth'] == 0).all()   # not the crossing at 3.15 further on
    # an unobserved slab between the two resets "previous": the walk goes on and finds the third crossing
    gap = weight.copy()
    gap[21:23] = 0
    after = to.raycast(tsdf, gap, origin, voxel, K, np.eye(4), (5, 5), 1.8, 3.8, 0.15)
    assert list(after['info']) == [1, 25, 0, 0] and np.abs(after['depth'] - 3.15).max() < 1e-6
    off = to.raycast(tsdf, weight, origin, voxel, K, np.eye(4), (5, 5), 0.5, 3.8, 0.15, normals=True, found=[0])
    assert (off['depth'] == 0).all() and (off['normals'] == 0).all() and (off['info'] == 0).all()


def test_the_corner_scene_flags_nothing_and_matches_its_renderer():
    f = to.fused()
    sc = io.scene(48, 64, 48, 64, 3)
    assert f['info'][:, 1].tolist() == [62639, 49100] and not f['near'].any() and not (np.abs(f['tsdf'] + 1) < 1e-9).any()
    ray = to.raycast(f['tsdf'], f['weight'], f['origin'], f['voxel'], sc['K_a'], sc['c2w_a'], (48, 64), 0.5, 8.0, f['trunc'] / 2)
    hit = ray['depth'] > 0
    err = np.abs(ray['depth'][hit] - io.render(48, 64, sc['K_a'], sc['c2w_a'], io.PLANES)[hit])
    print(f'{hit.sum()} pixels hit, depth error median {np.median(err):.2e}, p90 {np.percentile(err, 90):.2e}, max {err.max():.2e}')
    assert ray['info'].tolist() == [1, 2353, 0, 0] and not ray['near'].any()
    assert np.median(err) < f['voxel'] / 10 and err.max() < 2 * f['voxel']   # well inside a voxel; the worst sit on the creases


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and name in declared_symbols()
        assert getattr(_lib.load_library(), name) is not None


K9 = (ctypes.c_double * 9)(100.0, 0.5, 64.0, 0.0, 100.0, 48.0, 0.0, 0.0, 1.0)
P = ctypes.c_void_p(4096)              # never dereferenced: every call below fails its checks before any HIP call
ODD8, ODD4 = ctypes.c_void_p(4100), ctypes.c_void_p(4098)
NAN, INF = float('nan'), float('inf')
VOLUME_CASES = ((dict(Nx=1), b'2^28'), (dict(Ny=1), b'2^28'), (dict(Nz=1), b'2^28'), (dict(Nx=1 << 10, Ny=1 << 10, Nz=(1 << 8) + 1), b'2^28'),
                (dict(Nx=1 << 16, Ny=1 << 16, Nz=1 << 16), b'2^28'), (dict(voxel=0.0), b'voxel'), (dict(voxel=-1.0), b'voxel'),
                (dict(voxel=INF), b'voxel'), (dict(voxel=NAN), b'voxel'), (dict(tsdf=None), b'NULL'), (dict(weight=None), b'NULL'),
                (dict(origin=None), b'NULL'), (dict(origin=(ctypes.c_double * 3)(0.0, NAN, 0.0)), b'origin'),
                (dict(origin=(ctypes.c_double * 3)(INF, 0.0, 0.0)), b'origin'), (dict(tsdf=ODD4), b'aligned'), (dict(weight=ODD4), b'aligned'))


def _bad_k(i, v, n=1):
    k = (ctypes.c_double * (9 * n))(*(list(K9) * n))
    k[i] = v
    return k


def _check(call, cases, name):
    lib = _lib.load_library()
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())
        assert name in lib.cotr_raster_last_error()


def test_integrate_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    O = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    K2 = (ctypes.c_double * 18)(*(list(K9) * 2))

    def call(tsdf=P, weight=P, Nx=8, Ny=8, Nz=8, origin=O, voxel=0.1, trunc=0.3, depths=P, n=2, H=96, W=128, Ks=K2, c2w=P, found=None, obs=None,
             max_weight=64.0, info=P):
        return lib.cotr_tsdf_integrate(tsdf, weight, Nx, Ny, Nz, origin, voxel, trunc, depths, n, H, W, Ks, c2w, found, obs, max_weight, info, None)
    w2 = lambda a, b: (ctypes.c_double * 2)(a, b)   # noqa: E731
    _check(call, VOLUME_CASES + (
        (dict(trunc=0.0), b'trunc'), (dict(trunc=-0.1), b'trunc'), (dict(trunc=INF), b'trunc'), (dict(trunc=NAN), b'trunc'),
        (dict(n=0), b'[1, 32]'), (dict(n=33), b'[1, 32]'), (dict(H=0), b'pixels'), (dict(W=0), b'pixels'),
        (dict(H=1 << 14, W=(1 << 14) + 1), b'pixels'), (dict(max_weight=0.0), b'max_weight'), (dict(max_weight=-1.0), b'max_weight'),
        (dict(max_weight=NAN), b'max_weight'), (dict(depths=None), b'NULL'), (dict(Ks=None), b'NULL'), (dict(c2w=None), b'NULL'),
        (dict(info=None), b'NULL'), (dict(Ks=_bad_k(0, 0.0, 2)), b'focal'), (dict(Ks=_bad_k(9 + 4, 0.0, 2)), b'focal'),
        (dict(Ks=_bad_k(9 + 2, NAN, 2)), b'focal'), (dict(Ks=_bad_k(1, INF, 2)), b'focal'), (dict(obs=w2(1.0, 0.0)), b'obs_weight'),
        (dict(obs=w2(-1.0, 1.0)), b'obs_weight'), (dict(obs=w2(1.0, INF)), b'obs_weight'), (dict(obs=w2(NAN, 1.0)), b'obs_weight'),
        (dict(depths=ODD4), b'aligned'), (dict(c2w=ODD8), b'aligned'), (dict(found=ODD4), b'aligned'), (dict(info=ODD4), b'aligned')),
        b'cotr_tsdf_integrate')


def test_raycast_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    O = (ctypes.c_double * 3)(0.0, 0.0, 0.0)

    def call(tsdf=P, weight=P, Nx=8, Ny=8, Nz=8, origin=O, voxel=0.1, K=K9, c2w=P, found=None, H=96, W=128, near=0.0, far=8.0, step=0.15, depth=P,
             normal=None, info=P):
        return lib.cotr_tsdf_raycast(tsdf, weight, Nx, Ny, Nz, origin, voxel, K, c2w, found, H, W, near, far, step, depth, normal, info, None)
    _check(call, VOLUME_CASES + (
        (dict(H=0), b'pixels'), (dict(W=0), b'pixels'), (dict(H=(1 << 14) + 1, W=1 << 14), b'pixels'), (dict(near=-0.1), b'near'),
        (dict(near=NAN), b'near'), (dict(near=INF), b'near'), (dict(far=0.0), b'far'), (dict(near=1.0, far=1.0), b'far'), (dict(far=INF), b'far'),
        (dict(far=NAN), b'far'), (dict(step=0.0), b'step'), (dict(step=-1.0), b'step'), (dict(step=NAN), b'step'), (dict(step=INF), b'step'),
        (dict(far=65537.0, step=1.0), b'65536'), (dict(far=65536.5, step=1.0), b'65536'), (dict(far=1.0, step=1e-6), b'65536'),
        (dict(K=None), b'NULL'), (dict(c2w=None), b'NULL'), (dict(depth=None), b'NULL'), (dict(info=None), b'NULL'),
        (dict(K=_bad_k(0, 0.0)), b'focal'), (dict(K=_bad_k(4, 0.0)), b'focal'), (dict(K=_bad_k(5, NAN)), b'focal'),
        (dict(c2w=ODD8), b'aligned'), (dict(found=ODD4), b'aligned'), (dict(depth=ODD4), b'aligned'), (dict(normal=ODD8), b'aligned'),
        (dict(info=ODD4), b'aligned')), b'cotr_tsdf_raycast')


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
K = np.array([[100.0, 0.5, 6.0], [0.0, 100.0, 5.0], [0.0, 0.0, 1.0]])
D = np.ones((2, 10, 12), np.float32)
C = np.stack([np.eye(4)] * 2)


def _volume():
    """a volume's scalars without its tensors: every check below fails before a tensor is read"""
    v = TsdfVolume.__new__(TsdfVolume)
    v.origin, v.voxel, v.dims, v.trunc, v.max_weight = np.zeros(3), 0.1, (8, 8, 8), 0.3, 64.0
    v.device, v.tsdf, v.weight = torch.device('cpu'), None, None
    return v


def test_wrapper_argument_errors_without_a_gpu():
    for kw, word in ((dict(origin=(0, 0)), 'origin'), (dict(origin=(0, NAN, 0)), 'origin'), (dict(voxel=0.0), 'voxel'), (dict(voxel=INF), 'voxel'),
                     (dict(dims=(8, 8)), 'dims'), (dict(dims=(1, 8, 8)), 'Nx'), (dict(dims=(8, 8, 1.5)), 'Nz'), (dict(dims=(1 << 10, 1 << 10, 257)), '2\\^28'),
                     (dict(trunc=0.0), 'trunc'), (dict(trunc=NAN), 'trunc'), (dict(max_weight=0.0), 'max_weight'), (dict(max_weight=NAN), 'max_weight')):
        args = dict(origin=(0.0, 0.0, 0.0), voxel=0.1, dims=(8, 8, 8))
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            TsdfVolume(**args)
    v = _volume()
    for kw, word in ((dict(volume=None), 'TsdfVolume'), (dict(depths=D[0]), r'\[n, H, W\]'), (dict(depths=D.astype(np.float64)), 'float32'),
                     (dict(Ks=np.eye(4)), r'\[3, 3\]'), (dict(Ks=np.stack([K] * 3)), r'\[3, 3\]'), (dict(Ks=np.diag([0.0, 1.0, 1.0])), 'focal'),
                     (dict(c2ws=C[:1]), 'c2ws'), (dict(c2ws=np.stack([np.eye(3)] * 2)), r'\[4, 4\]'), (dict(c2ws=C * NAN), r'\[4, 4\]'),
                     (dict(weights=[1.0]), 'weights'), (dict(weights=[1.0, 0.0]), 'weights'), (dict(weights=[INF, 1.0]), 'weights'),
                     (dict(found=[1, 1, 1]), 'found')):
        args = dict(volume=v, depths=D, Ks=K, c2ws=C)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            integrate_depths(**args)
    for kw, word in ((dict(volume=None), 'TsdfVolume'), (dict(K=np.eye(2)), r'\[3, 3\]'), (dict(K=np.diag([1.0, 0.0, 1.0])), 'focal'),
                     (dict(c2w=np.eye(3)), r'\[4, 4\]'), (dict(c2w=None), r'\[4, 4\]'), (dict(shape=(10,)), 'shape'), (dict(shape=(0, 12)), 'H'),
                     (dict(shape=(10, 1.5)), 'W'), (dict(shape=(1 << 14, (1 << 14) + 1)), '2\\^28'), (dict(near=-1.0), 'near'), (dict(near=NAN), 'near'),
                     (dict(far=0.0), 'far'), (dict(near=2.0, far=2.0), 'far'), (dict(far=INF), 'far'), (dict(step=0.0), 'step'), (dict(step=INF), 'step'),
                     (dict(far=10.0, step=1e-4), '65536')):
        args = dict(volume=v, K=K, c2w=np.eye(4), shape=(10, 12))
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            raycast_volume(**args)
    cap = Capture(None, D[0], K, np.eye(4))
    for kw, word in ((dict(caps=[]), 'at least one'), (dict(caps=[cap._replace(depth=D[0].astype(np.float64))]), 'float32'),
                     (dict(caps=[cap._replace(K=np.eye(2))]), r'\[3, 3\]'), (dict(caps=[cap._replace(c2w=None)]), r'\[4, 4\]'),
                     (dict(caps=[cap, cap], weights=[1.0]), 'weights'), (dict(volume=None), 'origin, voxel and dims'),
                     (dict(volume=None, origin=(0, 0, 0), voxel=0.1), 'origin, voxel and dims'), (dict(voxel=0.1), 'not both'),
                     (dict(trunc=0.3), 'not both'), (dict(volume=None, origin=(0, 0, 0), voxel=0.0, dims=(8, 8, 8)), 'voxel'),
                     (dict(volume=None, origin=(0, 0, 0), voxel=0.1, dims=(8, 8, 8), trunc=-1.0), 'trunc')):
        args = dict(caps=[cap], volume=v)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            fuse_captures(**args)
    for kw, word in ((dict(max_dist=0.0), 'max_dist'), (dict(iters=65), 'iters'), (dict(stride=0), 'stride'), (dict(normal_cos=2.0), 'normal_cos'),
                     (dict(c2w0=np.eye(3)), r'\[4, 4\]'), (dict(c2w0=None), r'\[4, 4\]'), (dict(cap=cap._replace(depth=np.ones((2, 12), np.float32))), '3 x 3'),
                     (dict(cap=cap._replace(K=np.diag([0.0, 1.0, 1.0]))), 'focal'), (dict(step=0.0), 'step'), (dict(far=-1.0), 'far'),
                     (dict(volume=None), 'TsdfVolume')):
        args = dict(volume=v, cap=cap, c2w0=np.eye(4))
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            track_capture(**args)
    with pytest.raises(TypeError, match='unexpected keyword'):
        track_capture(v, cap, np.eye(4), max_dst=1.0)


def test_the_default_far_reaches_the_farthest_corner():
    v = _volume()
    assert np.array_equal(v.corners()[0], np.zeros(3)) and np.allclose(v.corners()[7], [0.7, 0.7, 0.7]) and len({tuple(c) for c in v.corners()}) == 8
    from cotr_amd.inference import tsdf
    m = np.eye(4)
    m[:3, 3] = (-1.0, 0.35, 0.35)
    _, H, W, near, far, step = tsdf._ray_args(v, m, (10, 12), None, None, None)
    assert (H, W, near, step) == (10, 12, 0.0, 0.15) and abs(far - np.sqrt(1.7 ** 2 + 2 * 0.35 ** 2)) < 1e-12


def test_cpu_tensors_are_refused():
    v = _volume()
    for kw in (dict(depths=torch.ones((2, 10, 12))), dict(c2ws=torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)),
               dict(found=torch.ones(2, dtype=torch.int32))):
        args = dict(volume=v, depths=D, Ks=K, c2ws=C)
        args.update(kw)
        with pytest.raises(_lib.CotrHipError, match='MI355X only'):
            integrate_depths(**args)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        raycast_volume(v, K, torch.eye(4, dtype=torch.float64), (10, 12))
    cap = Capture(None, torch.ones((10, 12)), K, np.eye(4))
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        fuse_captures([cap], v)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        track_capture(v, cap, np.eye(4))


def test_zoom_engine_fuse_registers_against_the_first_capture_and_fuses_what_it_placed(monkeypatch):
    from cotr_amd.inference import ZoomEngine, tsdf
    placed = {'b': np.eye(4) * 2, 'c': None, 'd': np.eye(4) * 3}
    calls, fused = [], []
    monkeypatch.setattr(tsdf, 'fuse_captures', lambda caps, volume: fused.append((caps, volume)))

    class Spy(ZoomEngine):
        def __init__(self):
            pass

        def register(self, cap_a, cap_b, **kw):
            calls.append((cap_a.image, cap_b.image, kw))
            return placed[cap_b.image], 'corrs', 'mask'
    caps = [Capture(n, 'depth', 'K', np.eye(4) if n == 'a' else None) for n in 'abcd']
    volume, poses, found = Spy().fuse(caps, 'volume', icp_iters=4, seed=1)
    assert volume == 'volume' and found == [True, True, False, True] and poses[2] is None
    assert calls == [('a', n, dict(icp_iters=4, seed=1)) for n in 'bcd']
    (got, vol), = fused
    assert vol == 'volume' and [c.image for c in got] == ['a', 'b', 'd'] and all(np.array_equal(c.c2w, p) for c, p in zip(got, (poses[0], poses[1], poses[3])))
