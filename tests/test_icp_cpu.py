"""The dense point-to-plane ICP without a GPU: the numpy restatement (tests/icp_oracle.py) against its scenes - convergence to a
plateau, the stops on one and two planes and below 6 pairs, the Jacobian against central differences, the order noise behind
the GPU tests' bound - and the argument checks of the C ABI (they run before any HIP call) and of the Python wrappers."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.build import declared_symbols
from cotr_amd.inference import icp_depth, refine_registration, register_captures
from cotr_amd.inference.rigid3d import register_captures_tensors
from tests import icp_oracle as io
from tests import pnp_oracle as po

NAMES = ['cotr_icp_depth_scratch_bytes', 'cotr_icp_depth']


def _run(sc, iters, **kw):
    return io.icp(sc['maps_a'], sc['K_a'], sc['maps_b'], sc['R0'], sc['t0'], iters=iters, **kw)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_maps_are_the_lift_of_every_pixel_centre_with_unit_normals_towards_the_camera():
    sc = io.corner_scene()
    H, W = sc['depth_b'].shape
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    V = po.lift(np.stack([xs.ravel(), ys.ravel()], 1), sc['depth_b'], sc['K_b']).reshape(H, W, 3)
    m = sc['maps_b']
    assert np.array_equal(m[..., :3], V)
    n = m[1:-1, 1:-1, 3:]
    assert np.isnan(m[0, :, 3:]).all() and np.isnan(m[-1, :, 3:]).all() and np.isnan(m[:, 0, 3:]).all() and np.isnan(m[:, -1, 3:]).all()
    assert np.isfinite(n).all() and np.abs(np.linalg.norm(n, axis=-1) - 1).max() < 1e-15 and ((n * m[1:-1, 1:-1, :3]).sum(-1) <= 0).all()
    # away from the two creases the normal is a plane's own, in B's camera frame
    planes = np.array([np.asarray(p, np.float64) / np.linalg.norm(p) for p, _ in io.PLANES]) @ sc['c2w_b'][:3, :3]
    cos = np.abs(n @ planes.T).max(-1)
    assert (cos > 1 - 1e-6).mean() > 0.95   # float32 depths: 5e-7 of a 0.05 step between neighbours
    # a hole takes the vertex of its pixel and the normals of the pixel and its four neighbours; a depth step takes the normal
    d = sc['depth_b'].copy()
    d[40, 50], d[60, 70] = 0.0, d[60, 70] * 1.2
    h = io.maps(d, sc['K_b'])
    gone = np.isnan(h[..., 3]) & ~np.isnan(m[..., 3])
    want = np.zeros((H, W), bool)
    for (y, x) in ((40, 50), (60, 70)):
        want[y, x] = want[y - 1, x] = want[y + 1, x] = want[y, x - 1] = want[y, x + 1] = True
    assert np.array_equal(gone, want) and np.isnan(h[40, 50, :3]).all() and np.isfinite(h[60, 70, :3]).all()


def test_convergence_to_a_plateau_on_the_corner():
    sc = io.corner_scene()
    r = _run(sc, 20)
    start, end = io.errors(sc['R0'], sc['t0'], sc), io.errors(r['R'], r['t'], sc)
    print(f'start {start[0]:.3e} / {start[1]:.3e}, after 20 steps {end[0]:.3e} / {end[1]:.3e}, {r["info"][2]} pairs, rmse {r["stats"][1]:.3e}')
    assert list(r['info'][:4]) == [1, 20, r['info'][2], 0] and len(r['poses']) == 21
    # the plateau: from the fifth evaluation on the pose moves by rounding only (the pairs no longer change, and a
    # Gauss-Newton iteration on fixed pairs contracts to its fixed point)
    for k in range(5, 21):
        assert io.pose_distance(*r['poses'][k], r['R'], r['t']) < 1e-12, k
    assert np.array_equal(_run(sc, 5)['assoc'], r['assoc'])
    # and it is a registration: an order of magnitude nearer than the start in both parts
    assert end[0] < 0.1 * start[0] and end[1] < 0.1 * start[1]
    ratio = r['hist'][:20, 29] / r['hist'][:20, 30]
    assert (ratio > 1e-3).all() and (ratio < 1e-2).all()


@pytest.mark.parametrize('planes', [1, 2])
def test_fewer_than_three_planes_stop_as_ill_conditioned_and_leave_the_start(planes):
    sc = io.scene(96, 128, 96, 128, planes)
    r = _run(sc, 5)
    ratio = r['hist'][0, 29] / r['hist'][0, 30]
    print(f'{planes} plane(s): l_min / l_max = {ratio:.2e}, {r["info"][2]} pairs')
    assert list(r['info'][:4]) == [0, 0, r['info'][2], 2] and r['info'][2] > 10000
    assert np.array_equal(r['R'], sc['R0']) and np.array_equal(r['t'], sc['t0'])
    assert ratio < 1e-7 and (r['hist'][1:] == 0).all()
    # the pivot test of the sparse refits would have let the single plane through, which is why it is not the rule here
    assert planes == 2 or ratio < 1e-11


@pytest.mark.parametrize('keep', [0, 5, 6])
def test_fewer_than_6_pairs_stop(keep):
    sc = io.corner_scene()
    first = io.evaluate(sc['maps_a'], sc['K_a'], sc['maps_b'], sc['R0'], sc['t0'])
    mask = np.zeros(sc['depth_b'].shape, np.uint8)
    mask.reshape(-1)[np.flatnonzero(first['pairs'])[:: 1500][:keep]] = 1
    r = _run(sc, 0, src_mask=mask)
    assert r['info'][2] == keep and r['info'][4] == keep and r['info'][3] == (1 if keep < 6 else 0)
    r = _run(sc, 3, src_mask=mask)
    assert (r['info'][3] == 1) == (keep < 6)
    if keep < 6:
        assert list(r['info'][:5]) == [0, 0, keep, 1, keep] and np.array_equal(r['R'], sc['R0']) and np.array_equal(r['t'], sc['t0'])


def test_jacobian_is_the_central_difference_of_the_residual_at_fixed_pairs():
    sc = io.corner_scene()
    R, t = sc['R0'], sc['t0']
    e = io.evaluate(sc['maps_a'], sc['K_a'], sc['maps_b'], R, t)
    idx = np.flatnonzero(e['pairs'])[::97]
    X = io.source(sc['maps_b'])[0][idx]
    A = sc['maps_a'].reshape(-1, 6)[e['assoc'][idx]]

    def residual(d):
        Rd, td = io.apply(R, t, d)
        return ((X @ Rd.T + td - A[:, :3]) * A[:, 3:]).sum(1)
    assert np.abs(residual(np.zeros(6)) - e['r'][idx]).max() < 1e-14
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        num = (residual(d) - residual(-d)) / (2 * h)
        assert np.abs(num - e['J'][idx, k]).max() < 1e-8 * max(1.0, np.abs(e['J'][idx, k]).max()), k


def test_order_noise_and_no_pixel_near_a_decision():
    cases = io.solving_cases()
    # the sweep: the maps up to 8 x 8, 5 x 13 and 3 x 683 see one plane (or hold fewer than 6 pairs) and do not solve, every other does
    assert [c[2:] for c in cases if c[:2] == (96, 128)] == [(16, 16), (23, 89), (32, 64), (17, 241), (80, 100), (96, 128)]
    assert [c[2:] for c in cases if c[:2] == (24, 32)] == list(io.SIZES_B_SMALL_A)
    worst = 0.0
    for c in cases:
        sc = io.scene(*c, 3, io.SWEEP_EDGE)
        worst = max(worst, io.order_noise(sc))
        assert not _run(sc, 3)['near'].any(), c
    sc = io.corner_scene()
    for stride in (1, 2, 3):
        worst = max(worst, io.order_noise(sc, stride=stride))
    print(f'order noise of one step: {worst:.3e} (at 96 x 128: {io.order_noise(sc):.3e})')
    assert worst <= io.ORDER_NOISE and io.STEP_BOUND == 1000 * io.ORDER_NOISE
    assert worst > io.ORDER_NOISE / 100   # the bound is the noise measured, not a round number far above it


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and name in declared_symbols()
        assert getattr(_lib.load_library(), name) is not None


def test_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    b = ctypes.c_size_t()
    P = ctypes.c_void_p(4096)           # never dereferenced: every call below fails its checks before any HIP call
    for shape in ((2, 3, 3, 3), (3, 2, 3, 3), (3, 3, 2, 3), (3, 3, 3, 2), (1 << 14, (1 << 14) + 1, 3, 3), (3, 3, (1 << 14) + 1, 1 << 14)):
        assert lib.cotr_icp_depth_scratch_bytes(*shape, 1, ctypes.byref(b)) == -1 and b'2^28' in lib.cotr_raster_last_error()
    for stride in (0, 65):
        assert lib.cotr_icp_depth_scratch_bytes(96, 128, 96, 128, stride, ctypes.byref(b)) == -1 and b'stride' in lib.cotr_raster_last_error()
    assert lib.cotr_icp_depth_scratch_bytes(96, 128, 96, 128, 1, None) == -1 and b'NULL' in lib.cotr_raster_last_error()
    assert lib.cotr_icp_depth_scratch_bytes(1 << 14, 1 << 14, 3, 3, 64, ctypes.byref(b)) == 0 and b.value >= 48 << 28
    assert lib.cotr_icp_depth_scratch_bytes(96, 128, 96, 128, 1, ctypes.byref(b)) == 0
    need = b.value
    assert need >= 2 * 96 * 128 * 48 + 6 * 29 * 8 + 96 * 128
    assert lib.cotr_icp_depth_scratch_bytes(96, 128, 96, 128, 3, ctypes.byref(b)) == 0 and b.value < need
    K = (ctypes.c_double * 9)(100.0, 0.5, 64.0, 0.0, 100.0, 48.0, 0.0, 0.0, 1.0)

    def bad_k(i, v):
        k = (ctypes.c_double * 9)(*K)
        k[i] = v
        return k

    def call(Ha=96, Wa=128, Hb=96, Wb=128, da=P, db=P, Ka=K, Kb=K, R0=P, t0=P, c2w=None, found=None, mask=None, max_dist=0.25, normal_cos=0.5,
             edge=0.05, cond_tol=1e-6, iters=10, stride=1, R=P, t=P, info=P, stats=P, hist=None, assoc=None, ma=None, mb=None, scratch=P,
             nbytes=need):
        return lib.cotr_icp_depth(da, Ha, Wa, Ka, db, Hb, Wb, Kb, R0, t0, c2w, found, mask, max_dist, normal_cos, edge, cond_tol, iters, stride,
                                  R, t, info, stats, hist, assoc, ma, mb, scratch, nbytes, None)
    nan, inf = float('nan'), float('inf')
    odd8, odd4 = ctypes.c_void_p(4100), ctypes.c_void_p(4098)
    for kw, word in ((dict(Ha=2), b'2^28'), (dict(Wa=2), b'2^28'), (dict(Hb=2), b'2^28'), (dict(Wb=2), b'2^28'),
                     (dict(Ha=1 << 14, Wa=(1 << 14) + 1), b'2^28'), (dict(Hb=(1 << 14) + 1, Wb=1 << 14), b'2^28'),
                     (dict(stride=0), b'stride'), (dict(stride=65), b'stride'), (dict(iters=-1), b'iters'), (dict(iters=65), b'iters'),
                     (dict(max_dist=0.0), b'max_dist'), (dict(max_dist=-1.0), b'max_dist'), (dict(max_dist=inf), b'max_dist'),
                     (dict(max_dist=nan), b'max_dist'), (dict(normal_cos=-1.5), b'normal_cos'), (dict(normal_cos=1.5), b'normal_cos'),
                     (dict(normal_cos=nan), b'normal_cos'), (dict(edge=0.0), b'edge'), (dict(edge=inf), b'edge'), (dict(edge=nan), b'edge'),
                     (dict(cond_tol=0.0), b'cond_tol'), (dict(cond_tol=1.0), b'cond_tol'), (dict(cond_tol=nan), b'cond_tol'),
                     (dict(da=None), b'NULL'), (dict(db=None), b'NULL'), (dict(Ka=None), b'NULL'), (dict(Kb=None), b'NULL'),
                     (dict(R0=None), b'NULL'), (dict(t0=None), b'NULL'), (dict(R=None), b'NULL'), (dict(t=None), b'NULL'),
                     (dict(info=None), b'NULL'), (dict(stats=None), b'NULL'), (dict(scratch=None), b'NULL'),
                     (dict(Ka=bad_k(0, 0.0)), b'focal'), (dict(Kb=bad_k(4, 0.0)), b'focal'), (dict(Ka=bad_k(2, nan)), b'focal'),
                     (dict(Kb=bad_k(1, inf)), b'focal'),
                     (dict(da=odd4), b'aligned'), (dict(db=odd4), b'aligned'), (dict(R0=odd8), b'aligned'), (dict(t0=odd8), b'aligned'),
                     (dict(c2w=odd8), b'aligned'), (dict(found=odd4), b'aligned'), (dict(R=odd8), b'aligned'), (dict(t=odd8), b'aligned'),
                     (dict(info=odd4), b'aligned'), (dict(stats=odd8), b'aligned'), (dict(hist=odd8), b'aligned'), (dict(assoc=odd4), b'aligned'),
                     (dict(ma=odd8), b'aligned'), (dict(mb=odd8), b'aligned'), (dict(scratch=ctypes.c_void_p(4104)), b'aligned'),
                     (dict(nbytes=need - 1), b'smaller')):
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())
        assert b'cotr_icp_depth' in lib.cotr_raster_last_error()


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
K = np.array([[100.0, 0.5, 6.0], [0.0, 100.0, 5.0], [0.0, 0.0, 1.0]])
D = np.ones((10, 12), np.float32)


def _capture(depth=None, K_=K, c2w=None):
    from cotr_amd.data import Capture
    return Capture(None, D if depth is None else depth, K_, np.eye(4) if c2w is None else c2w)


def test_wrapper_argument_errors_without_a_gpu():
    R, t = np.eye(3), np.zeros(3)
    for kw, word in ((dict(max_dist=0.0), 'max_dist'), (dict(max_dist=float('inf')), 'max_dist'), (dict(max_dist=float('nan')), 'max_dist'),
                     (dict(normal_cos=1.5), 'normal_cos'), (dict(normal_cos=-1.5), 'normal_cos'), (dict(edge=0.0), 'edge'),
                     (dict(edge=float('inf')), 'edge'), (dict(cond_tol=0.0), 'cond_tol'), (dict(cond_tol=1.0), 'cond_tol'),
                     (dict(iters=-1), 'iters'), (dict(iters=65), 'iters'), (dict(iters=1.5), 'iters'), (dict(stride=0), 'stride'),
                     (dict(stride=65), 'stride'), (dict(stride=1.5), 'stride'), (dict(src_mask=np.ones((10, 11), np.uint8)), 'src_mask'),
                     (dict(src_mask=np.ones((10, 12), np.float32)), 'src_mask'), (dict(c2w_a=np.eye(3)), r'\[4, 4\]'),
                     (dict(depth_a=np.ones((10, 12))), 'float32'), (dict(depth_b=np.ones((10, 12))), 'float32'),
                     (dict(depth_a=np.ones((2, 12), np.float32)), '3 x 3'), (dict(depth_b=np.ones((10, 2), np.float32)), '3 x 3'),
                     (dict(K_a=np.diag([0.0, 1.0, 1.0])), 'focal'), (dict(K_b=np.eye(4)), r'\[3, 3\]'), (dict(R0=np.eye(4)), 'R0'),
                     (dict(t0=np.zeros(4)), 't0')):
        args = dict(depth_a=D, K_a=K, depth_b=D, K_b=K, R0=R, t0=t, max_dist=0.1)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            icp_depth(**args)
    for kw, word in ((dict(max_dist=0.0), 'max_dist'), (dict(iters=65), 'iters'), (dict(stride=0), 'stride'), (dict(normal_cos=2.0), 'normal_cos')):
        with pytest.raises(ValueError, match=word):
            refine_registration(_capture(), _capture(), np.eye(4), **kw)
    with pytest.raises(ValueError, match=r'\[4, 4\]'):
        refine_registration(_capture(), _capture(), np.eye(3))
    with pytest.raises(ValueError, match=r'\[4, 4\]'):
        refine_registration(_capture(), _capture(), None)
    with pytest.raises(TypeError, match='unexpected keyword'):
        refine_registration(_capture(), _capture(), np.eye(4), max_dst=1.0)
    p = np.zeros((20, 2))
    for kw, word in ((dict(icp_iters=-1), 'icp_iters'), (dict(icp_iters=65), 'icp_iters'), (dict(icp_iters=1.5), 'icp_iters'),
                     (dict(icp_iters=3, with_scale=True), 'with_scale'), (dict(icp_iters=3, icp_max_dist=0.0), 'max_dist'),
                     (dict(icp_iters=3, icp_max_dist=float('inf')), 'max_dist')):
        with pytest.raises(ValueError, match=word):
            register_captures(p, p, _capture(), _capture(), **kw)
        with pytest.raises(ValueError, match=word):
            register_captures_tensors(p, p, D, K, None, D, K, **kw)
    with pytest.raises(ValueError, match='3 x 3'):
        register_captures(p, p, _capture(depth=np.ones((2, 12), np.float32)), _capture(), icp_iters=3)


def test_cpu_tensors_are_refused():
    R, t = np.eye(3), np.zeros(3)
    for kw in (dict(depth_a=torch.ones((10, 12))), dict(depth_b=torch.ones((10, 12))), dict(R0=torch.eye(3, dtype=torch.float64)),
               dict(t0=torch.zeros(3, dtype=torch.float64)), dict(src_mask=torch.ones((10, 12), dtype=torch.uint8))):
        args = dict(depth_a=D, K_a=K, depth_b=D, K_b=K, R0=R, t0=t, max_dist=0.1)
        args.update(kw)
        with pytest.raises(_lib.CotrHipError, match='MI355X only'):
            icp_depth(**args)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        refine_registration(_capture(depth=torch.ones((10, 12))), _capture(), np.eye(4))
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        register_captures(np.zeros((20, 2)), np.zeros((20, 2)), _capture(), _capture(depth=torch.ones((10, 12))), icp_iters=3)


def test_zoom_engine_register_hands_the_icp_arguments_on(monkeypatch):
    from cotr_amd.data import Capture
    from cotr_amd.inference import ZoomEngine, rigid3d
    want = np.random.default_rng(0).uniform(0, 100, (12, 4))
    calls = []
    monkeypatch.setattr(rigid3d, 'register_captures', lambda pa, pb, cap_a, cap_b, **kw: calls.append(kw) or ('c2w', 'mask'))

    class Spy(ZoomEngine):
        def __init__(self):
            pass

        def cotr_corr_multiscale(self, *a, **kw):
            return want
    c2w, corrs, mask = Spy().register(Capture('a', 'depth', 'K', 'c2w'), Capture('b', 'depth', 'K', None), icp_iters=10, icp_max_dist=0.2, seed=1)
    assert (c2w, mask) == ('c2w', 'mask') and calls == [dict(icp_iters=10, icp_max_dist=0.2, seed=1)]
