"""The bundle adjustment rules of DESIGN.md 3h-7 without a GPU: the numpy restatement tests/bundle_oracle.py against central
differences, against a dense solve of the full normal system and against scipy's least squares on the same residuals; its cost
over kept and rejected steps, the freeze and landmark rules, the cases that take no step, the order noise of its sums (the
constants the GPU test is held to), and every argument error of the C ABI and of the wrappers."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.build import declared_symbols
from cotr_amd.inference import bundle_adjust, bundle_adjust_tensors
from cotr_amd.inference.structure import reconstruct_tensors
from tests import bundle_oracle as bo
from tests import structure_oracle as so

# V, N, noise px, outlier views: the rows of the feasibility table of 3h-7
ROWS = {(3, 12): (0.0, 0.0), (3, 64): (0.0, 0.0), (4, 65): (0.5, 0.0), (5, 257): (0.7, 0.0), (8, 1025): (0.7, 0.25), (32, 65): (0.7, 0.25)}


@functools.lru_cache(maxsize=None)
def fixture(V, N):
    return bo.fixture(V, N, *ROWS[(V, N)])


def run(fx, **kw):
    a = dict(visible=fx['used'], fixed_views=fx['fixed'], iters=15)
    a.update(kw)
    return bo.bundle_adjust(fx['points'], fx['cams'], fx['poses0'], fx['X0'], **a)


def first_round(fx, lam=1e-3):
    """the state, set and flags the first iteration of a call sees"""
    V, N = fx['points'].shape[:2]
    fixed = np.zeros(V, bool)
    fixed[list(fx['fixed'])] = True
    tab = bo.table(fx['cams'], fx['poses0'])
    pix = so.f32(fx['points'])
    sets, frozen, landmark, _, _ = bo.select(tab, pix, fx['used'] != 0, fx['X0'], fixed, True, np.float32(16.0), 50.0)
    return dict(tab=tab, pix=pix, sets=sets, landmark=landmark, free=~fixed & ~frozen, X=fx['X0'], lam=lam)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


# ---- the Jacobians --------------------------------------------------------------------------------------------------------
def test_jacobians_against_central_differences():
    # central differences with h = 1e-6 on residuals of up to a few hundred pixels: rounding 2^-52 |f| / h ~ 1e-7, truncation
    # h^2 f''' / 6 ~ 1e-10; the entries are of the order fx / z ~ 100, so 1e-5 absolute is 100 times the rounding
    fx = fixture(3, 12)
    h, tol = 1e-6, 1e-5
    pix = so.f32(fx['points'])
    X = fx['X0']
    for v in range(3):
        u, w = pix[v, :, 0], pix[v, :, 1]

        def res(poses, Xs):
            r = so.project(bo.table(fx['cams'], poses), v, u, w, [Xs[:, 0], Xs[:, 1], Xs[:, 2]])
            return np.stack([r['du'], r['dv']])
        _, cu, cv, pu, pv = bo.observe(bo.table(fx['cams'], fx['poses0']), v, u, w, [X[:, 0], X[:, 1], X[:, 2]])
        for k in range(3):
            d = np.zeros(3)
            d[k] = h
            num = (res(fx['poses0'], X + d) - res(fx['poses0'], X - d)) / (2 * h)
            assert np.abs(num[0] - pu[k]).max() <= tol and np.abs(num[1] - pv[k]).max() <= tol
        for k in range(6):
            def moved(sign):
                P = fx['poses0'].reshape(-1, 3, 4).copy()
                d = np.zeros(6)
                d[k] = sign * h
                P[v, :, :3] = so.rotation(d[:3]) @ P[v, :, :3]
                P[v, :, 3] += d[3:]
                return P.reshape(-1, 12)
            num = (res(moved(1), X) - res(moved(-1), X)) / (2 * h)
            assert np.abs(num[0] - cu[k]).max() <= tol and np.abs(num[1] - cv[k]).max() <= tol, (v, k)


# ---- the Schur step against the full system -------------------------------------------------------------------------------
def test_schur_step_against_the_dense_normal_system():
    worst = 0.0
    for shape in ((3, 12), (4, 65)):
        for lam in (1e-3, 1e3):
            s = first_round(fixture(*shape), lam)
            sys = bo.reduced_system(s['tab'], s['pix'], s['sets'], s['landmark'], s['free'], s['X'], lam)
            dc = bo.cholesky_solve(sys['S'], sys['b'])
            dX = bo.back_substitute(sys, s['sets'], dc)
            dc2, dX2, moves = bo.dense_step(s['tab'], s['pix'], s['sets'], s['landmark'], s['free'], s['X'], lam)
            assert np.array_equal(moves, sys['moves']) and moves.all()
            worst = max(worst, rel(dc, dc2), rel(dX, dX2))
    print(f'Schur step against the dense solve: largest relative difference {worst:.3e}')
    assert worst <= bo.SCHUR_ROUTES


# ---- the cost over the iterations -----------------------------------------------------------------------------------------
def test_cost_falls_over_kept_steps_and_stays_over_rejected_ones():
    for shape in ((3, 64), (4, 65), (5, 257)):
        trace = []
        r = run(fixture(*shape), trace=trace)
        assert len(trace) == 15 and r['info'][5] + r['info'][6] == 15 and r['info'][5] == sum(t['kept'] for t in trace) > 0
        assert any(not t['kept'] for t in trace)
        for t, nxt in zip(trace, trace[1:] + [dict(cost=r['stats'][1], lam=r['stats'][2])]):
            if t['kept']:
                assert t['cand'] < t['cost'] and nxt['cost'] == t['cand'] and nxt['lam'] == max(t['lam'] / 10, 1e-12)
            else:
                assert nxt['cost'] == t['cost'] and nxt['lam'] == 10 * t['lam']


def test_lambda_above_the_limit_ends_the_round():
    # once converged nearly every step is rejected and lambda climbs by 10 a time: past 1e12 the round is over before its 64 iterations
    trace = []
    r = run(fixture(3, 12), iters=64, trace=trace)
    assert len(trace) < 64 and not trace[-1]['kept'] and trace[-1]['lam'] <= 1e12 < r['stats'][2]
    assert r['info'][5] + r['info'][6] == len(trace)


# ---- the final cost against scipy -----------------------------------------------------------------------------------------
def _scipy_cost(fx, r0):
    from scipy.optimize import least_squares
    V, N = fx['points'].shape[:2]
    sets, free, moving = r0['used'] != 0, np.flatnonzero(~r0['frozen'] & ~np.isin(np.arange(V), fx['fixed'])), np.flatnonzero(~r0['landmark'])
    vi, pi = np.nonzero(sets)
    pix = so.f32(fx['points'])[vi, pi]
    k = fx['cams'][vi]
    P0 = fx['poses0'].reshape(V, 3, 4)

    def residuals(x):
        R, t, X = P0[:, :, :3].copy(), P0[:, :, 3].copy(), fx['X0'].copy()
        for s, v in enumerate(free):
            d = x[6 * s:6 * s + 6]
            R[v], t[v] = so.rotation(d[:3]) @ P0[v, :, :3], P0[v, :, 3] + d[3:]
        X[moving] = x[6 * len(free):].reshape(-1, 3)
        Y = np.einsum('oij,oj->oi', R[vi], X[pi]) + t[vi]
        xn, yn = Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2]
        return np.concatenate([k[:, 0] * xn + k[:, 4] * yn + k[:, 2] - pix[:, 0], k[:, 1] * yn + k[:, 3] - pix[:, 1]])
    x0 = np.concatenate([np.zeros(6 * len(free)), fx['X0'][moving].reshape(-1)])
    sol = least_squares(residuals, x0, method='trf', x_scale='jac', ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=200)
    return 2.0 * sol.cost


@pytest.mark.parametrize('shape', [(3, 12), (3, 64), (4, 65), (5, 257), (32, 65)])
def test_final_cost_against_scipy(shape):
    fx = fixture(*shape)
    r = run(fx)
    ref = _scipy_cost(fx, r)
    print(f'{shape}: cost {r["stats"][0]:.6g} -> {r["stats"][1]:.10g}, scipy {ref:.10g}, relative {abs(r["stats"][1] - ref) / ref:.2e}')
    assert r['stats'][1] < r['stats'][0]
    if ref < 1e-6:
        assert r['stats'][1] < 1e-6
    else:
        assert abs(r['stats'][1] - ref) <= 1e-6 * ref


def test_quality_of_the_restatement():
    # the worst pose error falls below a tenth of its start on the noisy rows the device is compared on
    for shape in ((5, 257), (8, 1025)):
        fx = fixture(*shape)
        r = run(fx)
        e0, e1 = bo.pose_errors(fx['poses0'], fx['sc']['poses']), bo.pose_errors(r['poses'], fx['sc']['poses'])
        print(f'{shape}: rotation {e0[0]:.3g} -> {e1[0]:.3g} deg, centre {e0[1]:.3g} -> {e1[1]:.3g}')
        assert e1[0] < 0.1 * e0[0]


# ---- frozen views and landmarks -------------------------------------------------------------------------------------------
def test_starved_views_are_frozen_and_keep_their_bits():
    fx = fixture(32, 65)
    r = run(fx)
    assert list(np.flatnonzero(r['frozen'])) == [6, 19, 23] and list(fx['used'].sum(axis=1)[[6, 19, 23]]) == [1, 2, 0]
    assert r['info'][2] == 27 and r['info'][3] == 3 and r['info'][5] > 0
    for v in range(32):
        same = np.array_equal(r['poses'][v].view(np.uint64), fx['poses0'][v].view(np.uint64))
        assert same == (v in (0, 1, 6, 19, 23)), v
    assert not r['used'][[6, 19, 23]].any() and r['info'][1] == r['used'].sum()


def test_a_point_seen_once_is_a_landmark():
    fx = dict(fixture(4, 65))
    vis = fx['used'].copy()
    vis[:, 5] = 0
    vis[2, 5] = 1            # a free view alone sees point 5
    r = run(fx, visible=vis)
    assert r['landmark'][5] and r['landmark'].sum() == 1 and r['info'][4] == 1 and r['used'][2, 5] == 1
    assert np.array_equal(r['X'][5].view(np.uint64), fx['X0'][5].view(np.uint64))
    moved = np.flatnonzero((r['X'] != fx['X0']).any(axis=1))
    assert len(moved) == 64 and 5 not in moved and r['info'][5] > 0


# ---- no step --------------------------------------------------------------------------------------------------------------
def test_calls_that_take_no_step_return_the_input_bits():
    fx = fixture(4, 65)
    r = run(fx, iters=0)
    assert np.array_equal(r['poses'].view(np.uint64), fx['poses0'].view(np.uint64)) and np.array_equal(r['X'].view(np.uint64), fx['X0'].view(np.uint64))
    assert list(r['info']) == [1, 260, 2, 0, 0, 0, 0, 1] and r['stats'][0] == r['stats'][1] > 0 and r['stats'][2] == 1e-3
    assert np.array_equal(r['used'], fx['used'])
    one = dict(points=fx['points'][:, :1], cams=fx['cams'], poses0=fx['poses0'], X0=fx['X0'][:1], used=fx['used'][:, :1], fixed=(0, 1))
    r = run(one, rounds=2)      # N = 1: every free view is starved
    assert np.array_equal(r['poses'].view(np.uint64), one['poses0'].view(np.uint64)) and np.array_equal(r['X'].view(np.uint64), one['X0'].view(np.uint64))
    assert list(r['info']) == [1, 2, 0, 2, 0, 0, 0, 2] and list(r['used'][:, 0]) == [1, 1, 0, 0]
    r = run(fx, found=0)
    assert not r['poses'].any() and not r['X'].any() and not r['used'].any() and not r['stats'].any() and not r['info'].any()


# ---- the order of the sums ------------------------------------------------------------------------------------------------
def test_order_noise():
    sums = step = full = 0.0
    for shape in ((3, 64), (4, 65), (5, 257), (8, 1025), (32, 65)):
        fx = fixture(*shape)
        s = first_round(fx)
        up = bo.reduced_system(s['tab'], s['pix'], s['sets'], s['landmark'], s['free'], s['X'], s['lam'], 'asc')
        down = bo.reduced_system(s['tab'], s['pix'], s['sets'], s['landmark'], s['free'], s['X'], s['lam'], 'desc')
        cu, cd = bo.cost(s['tab'], s['pix'], s['sets'], s['X'], 'asc')[0], bo.cost(s['tab'], s['pix'], s['sets'], s['X'], 'desc')[0]
        sums = max(sums, rel(up['S'], down['S']), rel(up['b'], down['b']), abs(cu - cd) / cd)
        for iters in (1, 15):
            a, b = run(fx, iters=iters, order='asc'), run(fx, iters=iters, order='desc')
            assert np.array_equal(a['used'], b['used']) and np.array_equal(a['info'][:5], b['info'][:5])
            d = max(rel(a['poses'], b['poses']), rel(a['X'], b['X']), abs(a['stats'][1] - b['stats'][1]) / b['stats'][1])
            if iters == 1:
                step = max(step, d)
            else:
                full = max(full, d)
    # the fixtures the device is compared on after one iteration (tests/test_bundle_gpu.py) lie under the same constant
    extra = [(bo.big_fixture(N), 1e-3) for N in (65, 257)] + [(bo.step_fixture(V, N), lam) for V in (2, 3, 5) for N in (4, 65, 257, 2049)
                                                             for lam in (1e-3, 1e3)]
    extra.append((bo.repeated_fixture(), 1e3))        # well conditioned at this damping (at 1e-3 it stands on the damping alone)
    for fx, lam in extra:
        a, b = run(fx, iters=1, lambda0=lam, order='asc'), run(fx, iters=1, lambda0=lam, order='desc')
        assert np.array_equal(a['used'], b['used']) and np.array_equal(a['info'], b['info'])
        step = max(step, rel(a['poses'], b['poses']), rel(a['X'], b['X']), abs(a['stats'][1] - b['stats'][1]) / b['stats'][1])
    print(f'ascending against descending sums: S, b and cost {sums:.3e}, poses and X after one iteration {step:.3e}, after a run {full:.3e}')
    assert sums <= bo.ORDER_NOISE_SUMS and step <= bo.ORDER_NOISE_STEP and full <= bo.ORDER_NOISE_RUN


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
NAMES = ('cotr_bundle_adjust', 'cotr_bundle_adjust_scratch_bytes')


def test_symbols_are_declared_and_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and name in declared_symbols()
        assert getattr(_lib.load_library(), name) is not None


def test_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    b = ctypes.c_size_t()
    P = ctypes.c_void_p(4096)           # never dereferenced: every call below fails its checks before any HIP call
    for V, n, word in ((1, 10, b'[2, 32]'), (33, 10, b'[2, 32]'), (2, 0, b'[1, 2^20]'), (2, (1 << 20) + 1, b'[1, 2^20]')):
        assert lib.cotr_bundle_adjust_scratch_bytes(V, n, ctypes.byref(b)) == -1 and word in lib.cotr_raster_last_error()
    assert lib.cotr_bundle_adjust_scratch_bytes(2, 10, None) == -1 and b'NULL' in lib.cotr_raster_last_error()
    assert lib.cotr_bundle_adjust_scratch_bytes(32, 1 << 20, ctypes.byref(b)) == 0
    assert b.value >= (1 << 20) * (2 * 24 + 4 + 2 + 72) + 512 * 528 * 63 * 8
    assert lib.cotr_bundle_adjust_scratch_bytes(3, 100, ctypes.byref(b)) == 0
    need = b.value
    fixed3 = (ctypes.c_uint8 * 3)

    def call(V=3, n=100, thr=4.0, dist=50.0, rounds=1, iters=10, lam=1e-3, pts=P, vis=None, cams=P, poses=P, X=P, fixed=None, found=None,
             poses_out=P, X_out=P, used=P, stats=P, info=P, scratch=P, nbytes=need):
        return lib.cotr_bundle_adjust(pts, vis, cams, poses, X, fixed, V, n, found, thr, dist, rounds, iters, lam, poses_out, X_out, used, stats,
                                      info, scratch, nbytes, None)
    for kw, word in ((dict(V=1), b'[2, 32]'), (dict(V=33), b'[2, 32]'), (dict(n=0), b'[1, 2^20]'), (dict(n=(1 << 20) + 1), b'[1, 2^20]'),
                     (dict(thr=0.0), b'threshold'), (dict(thr=-1.0), b'threshold'), (dict(thr=float('nan')), b'threshold'),
                     (dict(thr=float('inf')), b'threshold'), (dict(thr=1e30), b'squared threshold'), (dict(thr=1e-30), b'squared threshold'),
                     (dict(dist=0.0), b'distance_thresh'), (dict(dist=float('inf')), b'distance_thresh'), (dict(dist=float('nan')), b'distance_thresh'),
                     (dict(rounds=0), b'rounds'), (dict(rounds=9), b'rounds'), (dict(iters=-1), b'iters'), (dict(iters=65), b'iters'),
                     (dict(lam=0.0), b'lambda0'), (dict(lam=1e-13), b'lambda0'), (dict(lam=1e13), b'lambda0'), (dict(lam=float('nan')), b'lambda0'),
                     (dict(lam=float('inf')), b'lambda0'), (dict(fixed=fixed3(0, 0, 0)), b'must be fixed'), (dict(fixed=fixed3(1, 1, 1)), b'must not be fixed'),
                     (dict(pts=None), b'NULL'), (dict(cams=None), b'NULL'), (dict(poses=None), b'NULL'), (dict(X=None), b'NULL'),
                     (dict(poses_out=None), b'NULL'), (dict(X_out=None), b'NULL'), (dict(used=None), b'NULL'), (dict(stats=None), b'NULL'),
                     (dict(info=None), b'NULL'), (dict(scratch=None), b'NULL'), (dict(pts=ctypes.c_void_p(4104)), b'aligned'),
                     (dict(cams=ctypes.c_void_p(4100)), b'aligned'), (dict(poses=ctypes.c_void_p(4100)), b'aligned'), (dict(X=ctypes.c_void_p(4100)), b'aligned'),
                     (dict(poses_out=ctypes.c_void_p(4100)), b'aligned'), (dict(X_out=ctypes.c_void_p(4100)), b'aligned'),
                     (dict(stats=ctypes.c_void_p(4100)), b'aligned'), (dict(info=ctypes.c_void_p(4098)), b'aligned'),
                     (dict(found=ctypes.c_void_p(4098)), b'aligned'), (dict(scratch=ctypes.c_void_p(4104)), b'aligned'), (dict(nbytes=need - 1), b'smaller')):
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
def test_wrapper_argument_errors_without_a_gpu():
    pts, cams, poses = np.zeros((3, 20, 2)), np.tile([500.0, 500.0, 320.0, 240.0, 0.0], (3, 1)), np.tile(np.eye(3, 4).reshape(12), (3, 1))
    X = np.ones((20, 3))
    for fn in (bundle_adjust_tensors, bundle_adjust):
        for bad, word in ((dict(points=np.zeros((20, 2))), r'\[V, N, 2\]'), (dict(points=np.zeros((1, 20, 2))), 'between 2 and 32 views'),
                          (dict(points=np.zeros((33, 20, 2))), 'between 2 and 32 views'), (dict(points=np.zeros((3, 0, 2))), 'between 1 and'),
                          (dict(points=np.zeros((2, (1 << 20) + 1, 2)), X=np.zeros(((1 << 20) + 1, 3))), '2\\^20 points'),
                          (dict(cameras=cams[:2]), 'cameras must be'), (dict(cameras=np.diag([0.0, 500.0, 1.0])), 'focal'),
                          (dict(poses=poses[:2]), 'poses must be'), (dict(X=np.ones((19, 3))), r'X must be \[N, 3\]'), (dict(X=np.ones((20, 2))), r'X must be \[N, 3\]'),
                          (dict(visible=np.ones((3, 19))), 'visible must be'), (dict(fixed_views=()), 'must be fixed'),
                          (dict(fixed_views=(0, 1, 2)), 'must not be fixed'), (dict(fixed_views=(3,)), 'fixed_views must name'),
                          (dict(fixed_views=(-1,)), 'fixed_views must name'), (dict(fixed_views=np.array([True, False])), 'mask must be'),
                          (dict(fixed_views=np.array([True, True, True])), 'must not be fixed'),
                          (dict(threshold=0.0), 'threshold'), (dict(threshold=float('nan')), 'threshold'), (dict(threshold=1e30), 'squared'),
                          (dict(distance_thresh=0.0), 'distance_thresh'), (dict(distance_thresh=float('inf')), 'distance_thresh'),
                          (dict(rounds=0), 'rounds'), (dict(rounds=9), 'rounds'), (dict(rounds=1.5), 'rounds'), (dict(iters=-1), 'iters'),
                          (dict(iters=65), 'iters'), (dict(iters=2.5), 'iters'), (dict(lambda0=0.0), 'lambda0'), (dict(lambda0=1e13), 'lambda0'),
                          (dict(lambda0=float('nan')), 'lambda0')):
            kw = dict(points=pts, cameras=cams, poses=poses, X=X)
            kw.update(bad)
            with pytest.raises(ValueError, match=word):
                fn(**kw)
    img = np.zeros((10, 12, 3), np.uint8)
    K = np.array([[500.0, 0.5, 320.0], [0.0, 510.0, 240.0], [0.0, 0.0, 1.0]])
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match='bundle_rounds'):
            reconstruct_tensors(np.zeros((5, 4)), img, img, K, K, bundle_rounds=bad)


def test_cpu_tensors_are_refused():
    pts, cams, poses = np.zeros((3, 20, 2)), np.tile([500.0, 500.0, 320.0, 240.0, 0.0], (3, 1)), np.tile(np.eye(3, 4).reshape(12), (3, 1))
    X = np.ones((20, 3))
    for kw in (dict(points=torch.from_numpy(pts)), dict(poses=torch.from_numpy(poses)), dict(X=torch.from_numpy(X)),
               dict(visible=torch.ones((3, 20), dtype=torch.uint8)), dict(found=torch.ones(8, dtype=torch.int32))):
        a = dict(points=pts, cameras=cams, poses=poses, X=X)
        a.update(kw)
        with pytest.raises(_lib.CotrHipError, match='MI355X only'):
            bundle_adjust_tensors(**a)
