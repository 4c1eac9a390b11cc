"""The relative-pose refit without a GPU: the numpy restatement (tests/pose_refit_oracle.py) against itself by a second route
and against the scenes, the properties the device tests' fixtures were chosen for, the order noise the device bounds are
derived from, and every argument error of the ABI and of the wrappers."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.build import declared_symbols
from tests import essential_oracle as eo
from tests import pose_refit_oracle as po

K = np.array([[800.0, 1.5, 320.0], [0.0, 780.0, 240.0], [0.0, 0.0, 1.0]])
ids = lambda s: f'n{s[0]}-seed{s[6]}'   # noqa: E731


def _proper(R):
    return np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scene', po.SIZES, ids=ids)
def test_analytic_jacobian_against_central_differences(scene):
    """The quotient rule against (r(+h) - r(-h)) / 2h along the five parameters, h = 1e-6, over every point of the scene
    (outliers included).  Central differences carry h^2 times a third derivative and eps / h of rounding, 1e-10 at O(1)
    residuals; measured over SIZES: at most 5.1e-10 of the largest entry.  Allowed: 1e-8."""
    s = po.start(scene)
    xn1, xn2 = eo.normalise(s['p1'], s['K1']), eo.normalise(s['p2'], s['K2'])
    R, t = s['R0'], po.unit(s['t0'])
    E, dE, _, _ = po.derive(R, t)
    r, J, skip = po.jacobian(E, dE, xn1, xn2)
    Jn = po.jacobian_numeric(R, t, xn1, xn2)
    worst = np.abs(J - Jn).max() / np.abs(J).max()
    print(f'n={scene[0]}: analytic against numeric {worst:.2e}')
    assert not skip.any() and worst <= 1e-8
    # r^2 is the Sampson error of essential_oracle
    assert np.allclose(r * r, eo.errors(E.reshape(1, 9), xn1, xn2)[0], rtol=1e-6, atol=0)


def exact_scene(n=40):
    """R = I, t = e_0, focal length 1: x2 = x1 + 1 / z, y2 = y1 with dyadic coordinates and depths 4 or 8, so every residual is
    exactly 0 in float64 and the points are float32 numbers"""
    rng = np.random.default_rng(0)
    x1 = rng.integers(-64, 65, (n, 2)) / 64.0
    z = rng.choice([4.0, 8.0], n)
    x2 = x1 + np.stack([1.0 / z, np.zeros(n)], axis=1)
    return x1, x2, np.eye(3), np.eye(3), np.array([1.0, 0.0, 0.0])


def test_true_pose_of_exact_points_is_a_fixed_point():
    x1, x2, K1, R, t = exact_scene()
    assert np.array_equal(eo.f32(x1), x1) and np.array_equal(eo.f32(x2), x2)
    q = po.refine(R, 3.0 * t, x1, x2, K1, None, None, 0.01, 50.0, 4, 10)
    assert list(q['info']) == [1, 40, 4, 0, 0, 0, 0, 0]
    assert np.array_equal(q['R'], R) and np.array_equal(q['t'], t) and q['mask'].all()
    assert all(r['kept'] == 0 and r['errs'] == [0.0] for r in q['rounds'])
    assert np.array_equal(q['E'], po.unit_signed(eo.essential_of(R, t)))


@pytest.mark.parametrize('scene', [eo.SCENES[2], eo.SCENES[3], (64, 0.0, 0.0, 1.0, 0, 0, 12)], ids=ids)
def test_returns_to_the_pose_of_a_noise_free_scene(scene):
    """From the scene's pose turned by 1 degree (its direction by 3) on the scene's own inliers.  The points are rounded to
    float32, 3e-5 px or 4e-8 of a focal length: the fit started at the scene's pose itself ends 7.6e-9, 3.1e-9 and 5.1e-8 away
    from it (an entry of R or t; n = 300, 1000, 64).  Measured from the turned pose: 3.8e-8, 1.1e-8, 5.2e-8.  Allowed: 2e-7."""
    n, outl, _, thr, _, _, seed = scene
    p1, p2, K1, K2, R, t, good = eo.two_view_scene(n, outl, seed, 0.0)
    R0, t0 = po.perturbed(R, t, 1.0, 3.0, 7)
    assert eo.rotation_error_deg(R0, R) > 0.99 and eo.direction_error_deg(t0, t) > 2.99
    q = po.refine(R0, t0, p1, p2, K1, K2, good, thr, 50.0, 1, 10)
    d = max(np.abs(q['R'] - R).max(), np.abs(q['t'] - t).max())
    print(f'n={n}: {q["info"][3]} steps kept, {d:.2e} from the scene')
    assert q['info'][3] >= 3 and d <= 2e-7
    assert _proper(q['R']) and abs(np.linalg.norm(q['t']) - 1) < 1e-15
    # more rounds re-count to the same inliers and stay there
    q4 = po.refine(R0, t0, p1, p2, K1, K2, good, thr, 50.0, 4, 10)
    assert np.array_equal(q4['mask'], good) and max(np.abs(q4['R'] - R).max(), np.abs(q4['t'] - t).max()) <= 2e-7


@pytest.mark.parametrize('scene', po.SIZES, ids=ids)
def test_fixture_properties_rotation_and_monotone_error(scene):
    """What tests/test_pose_refit_gpu.py relies on, for the restatement alone: every re-counted mask has a relative margin
    above 1e-6; the result is a rotation to 1e-12 with |t| = 1; the error on a round's fixed mask never rises; the info"""
    ref = po.reference(scene)
    s = po.start(scene)
    assert s['mask0'].sum() >= 5
    assert min(r['recount_margin'] for r in ref['rounds']) > 1e-6
    assert _proper(ref['R']) and abs(np.linalg.norm(ref['t']) - 1) < 1e-15
    assert abs(np.linalg.norm(ref['E']) - 1) < 1e-15 and ref['E'][np.argmax(np.abs(ref['E']))] > 0
    for r in ref['rounds']:
        assert len(r['errs']) == r['kept'] + 1 and all(b < a for a, b in zip(r['errs'], r['errs'][1:]))
    assert ref['info'][0] == 1 and ref['info'][1] == ref['mask'].sum() and ref['info'][2] == 8
    assert ref['info'][3] == sum(r['kept'] for r in ref['rounds']) and ref['info'][4] == ref['rounds'][-1]['kept']
    # no step and one round: the input, t normalised
    q = po.refine(s['R0'], 2.0 * s['t0'], s['p1'], s['p2'], s['K1'], s['K2'], s['mask0'], s['thr'], 50.0, 1, 0)
    assert np.array_equal(q['R'], s['R0']) and np.array_equal(q['t'], po.unit(2.0 * s['t0'])) and np.array_equal(q['mask'], s['mask0'])


def test_order_noise_is_what_the_device_bounds_are_derived_from():
    """The restatement with its sums forwards against backwards over SIZES.  Measured: the refit (8 rounds of 10) differs by up
    to 5.0e-9 in an entry of R or t, at n = 63, where a marginal step is kept one way and not the other; one accumulation
    differs by up to 2.5e-15 of the largest sum of its group.  The device is allowed 1000 times each."""
    refit = [po.order_noise(s) for s in po.SIZES]
    one = [po.sums_order_noise(s) for s in po.SIZES]
    print('refit: ' + ' '.join(f'{v:.1e}' for v in refit) + '\nsums:  ' + ' '.join(f'{v:.1e}' for v in one))
    assert max(refit) <= po.ORDER_NOISE and max(one) <= po.SUMS_ORDER_NOISE
    assert po.REFIT_BOUND == 1000 * po.ORDER_NOISE and po.SUMS_BOUND == 1000 * po.SUMS_ORDER_NOISE
    assert po.ORDER_NOISE <= 1e-8 and po.SUMS_ORDER_NOISE <= 1e-14


@pytest.mark.parametrize('scene', po.QUALITY, ids=lambda s: f'n{s[0]}-it{s[5]}')
def test_four_rounds_improve_the_ransac_pose_on_the_quality_scenes(scene):
    """For the restatement alone, from its own RANSAC pose and pose mask: after 4 rounds of 10 both pose errors are below the
    unrefined ones, and the re-counted masks keep their margin"""
    ref = eo.reference(scene)
    pose = ref['pose']
    assert scene[0] >= 1000 or scene[2] == 0.0
    q = po.refine(pose['R'], pose['t'], ref['p1'], ref['p2'], ref['K1'], ref['K2'], pose['mask'], scene[3], 50.0, 4, 10)
    before = eo.rotation_error_deg(pose['R'], ref['R']), eo.direction_error_deg(pose['t'], ref['t'])
    after = eo.rotation_error_deg(q['R'], ref['R']), eo.direction_error_deg(q['t'], ref['t'])
    print(f'n={scene[0]}: {before[0]:.3g} / {before[1]:.3g} -> {after[0]:.3g} / {after[1]:.3g} deg')
    assert after[0] < before[0] and after[1] < before[1]
    assert min(r['recount_margin'] for r in q['rounds']) > 1e-6


def test_tangent_basis_rule():
    for k in range(3):
        for sign in (1.0, -1.0):
            t = np.zeros(3)
            t[k] = sign
            b1, b2, kk = po.basis(t)
            assert kk == (1 if k == 0 else 0)                 # the first index whose entry is 0
            assert abs(b1 @ t) == 0 and abs(b2 @ t) == 0 and abs(b1 @ b2) == 0 and np.linalg.norm(b1) == 1 and np.linalg.norm(b2) == 1
            assert np.array_equal(np.cross(b1, b2), t)        # (b1, b2, t) is right-handed
    s = 1.0 / np.sqrt(3.0)
    for t, want in ((np.array([s, s, s]), 0), (np.array([s, -s, s]), 0), (po.unit([2.0, 1.0, 1.0]), 1), (po.unit([1.0, 2.0, 1.0]), 0),
                    (po.unit([2.0, 2.0, -1.0]), 2), (po.unit([0.3, -0.2, 0.9]), 1)):
        b1, b2, k = po.basis(t)
        assert k == want
        e = np.eye(3)[k]
        assert np.allclose(b1, np.cross(e, t) / np.linalg.norm(np.cross(e, t)), atol=1e-16) and np.allclose(b2, np.cross(t, b1), atol=1e-16)
        assert abs(b1 @ t) < 1e-16 and abs(b2 @ t) < 1e-16 and abs(np.linalg.norm(b2) - 1) < 1e-15
    # the five directions are the derivative of E along the step
    R, t = po.perturbed(np.eye(3), po.unit([0.3, -0.2, 0.9]), 20.0, 0.0, 1)
    E, dE, b1, b2 = po.derive(R, t)
    for k in range(5):
        d = np.zeros(5)
        d[k] = 1e-6
        Rp, tp = po.step(R, t, d, b1, b2)
        Rm, tm = po.step(R, t, -d, b1, b2)
        assert np.abs((po.cross_mat(tp, Rp) - po.cross_mat(tm, Rm)) / 2e-6 - dE[k]).max() < 1e-9


def test_degenerate_input_of_the_restatement():
    s = po.start(po.SIZES[3])
    a = (s['p1'], s['p2'], s['K1'], s['K2'], s['mask0'], s['thr'])
    for R0, t0, found in ((s['R0'], s['t0'], 0), (s['R0'] * np.nan, s['t0'], 1), (s['R0'], np.zeros(3), 1), (s['R0'], np.array([np.inf, 0, 0]), 1)):
        q = po.refine(R0, t0, *a, found=found)
        assert not q['R'].any() and not q['t'].any() and not q['E'].any() and not q['mask'].any() and not q['info'].any()
    few = np.zeros(s['p1'].shape[0], bool)
    few[np.flatnonzero(s['mask0'])[:4]] = True
    q = po.refine(s['R0'], s['t0'], s['p1'], s['p2'], s['K1'], s['K2'], few, s['thr'], 50.0, 1, 10)
    assert list(q['info'][:5]) == [1, 4, 1, 0, 0] and np.array_equal(q['R'], s['R0'])
    same1, same2 = np.repeat([[300.0, 200.0]], 64, 0), np.repeat([[310.0, 205.0]], 64, 0)
    q = po.refine(s['R0'], s['t0'], same1, same2, K, None, None, 1.0, 50.0, 2, 10)
    assert q['info'][3] == 0 and np.array_equal(q['R'], s['R0'])     # one point 64 times: a singular system, no step


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
NAMES = ('cotr_refine_pose', 'cotr_refine_pose_scratch_bytes')


def test_symbols_are_declared_and_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and name in declared_symbols()
        assert getattr(_lib.load_library(), name) is not None


def test_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    b = ctypes.c_size_t()
    P = ctypes.c_void_p(4096)           # never dereferenced: every call below fails its checks before any HIP call
    K9 = ctypes.c_double * 9
    good = K9(*K.reshape(9))
    for n in (4, (1 << 24) + 1):
        assert lib.cotr_refine_pose_scratch_bytes(n, ctypes.byref(b)) == -1 and b'[5, 2^24]' in lib.cotr_raster_last_error()
    assert lib.cotr_refine_pose_scratch_bytes(100, None) == -1 and b'NULL' in lib.cotr_raster_last_error()
    assert lib.cotr_refine_pose_scratch_bytes(5, ctypes.byref(b)) == 0 and b.value >= 5 * 32 + 22 * 8
    assert lib.cotr_refine_pose_scratch_bytes(1 << 24, ctypes.byref(b)) == 0 and b.value >= (1 << 24) * 32 + 8192 * 22 * 8
    assert lib.cotr_refine_pose_scratch_bytes(100, ctypes.byref(b)) == 0
    need = b.value

    def call(n=100, thr=1.0, dist=50.0, rounds=4, iters=10, R=P, t=P, pts=P, k1=good, k2=good, mask=None, found=None, out=P, t_out=P, E_out=P,
             mask_out=P, info=P, scratch=P, nbytes=need):
        return lib.cotr_refine_pose(R, t, pts, P, n, k1, k2, thr, dist, rounds, iters, mask, found, out, t_out, E_out, mask_out, info, scratch,
                                    nbytes, None)
    odd = ctypes.c_void_p(4100)
    for kw, word in ((dict(n=4), b'[5, 2^24]'), (dict(n=(1 << 24) + 1), b'[5, 2^24]'), (dict(thr=0.0), b'threshold'), (dict(thr=-1.0), b'threshold'),
                     (dict(thr=float('nan')), b'threshold'), (dict(thr=float('inf')), b'threshold'), (dict(dist=0.0), b'distance_thresh'),
                     (dict(dist=float('nan')), b'distance_thresh'), (dict(dist=float('inf')), b'distance_thresh'), (dict(rounds=0), b'rounds'),
                     (dict(rounds=9), b'rounds'), (dict(iters=-1), b'refine_iters'), (dict(iters=65), b'refine_iters'), (dict(R=None), b'NULL'),
                     (dict(t=None), b'NULL'), (dict(pts=None), b'NULL'), (dict(k1=None), b'NULL'), (dict(k2=None), b'NULL'), (dict(out=None), b'NULL'),
                     (dict(t_out=None), b'NULL'), (dict(E_out=None), b'NULL'), (dict(mask_out=None), b'NULL'), (dict(info=None), b'NULL'),
                     (dict(scratch=None), b'NULL'),
                     (dict(k2=K9(*np.diag([0.0, 780.0, 1.0]).reshape(9))), b'focal'), (dict(k1=K9(*np.diag([800.0, np.nan, 1.0]).reshape(9))), b'focal'),
                     (dict(k1=K9(*np.array([[800.0, np.inf, 0], [0, 780.0, 0], [0, 0, 1]]).reshape(9))), b'finite'),
                     (dict(k1=K9(*np.diag([-800.0, -780.0, 1.0]).reshape(9)), k2=K9(*np.diag([800.0, 780.0, 1.0]).reshape(9))), b'mean focal'),
                     (dict(R=odd), b'aligned'), (dict(t=odd), b'aligned'), (dict(E_out=odd), b'aligned'), (dict(found=ctypes.c_void_p(4098)), b'aligned'),
                     (dict(info=ctypes.c_void_p(4098)), b'aligned'), (dict(scratch=ctypes.c_void_p(4104)), b'aligned'), (dict(nbytes=need - 1), b'smaller')):
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
def test_wrapper_argument_errors_without_a_gpu():
    from cotr_amd.inference import refine_pose_tensors, refine_relative_pose, relative_pose
    from cotr_amd.inference.essential import relative_pose_tensors
    z, R, t = np.zeros((20, 2)), np.eye(3), np.array([1.0, 0.0, 0.0])
    for fn in (refine_pose_tensors, refine_relative_pose):
        with pytest.raises(ValueError, match='at least 5'):
            fn(R, t, np.zeros((4, 2)), np.zeros((4, 2)), K)
        with pytest.raises(ValueError, match='same length'):
            fn(R, t, z, np.zeros((21, 2)), K)
        with pytest.raises(ValueError, match=r'\[N, 2\]'):
            fn(R, t, np.zeros((20, 3)), np.zeros((20, 3)), K)
        with pytest.raises(ValueError, match=r'\[3, 3\]'):
            fn(R, t, z, z, np.eye(4))
        with pytest.raises(ValueError, match='focal'):
            fn(R, t, z, z, K, np.diag([500.0, np.nan, 1.0]))
        with pytest.raises(ValueError, match='threshold'):
            fn(R, t, z, z, K, threshold=0.0)
        with pytest.raises(ValueError, match='threshold'):
            fn(R, t, z, z, K, threshold=float('inf'))
        with pytest.raises(ValueError, match='mean focal'):
            fn(R, t, z, z, np.diag([-500.0, -500.0, 1.0]), np.diag([500.0, 500.0, 1.0]))
        with pytest.raises(ValueError, match='distance_thresh'):
            fn(R, t, z, z, K, distance_thresh=0.0)
        for rounds in (0, 9):
            with pytest.raises(ValueError, match='rounds'):
                fn(R, t, z, z, K, rounds=rounds)
        for iters in (-1, 65):
            with pytest.raises(ValueError, match='refine_iters'):
                fn(R, t, z, z, K, refine_iters=iters)
        with pytest.raises(ValueError, match=r'R must be \[3, 3\]'):
            fn(np.eye(4), t, z, z, K)
        with pytest.raises(ValueError, match='t must have 3'):
            fn(R, np.zeros(4), z, z, K)
        with pytest.raises(ValueError, match='one entry per correspondence'):
            fn(R, t, z, z, K, mask=np.ones(19))
        with pytest.raises(TypeError, match='unexpected keyword'):
            fn(R, t, z, z, K, round=1)
    for fn in (relative_pose, relative_pose_tensors):
        for rounds in (-1, 9):
            with pytest.raises(ValueError, match='refine_rounds'):
                fn(z, z, K, refine_rounds=rounds)
        for iters in (-1, 65):
            with pytest.raises(ValueError, match='refine_iters'):
                fn(z, z, K, refine_rounds=2, refine_iters=iters)


def test_cpu_tensors_are_refused():
    from cotr_amd.inference import refine_pose_tensors, refine_relative_pose
    z, R, t = np.zeros((20, 2)), np.eye(3), np.array([1.0, 0.0, 0.0])
    for fn in (refine_pose_tensors, refine_relative_pose):
        with pytest.raises(_lib.CotrHipError, match='MI355X only'):
            fn(torch.eye(3, dtype=torch.float64), t, z, z, K)
        with pytest.raises(_lib.CotrHipError, match='MI355X only'):
            fn(R, t, torch.zeros((20, 2), dtype=torch.float64), z, K)
        with pytest.raises(_lib.CotrHipError, match='MI355X only'):
            fn(R, t, z, z, K, mask=torch.ones(20))


def test_zoom_engine_passes_the_refit_arguments_through(monkeypatch):
    from cotr_amd.inference import ZoomEngine, essential
    want = np.random.default_rng(0).uniform(0, 100, (12, 4))
    calls = []

    def relative_pose_tensors(p1, p2, K1, K2=None, **kw):
        calls.append(kw)
        raise StopIteration
    monkeypatch.setattr(essential, 'relative_pose_tensors', relative_pose_tensors)

    class Spy(ZoomEngine):
        def __init__(self):
            pass

        def cotr_corr_multiscale(self, *a, **kw):
            return want
    with pytest.raises(StopIteration):
        Spy().relative_pose('a', 'b', K, K, refine_rounds=4, refine_iters=7, seed=3)
    assert calls == [dict(refine_rounds=4, refine_iters=7, seed=3)]
