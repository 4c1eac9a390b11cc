"""The essential-matrix estimator and recover_pose without a GPU: the numpy restatement (tests/essential_oracle.py) against
the equations a candidate has to satisfy, against ground truth, literal loops and LAPACK, the scenes the GPU tests use
against the properties they were chosen for, and the argument checks of the C ABI (they run before any HIP call) and of the
Python wrappers."""
import ctypes

import numpy as np
import pytest

from cotr_amd import _lib
from cotr_amd.build import declared_symbols
from tests import essential_oracle as eo

K = np.array([[800.0, 1.5, 320.0], [0.0, 780.0, 240.0], [0.0, 0.0, 1.0]])


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_sampler_is_the_f_paths_draws_with_model_size_5():
    from tests import guided_oracle as go
    s5, s7 = eo.samples(40, 300, 3), go.samples(40, 300, 3)
    assert np.array_equal(s5, s7[:, :5])
    assert (s5 >= 0).all() and all(len(set(r)) == 5 for r in s5)
    assert all(sorted(r) == [0, 1, 2, 3, 4] for r in eo.samples(5, 50, 1))


def test_normalisation_inverts_the_camera_matrix():
    rng = np.random.default_rng(0)
    p = eo.f32(rng.uniform(0, 640, (50, 2)))
    x = eo.normalise(p, K)
    back = np.c_[x, np.ones(50)] @ K.T
    assert np.abs(back[:, :2] - p).max() < 1e-10
    K2 = K * [[0.5, 1, 1], [1, 0.7, 1], [1, 1, 1]]
    assert eo.scaled_threshold(2.0, K, K2) == 2.0 / ((K[0, 0] + K[1, 1] + K2[0, 0] + K2[1, 1]) / 4.0) and K2[0, 0] == 400.0


@pytest.mark.parametrize('seed', range(6))
def test_every_candidate_satisfies_its_equations(seed):
    # At unit norm, whatever the conditioning of the sample: the five epipolar equations to 1e-12 and the trace constraint
    # to 1e-10 (a polished root of the ten cubics makes both vanish to rounding: coordinates and entries are O(1)).
    p1, p2, K1, K2, _, _, _ = eo.two_view_scene(300, 0.4 if seed % 2 else 0.0, seed, 1.0 if seed < 4 else 0.0)
    x1, x2 = eo.normalise(p1, K1), eo.normalise(p2, K2)
    total = 0
    for s in eo.samples(300, 60, seed):
        for var in ('x', 'z'):
            cands = eo.five_point(x1[s], x2[s], var)
            assert len(cands) <= 10
            for E in cands:
                epi, trace = eo.residuals(E, x1[s], x2[s])
                assert abs(np.linalg.norm(E) - 1) < 1e-14 and E[np.argmax(np.abs(E))] > 0
                assert epi <= 1e-12 and trace <= 1e-10, (epi, trace)
                total += 1
    assert total >= 120      # about 4.4 real candidates per sample


@pytest.mark.parametrize('seed', range(6))
def test_ground_truth_is_among_the_candidates_of_exact_points(seed):
    # five exact pairs (float64, no pixel rounding): a candidate equals [t]x R at unit norm up to sign.  A root of a
    # polynomial system moves by its condition number times the rounding of the coefficients (1.1e-16); 1e-8 allows a
    # condition number of 1e8.
    rng = np.random.default_rng(seed)
    _, _, _, _, R, t, _ = eo.two_view_scene(10, 0.0, seed, 0.0)
    Et = eo.unit_signed(eo.essential_of(R, t).reshape(9))
    for _ in range(10):
        X = np.concatenate([rng.uniform(-2, 2, (5, 2)), rng.uniform(4, 8, (5, 1))], axis=1)
        Y = X @ R.T + t
        cands = eo.five_point(X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:])
        assert cands and min(np.abs(E - Et).max() for E in cands) < 1e-8


def test_degenerate_samples_have_no_model():
    p = np.repeat([[0.1, 0.2]], 5, 0)
    assert eo.five_point(p, p + 0.05) == []
    r = eo.ransac(np.repeat([[300.0, 200.0]], 40, 0), np.repeat([[310.0, 205.0]], 40, 0), K, None, 1.0, 0.999, 30, 0)
    assert list(r['info']) == [0, 0, 30, -1, 0, 0, 0, 0] and (r['hyp_count'] == -1).all() and not r['mask'].any() and (r['E'] == 0).all()


@pytest.mark.parametrize('seed', range(30))
def test_vectorised_selection_equals_the_sequential_loop(seed):
    rng = np.random.default_rng(seed)
    iters, n = int(rng.integers(1, 200)), int(rng.integers(5, 300))
    conf = [0.5, 0.999, 0.999999][seed % 3]
    cnt = rng.integers(0, n + 1, 10 * iters)
    cnt[rng.random(10 * iters) < 0.6] = -1
    cnt[rng.random(10 * iters) < 0.3] = 5
    if seed % 4 == 0:
        cnt = np.minimum(cnt, rng.integers(5, 10))
    if seed % 5 == 0:
        cnt[(10 * iters) // 3] = n - 1
    assert eo.select(cnt, iters, n, conf) == eo.select_sequential(cnt, iters, n, conf)


def test_selection_details():
    cnt = np.full(50, 4)
    assert eo.select(cnt, 5, 100, 0.999) == (0, 0, 5, -1)        # nothing beats 4
    cnt[14] = cnt[23] = 5                                        # an equal count later: the first one is kept
    assert eo.select(cnt, 5, 100, 0.999) == (1, 5, 5, 14)
    cnt[31] = 100                                                # every point: stop after this iteration, whose rest is still looked at
    cnt[37] = 100
    assert eo.select(cnt, 5, 100, 0.999) == eo.select_sequential(cnt, 5, 100, 0.999) == (1, 100, 4, 31)


@pytest.mark.parametrize('seed', range(8))
def test_decomposition_against_svd_and_the_four_candidates(seed):
    _, _, _, _, R, t, _ = eo.two_view_scene(10, 0.0, seed, 0.0)
    E = eo.unit_signed(eo.essential_of(R, t).reshape(9)) * [1.0, -1.0][seed % 2]
    U, V, R1, R2, tt = eo.decompose(E)
    sv = np.linalg.svd(E.reshape(3, 3), compute_uv=False)
    assert abs(sv[0] - sv[1]) < 1e-12 and sv[2] < 1e-12
    # orthonormal, det +1, and U diag(s, s, 0) V^T is E again: float64 on O(1) entries, a few hundred operations
    for M in (U, V, R1, R2):
        assert np.abs(M.T @ M - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(M) - 1) < 1e-12
    assert np.abs(U @ np.diag([sv[0], sv[1], 0.0]) @ V.T - E.reshape(3, 3)).max() < 1e-12
    # against LAPACK's decomposition: the same two rotations and the same t up to sign
    Ul, _, Vtl = np.linalg.svd(E.reshape(3, 3))
    Ul, Vtl = Ul * np.sign(np.linalg.det(Ul)), Vtl * np.sign(np.linalg.det(Vtl))
    W = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]])
    lap = [Ul @ W @ Vtl, Ul @ W.T @ Vtl]
    assert min(np.abs(R1 - lap[0]).max() + np.abs(R2 - lap[1]).max(), np.abs(R1 - lap[1]).max() + np.abs(R2 - lap[0]).max()) < 1e-10
    assert min(np.abs(tt - Ul[:, 2]).max(), np.abs(tt + Ul[:, 2]).max()) < 1e-10
    # the true pose is one of the four
    cands = eo.pose_candidates(E)
    assert [np.array_equal(c[0], r) for c, r in zip(cands, (R1, R2, R1, R2))] == [True] * 4
    assert np.array_equal(cands[2][1], -cands[0][1]) and np.array_equal(cands[1][1], cands[0][1])
    assert min(np.abs(Rc - R).max() + np.abs(tc - t).max() for Rc, tc in cands) < 1e-10
    assert eo.decompose(np.full(9, np.nan)) is None and eo.decompose(np.zeros(9)) is None


@pytest.mark.parametrize('seed', range(6))
def test_exactly_one_candidate_puts_a_noise_free_scene_in_front(seed):
    p1, p2, K1, K2, R, t, _ = eo.two_view_scene(200, 0.0, seed, 0.0)
    r = eo.recover_pose(eo.essential_of(R, t).reshape(9), p1, p2, K1, K2)
    cnt = list(r['info'][2:6])
    assert sorted(cnt) == [0, 0, 0, 200] and r['info'][0] == 200 and r['info'][1] == cnt.index(200) and r['mask'].all()
    assert eo.rotation_error_deg(r['R'], R) < 1e-5 and eo.direction_error_deg(r['t'], t) < 1e-5
    half = np.arange(200) % 2 == 0
    r = eo.recover_pose(eo.essential_of(R, t).reshape(9), p1, p2, K1, K2, mask=half)
    assert r['info'][0] == 100 and np.array_equal(r['mask'], half)
    r = eo.recover_pose(eo.essential_of(R, t).reshape(9), p1, p2, K1, K2, dist=4.0)       # every depth is above 4
    assert list(r['info'][:6]) == [0, 0, 0, 0, 0, 0] and not r['mask'].any()


def test_closed_form_depths_against_lstsq():
    p1, p2, K1, K2, R, t, _ = eo.two_view_scene(60, 0.0, 3, 1.0)
    x1, x2 = eo.normalise(p1, K1), eo.normalise(p2, K2)
    for Rc, tc in eo.pose_candidates(eo.essential_of(R, t).reshape(9)):
        z1, z2, det = eo.depths(Rc, tc, x1, x2)
        for i in range(60):
            a, b = Rc @ np.r_[x1[i], 1.0], np.r_[x2[i], 1.0]
            z = np.linalg.lstsq(np.stack([a, -b], axis=1), -tc, rcond=None)[0]
            # a 2 x 2 normal system: relative 1e-9 allows a condition number of 1e7 (rays within 0.02 deg of parallel)
            assert abs(z[0] - z1[i]) <= 1e-9 * max(1.0, abs(z[0])) and abs(z[1] - z2[i]) <= 1e-9 * max(1.0, abs(z[1]))
    # a point on the baseline's direction: the rays are parallel, the determinant is 0, in front of nothing
    x = np.array([[0.0, 0.0]])
    assert eo.depths(np.eye(3), np.array([0.0, 0.0, 1.0]), x, x)[2][0] == 0.0
    assert not eo.in_front(np.eye(3), np.array([0.0, 0.0, 1.0]), x, x)[0]


@pytest.mark.parametrize('scene', eo.SCENES + eo.EDGES, ids=lambda s: f'n{s[0]}-it{s[5]}')
def test_scenes_have_the_properties_they_were_chosen_for(scene):
    n, outl, noise, thr, conf, iters, seed = scene
    ref = eo.reference(scene)
    r, pose = ref['ransac'], ref['pose']
    assert r['info'][0] and pose is not None
    # the x-route and the z-route of the action matrix: the same candidates on every iteration
    xn1, xn2 = eo.normalise(ref['p1'], ref['K1']), eo.normalise(ref['p2'], ref['K2'])
    Ez, ncz = eo.candidates(xn1, xn2, r['samples'], 'z')
    for it in range(iters):
        a = [r['hyp_E'][10 * it + k] for k in range(r['ncand'][it])]
        b = [Ez[10 * it + k] for k in range(ncz[it])]
        assert eo.set_distance(a, b) <= 1e-7, it
    assert np.array_equal(eo.counts(r['hyp_E'], eo.slots_used(r['ncand']), xn1, xn2, eo.scaled_threshold(thr, ref['K1'], ref['K2'])),
                          r['hyp_count'])
    assert tuple(r['info'][:4]) == eo.select_sequential(r['hyp_count'], iters, n, conf)
    # no depth of a masked point within 1e-9 relative of 0 or of the distance threshold: none has to be excluded
    assert pose['margin'] > 1e-9
    assert pose['info'][0] == max(pose['info'][2:6]) and abs(np.linalg.det(pose['R']) - 1) < 1e-12


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
NAMES = ('cotr_ransac_essential', 'cotr_ransac_essential_scratch_bytes', 'cotr_recover_pose', 'cotr_recover_pose_scratch_bytes')


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

    def cam(**kw):
        k = K.copy()
        for (i, j), v in kw.get('set', {}).items():
            k[i, j] = v
        return K9(*k.reshape(9))
    for n in (4, (1 << 24) + 1):
        assert lib.cotr_ransac_essential_scratch_bytes(n, 100, ctypes.byref(b)) == -1
        assert b'[5, 2^24]' in lib.cotr_raster_last_error()
        assert lib.cotr_recover_pose_scratch_bytes(n, ctypes.byref(b)) == -1
        assert b'[5, 2^24]' in lib.cotr_raster_last_error()
    for iters in (0, 6554):
        assert lib.cotr_ransac_essential_scratch_bytes(100, iters, ctypes.byref(b)) == -1
        assert b'max_iters' in lib.cotr_raster_last_error()
    assert lib.cotr_ransac_essential_scratch_bytes(100, 100, None) == -1 and b'NULL' in lib.cotr_raster_last_error()
    assert lib.cotr_recover_pose_scratch_bytes(100, None) == -1 and b'NULL' in lib.cotr_raster_last_error()
    assert lib.cotr_ransac_essential_scratch_bytes(5, 1, ctypes.byref(b)) == 0 and b.value >= 10 * 76 + 5 * 32
    assert lib.cotr_ransac_essential_scratch_bytes(1 << 24, 6553, ctypes.byref(b)) == 0 and b.value >= 65530 * 76 + (1 << 24) * 32
    assert lib.cotr_ransac_essential_scratch_bytes(100, 1000, ctypes.byref(b)) == 0
    need = b.value
    assert lib.cotr_recover_pose_scratch_bytes(100, ctypes.byref(b)) == 0 and b.value > 0
    need_pose = b.value

    def call(n=100, thr=1.0, conf=0.999, iters=1000, pts=P, k1=good, k2=good, out=P, scratch=P, nbytes=need, hyp=None):
        return lib.cotr_ransac_essential(pts, P, n, k1, k2, thr, conf, iters, 0, out, P, P, hyp, None, None, scratch, nbytes, None)
    for kw, word in ((dict(n=4), b'[5, 2^24]'), (dict(n=(1 << 24) + 1), b'[5, 2^24]'), (dict(iters=0), b'max_iters'),
                     (dict(iters=6554), b'max_iters'), (dict(thr=0.0), b'threshold'), (dict(thr=-1.0), b'threshold'),
                     (dict(thr=float('nan')), b'threshold'), (dict(thr=float('inf')), b'threshold'), (dict(conf=0.0), b'confidence'),
                     (dict(conf=1.0), b'confidence'), (dict(conf=float('nan')), b'confidence'), (dict(pts=None), b'NULL'),
                     (dict(k1=None), b'NULL'), (dict(k2=None), b'NULL'), (dict(out=None), b'NULL'), (dict(scratch=None), b'NULL'),
                     (dict(k1=cam(set={(0, 0): 0.0})), b'focal'), (dict(k2=cam(set={(1, 1): 0.0})), b'focal'),
                     (dict(k1=cam(set={(0, 0): float('nan')})), b'focal'), (dict(k2=cam(set={(1, 1): float('inf')})), b'focal'),
                     (dict(k1=cam(set={(0, 2): float('nan')})), b'finite'), (dict(k1=cam(set={(0, 1): float('inf')})), b'finite'),
                     (dict(k1=cam(set={(0, 0): -800.0, (1, 1): -780.0}), k2=cam(set={(0, 0): 800.0, (1, 1): 780.0})), b'mean focal'),
                     (dict(scratch=ctypes.c_void_p(4104)), b'aligned'), (dict(hyp=ctypes.c_void_p(4100)), b'aligned'),
                     (dict(nbytes=need - 1), b'smaller')):
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())

    def pose(n=100, dist=50.0, E=P, k1=good, k2=good, out=P, scratch=P, nbytes=need_pose, mask=None, found=None):
        return lib.cotr_recover_pose(E, P, P, n, k1, k2, dist, mask, found, out, P, P, P, scratch, nbytes, None)
    for kw, word in ((dict(n=4), b'[5, 2^24]'), (dict(n=(1 << 24) + 1), b'[5, 2^24]'), (dict(dist=0.0), b'distance_thresh'),
                     (dict(dist=float('nan')), b'distance_thresh'), (dict(dist=float('inf')), b'distance_thresh'), (dict(E=None), b'NULL'),
                     (dict(k1=None), b'NULL'), (dict(out=None), b'NULL'), (dict(scratch=None), b'NULL'),
                     (dict(k2=cam(set={(0, 0): 0.0})), b'focal'), (dict(k1=cam(set={(1, 2): float('nan')})), b'finite'),
                     (dict(E=ctypes.c_void_p(4100)), b'aligned'), (dict(found=ctypes.c_void_p(4098)), b'aligned'),
                     (dict(scratch=ctypes.c_void_p(4104)), b'aligned'), (dict(nbytes=need_pose - 1), b'smaller')):
        assert pose(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
def test_wrapper_argument_errors_without_a_gpu():
    from cotr_amd.inference import find_essential_mat, ransac_essential, recover_pose, relative_pose
    z = np.zeros((20, 2))
    for fn in (lambda *a, **k: find_essential_mat(*a, **k), lambda *a, **k: ransac_essential(*a, **k), lambda *a, **k: relative_pose(*a, **k),
               lambda a, b, *c, **k: recover_pose(np.eye(3), a, b, *c, **k)):
        with pytest.raises(ValueError, match='at least 5'):
            fn(np.zeros((4, 2)), np.zeros((4, 2)), K)
        with pytest.raises(ValueError, match='same length'):
            fn(z, np.zeros((21, 2)), K)
        with pytest.raises(ValueError, match=r'\[N, 2\]'):
            fn(np.zeros((20, 3)), np.zeros((20, 3)), K)
        with pytest.raises(ValueError, match=r'\[3, 3\]'):
            fn(z, z, np.eye(4))
        with pytest.raises(ValueError, match='focal'):
            fn(z, z, np.diag([0.0, 500.0, 1.0]))
        with pytest.raises(ValueError, match='focal'):
            fn(z, z, K, np.diag([500.0, np.nan, 1.0]))
    for fn in (find_essential_mat, ransac_essential, relative_pose):
        with pytest.raises(ValueError, match='max_iters'):
            fn(z, z, K, max_iters=0)
        with pytest.raises(ValueError, match='max_iters'):
            fn(z, z, K, max_iters=6554)
        with pytest.raises(ValueError, match='threshold'):
            fn(z, z, K, threshold=0.0)
        with pytest.raises(ValueError, match='threshold'):
            fn(z, z, K, threshold=float('inf'))
        with pytest.raises(ValueError, match='mean focal'):
            fn(z, z, np.diag([-500.0, -500.0, 1.0]), np.diag([500.0, 500.0, 1.0]))
    with pytest.raises(ValueError, match='confidence'):
        find_essential_mat(z, z, K, prob=1.0)
    with pytest.raises(ValueError, match='confidence'):
        relative_pose(z, z, K, confidence=0.0)
    with pytest.raises(ValueError, match='distance_thresh'):
        recover_pose(np.eye(3), z, z, K, distance_thresh=0.0)
    with pytest.raises(ValueError, match='distance_thresh'):
        relative_pose(z, z, K, distance_thresh=float('nan'))
    with pytest.raises(ValueError, match=r'E must be \[3, 3\]'):
        recover_pose(np.eye(4), z, z, K)
    with pytest.raises(ValueError, match='one entry per correspondence'):
        recover_pose(np.eye(3), z, z, K, mask=np.ones(19))
    with pytest.raises(TypeError, match='unexpected keyword'):
        relative_pose(z, z, K, treshold=1.0)


def test_zoom_engine_relative_pose_host_logic(monkeypatch):
    from cotr_amd.inference import FasterSparseEngine, SparseEngine, ZoomEngine, essential
    assert SparseEngine.relative_pose is ZoomEngine.relative_pose and FasterSparseEngine.relative_pose is ZoomEngine.relative_pose
    rng = np.random.default_rng(0)
    want = rng.uniform(0, 100, (12, 4))
    calls = []

    def relative_pose(p1, p2, K1, K2=None, **kw):
        calls.append((p1.copy(), p2.copy(), K1, K2, kw))
        return 'R', 't', 'mask'
    monkeypatch.setattr(essential, 'relative_pose', relative_pose)

    class Spy(ZoomEngine):
        def __init__(self):
            self.calls = []

        def cotr_corr_multiscale(self, img_a, img_b, zoom_ins=(1.0,), converge_iters=1, max_corrs=1000, queries_a=None, **kw):
            self.calls.append((img_a, img_b, tuple(zoom_ins), converge_iters, max_corrs, None if queries_a is None else queries_a.shape, kw))
            return want
    spy, zooms = Spy(), np.linspace(0.5, 0.0625, 4)
    R, t, corrs, mask = spy.relative_pose('a', 'b', 'Ka', 'Kb', max_corrs=77, seed=3)
    assert (R, t, mask) == ('R', 't', 'mask') and np.array_equal(corrs, want)
    R, t, corrs, mask = spy.relative_pose('a', 'b', 'Ka', 'Kb', queries_a=np.zeros((12, 2)), converge_iters=2, threshold=2.0)
    assert (R, t, mask) == ('R', 't', 'mask') and np.array_equal(corrs, want)
    assert spy.calls == [('a', 'b', tuple(zooms), 1, 77, None, {}), ('a', 'b', tuple(zooms), 2, 1000, (12, 2), {'force': True})]
    assert [c[2:] for c in calls] == [('Ka', 'Kb', {'seed': 3}), ('Ka', 'Kb', {'threshold': 2.0})]
    assert all(np.array_equal(c[0], want[:, :2]) and np.array_equal(c[1], want[:, 2:]) for c in calls)
