"""The absolute-pose estimator without a GPU: the numpy restatement (tests/pnp_oracle.py) against ground truth, against a
second route through itself and against literal loops, the scenes the GPU tests use against the properties they were chosen
for, ``rodrigues``, and the argument checks of the C ABI (they run before any HIP call) and of the Python wrappers."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.build import declared_symbols
from cotr_amd.inference import lift_pixels, localize, ransac_pnp, rodrigues, solve_pnp_ransac
from tests import pnp_oracle as po

K = np.array([[800.0, 1.5, 320.0], [0.0, 780.0, 240.0], [0.0, 0.0, 1.0]])
ALL = po.SCENES + po.EDGES
IDS = lambda s: f'n{s[0]}-it{s[5]}'   # noqa: E731


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_sampler_is_the_f_paths_draws_with_model_size_4():
    from tests import guided_oracle as go
    s4, s7 = po.samples(40, 300, 3), go.samples(40, 300, 3)
    assert np.array_equal(s4, s7[:, :4])
    assert all(sorted(r) == [0, 1, 2, 3] for r in po.samples(4, 50, 1))
    assert (po.samples(3, 10, 0)[:, 3] == -1).all()


@pytest.mark.parametrize('seed', range(6))
def test_p3p_has_the_true_pose_among_its_solutions(seed):
    # exact pixels (float64, no rounding): a solution equals the scene's pose.  A root of the quartic moves by its condition
    # number times the rounding of the coefficients; 1e-8 allows a condition number of 1e8.
    rng = np.random.default_rng(seed)
    X, _, Ks, R, t, _ = po.pnp_scene(90, 0.0, seed, 0.0)
    Y = X @ R.T + t
    p = Y @ Ks.T
    p = p[:, :2] / p[:, 2:]
    idx = rng.permutation(90).reshape(30, 3)
    sols, ok = po.p3p(X[idx], p[idx][:, :, 0], p[idx][:, :, 1], Ks)
    assert ok.all()
    truth = po.pack(R, t)
    for i in range(30):
        d = [po.pose_distance(s, truth) for s in sols[i] if np.isfinite(s).all()]
        assert d and min(d) < 1e-8, (i, d)
        Rs, _ = po.expand(sols[i][np.isfinite(sols[i]).all(axis=1)])
        assert np.abs(Rs @ np.swapaxes(Rs, -1, -2) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(Rs) - 1).max() < 1e-12


def test_samples_without_a_candidate():
    X, p, Ks, _, _, _ = po.pnp_scene(20, 0.0, 0, 0.0)
    line = X[0] + np.arange(20)[:, None] * (X[1] - X[0])                         # every object point on one line
    tab, has = po.candidates(line, p, Ks, po.samples(20, 30, 0))
    assert not has.any() and np.isnan(tab).all()
    r = po.ransac(line, p, Ks, max_iters=30)
    assert list(r['info']) == [0, 0, 30, -1, 0, 0, 0, 0] and (r['hyp_count'] == -1).all() and not r['mask'].any() and (r['R'] == 0).all()
    Xn = X.copy()
    Xn[::3] = np.nan                                                             # a NaN among the four points: no candidate
    smp = po.samples(20, 60, 1)
    tab, has = po.candidates(Xn, p, Ks, smp)
    assert np.array_equal(has, ~np.isin(smp, np.arange(0, 20, 3)).any(axis=1)) and has.any() and not has.all()
    assert not po.inliers(tab[has][0], Xn, p, Ks, 8.0)[0, ::3].any()             # and a NaN point is never an inlier


@pytest.mark.parametrize('scene', [s for s in ALL if s[2] == 0.0], ids=IDS)
def test_noise_free_scenes_give_the_scenes_pose(scene):
    # the pixels are rounded to float32 (half an ulp of 640 px: 3e-5 px, 6e-8 rad at a focal length of 500 px; depths of
    # 4-8 turn that into 5e-7 of translation): 1e-6 for the rotation entries and for t relative to its norm
    ref = po.reference(scene)
    r = ref['ransac']
    assert r['info'][0] and r['mask'].sum() == r['info'][1] >= ref['good'].sum() and r['mask'][ref['good']].all()
    assert po.rotation_error(r['R'], ref['R']) < 1e-6 and po.translation_error(r['t'], ref['t']) < 1e-6


@pytest.mark.parametrize('scene', ALL, ids=IDS)
def test_scenes_have_the_properties_they_were_chosen_for(scene):
    n, outl, noise, thr, conf, iters, seed = scene
    ref = po.reference(scene)
    r = ref['ransac']
    assert r['info'][0]
    # the sample order and a permuted one (the quartic in another depth ratio): the same chosen candidate on at least 99 %
    # of the iterations, which is what makes the GPU test's cap on excluded iterations fair
    tab2, has2 = po.candidates(ref['obj'], ref['img'], ref['K'], r['samples'], (2, 0, 1))
    bad = sum(1 for i in range(iters) if has2[i] != r['has'][i] or (has2[i] and po.pose_distance(tab2[i], r['hyp_pose'][i]) > 1e-7))
    assert bad <= iters // 100, f'{bad} of {iters} iterations differ between the two routes'
    # every candidate: a rotation, and its three sample points back within 1e-9 px
    Rs, _ = po.expand(r['hyp_pose'][r['has']])
    assert np.abs(Rs @ np.swapaxes(Rs, -1, -2) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(Rs) - 1).max() < 1e-12
    assert max(po.sample_residual_px(r['hyp_pose'][i], ref['obj'], ref['img'], ref['K'], r['samples'][i]) for i in np.flatnonzero(r['has'])) <= 1e-9
    assert tuple(r['info'][:4]) == po.select_sequential(r['hyp_count'], iters, n, conf)
    assert r['mask'].sum() == r['info'][1] >= 4
    # the refit: its dependence on the order of the sums stays below the figure the GPU test's bound is built on
    noise_rt = po.order_noise(scene)
    assert noise_rt <= po.ORDER_NOISE < 1e-9
    # refining does not raise the squared error on the inliers
    R0, t0 = po.expand(r['hyp_pose'][r['info'][3]])
    img = po.f32(ref['img'])[r['mask']]
    assert po.refit_sums(r['R'], r['t'], ref['obj'][r['mask']], img, ref['K'])[27] <= po.refit_sums(R0, t0, ref['obj'][r['mask']], img, ref['K'])[27]


@pytest.mark.parametrize('seed', range(30))
def test_vectorised_selection_equals_the_sequential_loop(seed):
    rng = np.random.default_rng(seed)
    iters, n = int(rng.integers(1, 1200)), int(rng.integers(4, 300))
    conf = [0.5, 0.99, 0.999999][seed % 3]
    cnt = rng.integers(0, n + 1, iters)
    cnt[rng.random(iters) < 0.3] = -1
    cnt[rng.random(iters) < 0.3] = 4
    if seed % 4 == 0:
        cnt = np.minimum(cnt, rng.integers(4, 9))
    if seed % 5 == 0:
        cnt[iters // 3] = n - 1
    assert po.select(cnt, iters, n, conf) == po.select_sequential(cnt, iters, n, conf)
    assert po.select(np.full(20, 3), 20, 50, 0.99) == (0, 0, 20, -1)             # nothing beats 3


def test_lift_rule():
    depth = np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    depth[1, 2], depth[2, 0], depth[0, 3], depth[2, 3] = 0.0, -1.0, np.nan, np.inf
    pts = np.array([[0.5, 0.0], [1.5, 0.0], [2.5, 1.5], [-0.5, 0.0], [-0.51, 0.0], [3.49, 1.0], [3.5, 1.0], [0.0, 2.5], [2.0, 1.0], [0.0, 2.0],
                    [3.0, 0.0], [3.0, 2.0], [1.0, 1.0]])
    X = po.lift(pts, depth, K)
    z = [1, 3, 12 - 1, 1, np.nan, 8, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, 6]   # ties to even; (2.5, 1.5) -> (2, 2)
    assert np.array_equal(X[:, 2], np.array(z, np.float64), equal_nan=True)
    assert np.array_equal(np.isnan(X).any(axis=1), np.isnan(X).all(axis=1))
    back = X[12] @ K.T
    assert np.abs(back[:2] / back[2] - pts[12]).max() < 1e-12
    c2w = po.pose_matrix((10, 20, 30), (1, 2, 3))
    assert np.abs(po.lift(pts, depth, K, c2w)[12] - (c2w[:3, :3] @ X[12] + c2w[:3, 3])).max() < 1e-12


def test_rodrigues_round_trips():
    rng = np.random.default_rng(0)
    assert np.array_equal(rodrigues(np.zeros(3)), np.eye(3)) and np.array_equal(rodrigues(np.eye(3)), np.zeros((3, 1)))
    for theta in (1e-12, 1e-7, 0.3, 1.0, 3.0, np.pi - 1e-4, np.pi - 1e-7, np.pi):
        for _ in range(5):
            ax = rng.normal(size=3)
            r = ax / np.linalg.norm(ax) * theta
            R = rodrigues(r)
            assert R.shape == (3, 3) and np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14
            assert np.array_equal(R, rodrigues(r.reshape(3, 1))) and np.array_equal(R, rodrigues(r.reshape(1, 3)))
            back = rodrigues(R)
            assert back.shape == (3, 1)
            # near pi the axis comes from sqrt((R_ii + 1) / 2): half the digits (1e-7); r and -r are then the same rotation.
            # Below cv2's 1e-5 rule the vector is 0 and R differs from I by theta itself (1e-7 here): 2e-7 covers both.
            assert np.abs(rodrigues(back) - R).max() < 2e-7
            if theta < 1e-5:                                                     # cv2's rule: sin(theta) below 1e-5 is no rotation
                assert (back == 0).all()
            elif theta < 3.1:
                assert np.abs(back[:, 0] - r).max() < 1e-9
    assert np.abs(rodrigues(np.array([0.0, 0.0, np.pi / 2])) - [[0, -1, 0], [1, 0, 0], [0, 0, 1]]).max() < 1e-15   # counter-clockwise
    with pytest.raises(ValueError, match='rotation vector'):
        rodrigues(np.zeros(4))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
NAMES = ('cotr_lift_pixels', 'cotr_ransac_pnp', 'cotr_ransac_pnp_scratch_bytes')


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

    def cam(i, j, v):
        k = K.copy()
        k[i, j] = v
        return K9(*k.reshape(9))
    for n in (3, (1 << 24) + 1):
        assert lib.cotr_ransac_pnp_scratch_bytes(n, 100, ctypes.byref(b)) == -1 and b'[4, 2^24]' in lib.cotr_raster_last_error()
    for iters in (0, (1 << 16) + 1):
        assert lib.cotr_ransac_pnp_scratch_bytes(100, iters, ctypes.byref(b)) == -1 and b'max_iters' in lib.cotr_raster_last_error()
    assert lib.cotr_ransac_pnp_scratch_bytes(100, 100, None) == -1 and b'NULL' in lib.cotr_raster_last_error()
    assert lib.cotr_ransac_pnp_scratch_bytes(4, 1, ctypes.byref(b)) == 0 and b.value >= 76 + 29 * 8
    assert lib.cotr_ransac_pnp_scratch_bytes(1 << 24, 1 << 16, ctypes.byref(b)) == 0 and b.value >= 65536 * 76 + 8192 * 29 * 8
    assert lib.cotr_ransac_pnp_scratch_bytes(100, 100, ctypes.byref(b)) == 0
    need = b.value

    def call(n=100, thr=8.0, conf=0.99, iters=100, refine=10, obj=P, k=good, R=P, t=P, scratch=P, nbytes=need, hyp=None):
        return lib.cotr_ransac_pnp(obj, P, n, k, thr, conf, iters, 0, refine, R, t, P, P, hyp, None, None, scratch, nbytes, None)
    for kw, word in ((dict(n=3), b'[4, 2^24]'), (dict(n=(1 << 24) + 1), b'[4, 2^24]'), (dict(iters=0), b'max_iters'),
                     (dict(iters=(1 << 16) + 1), b'max_iters'), (dict(thr=0.0), b'threshold'), (dict(thr=-1.0), b'threshold'),
                     (dict(thr=float('nan')), b'threshold'), (dict(thr=float('inf')), b'threshold'), (dict(thr=1e30), b'squared threshold'),
                     (dict(thr=1e-30), b'squared threshold'), (dict(conf=0.0), b'confidence'), (dict(conf=1.0), b'confidence'),
                     (dict(conf=float('nan')), b'confidence'), (dict(refine=-1), b'refine_iters'), (dict(refine=65), b'refine_iters'),
                     (dict(obj=None), b'NULL'), (dict(k=None), b'NULL'), (dict(R=None), b'NULL'), (dict(t=None), b'NULL'),
                     (dict(scratch=None), b'NULL'), (dict(k=cam(0, 0, 0.0)), b'focal'), (dict(k=cam(1, 1, float('nan'))), b'focal'),
                     (dict(k=cam(0, 2, float('inf'))), b'finite'), (dict(k=cam(0, 1, float('nan'))), b'finite'),
                     (dict(t=ctypes.c_void_p(4100)), b'aligned'), (dict(scratch=ctypes.c_void_p(4104)), b'aligned'),
                     (dict(hyp=ctypes.c_void_p(4100)), b'aligned'), (dict(nbytes=need - 1), b'smaller')):
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())

    def lift(H=10, W=12, n=5, depth=P, k=good, c2w=None, pts=P, out=P):
        return lib.cotr_lift_pixels(depth, H, W, k, c2w, pts, n, out, None)
    for kw, word in ((dict(H=0), b'H and W'), (dict(W=0), b'H and W'), (dict(H=1 << 15, W=1 << 14), b'2^28'), (dict(n=0), b'[1, 2^24]'),
                     (dict(n=(1 << 24) + 1), b'[1, 2^24]'), (dict(depth=None), b'NULL'), (dict(k=None), b'NULL'), (dict(pts=None), b'NULL'),
                     (dict(out=None), b'NULL'), (dict(k=cam(1, 1, 0.0)), b'focal'), (dict(k=cam(1, 2, float('nan'))), b'finite'),
                     (dict(depth=ctypes.c_void_p(4098)), b'aligned'), (dict(c2w=ctypes.c_void_p(4100)), b'aligned'),
                     (dict(out=ctypes.c_void_p(4100)), b'aligned')):
        assert lift(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
def _capture(depth=None, K_=K, c2w=None):
    from cotr_amd.data import Capture
    return Capture(None, np.ones((10, 12), np.float32) if depth is None else depth, K_, np.eye(4) if c2w is None else c2w)


def test_wrapper_argument_errors_without_a_gpu():
    o, p = np.zeros((20, 3)), np.zeros((20, 2))
    for fn in (ransac_pnp, solve_pnp_ransac):
        with pytest.raises(ValueError, match='at least 4'):
            fn(np.zeros((3, 3)), np.zeros((3, 2)), K)
        with pytest.raises(ValueError, match='same length'):
            fn(o, np.zeros((21, 2)), K)
        with pytest.raises(ValueError, match=r'\[N, 3\]'):
            fn(p, p, K)
        with pytest.raises(ValueError, match=r'\[N, 2\]'):
            fn(o, o, K)
        with pytest.raises(ValueError, match=r'\[3, 3\]'):
            fn(o, p, np.eye(4))
        with pytest.raises(ValueError, match='focal'):
            fn(o, p, np.diag([0.0, 500.0, 1.0]))
        with pytest.raises(ValueError, match='focal'):
            fn(o, p, np.diag([500.0, np.nan, 1.0]))
        with pytest.raises(ValueError, match='refine_iters'):
            fn(o, p, K, refine_iters=-1)
        with pytest.raises(ValueError, match='refine_iters'):
            fn(o, p, K, refine_iters=65)
    for kw, word in ((dict(max_iters=0), 'max_iters'), (dict(max_iters=(1 << 16) + 1), 'max_iters'), (dict(threshold=0.0), 'threshold'),
                     (dict(threshold=float('inf')), 'threshold'), (dict(threshold=float('nan')), 'threshold'), (dict(threshold=1e30), 'squared'),
                     (dict(confidence=0.0), 'confidence'), (dict(confidence=1.0), 'confidence')):
        with pytest.raises(ValueError, match=word):
            ransac_pnp(o, p, K, **kw)
        with pytest.raises(ValueError, match=word):
            localize(p, p, _capture(), K, **kw)
    with pytest.raises(ValueError, match='max_iters'):
        solve_pnp_ransac(o, p, K, iterations_count=0)
    with pytest.raises(ValueError, match='threshold'):
        solve_pnp_ransac(o, p, K, reprojection_error=0.0)
    with pytest.raises(ValueError, match='confidence'):
        solve_pnp_ransac(o, p, K, confidence=1.0)
    with pytest.raises(ValueError, match='dist_coeffs'):
        solve_pnp_ransac(o, p, K, np.array([0.1, 0, 0, 0]))
    with pytest.raises(ValueError, match='max_iters'):                           # zero distortion passes that check
        solve_pnp_ransac(o, p, K, np.zeros(5), iterations_count=0)
    # lift_pixels and localize
    d = np.ones((10, 12), np.float32)
    for bad, word in ((dict(points=np.zeros((5, 3))), r'\[N, 2\]'), (dict(points=np.zeros((0, 2))), 'between 1'), (dict(depth=d.astype(np.float64)), 'float32'),
                      (dict(depth=np.ones(5, np.float32)), r'\[H, W\]'), (dict(K=np.eye(2)), r'\[3, 3\]'), (dict(K=np.diag([1.0, 0.0, 1.0])), 'focal'),
                      (dict(c2w=np.eye(3)), r'\[4, 4\]'), (dict(c2w=np.full((4, 4), np.nan)), r'\[4, 4\]')):
        kw = dict(points=np.zeros((5, 2)), depth=d, K=K, c2w=None)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            lift_pixels(**kw)
    with pytest.raises(ValueError, match='at least 4'):
        localize(np.zeros((3, 2)), np.zeros((3, 2)), _capture(), K)
    with pytest.raises(ValueError, match='same length'):
        localize(p, np.zeros((21, 2)), _capture(), K)
    with pytest.raises(ValueError, match='float32'):
        localize(p, p, _capture(depth=np.ones((10, 12))), K)
    with pytest.raises(ValueError, match=r'\[4, 4\]'):
        localize(p, p, _capture(c2w=np.eye(3)), K)
    with pytest.raises(ValueError, match='focal'):
        localize(p, p, _capture(), np.diag([0.0, 1.0, 1.0]))
    with pytest.raises(TypeError, match='unexpected keyword'):
        localize(p, p, _capture(), K, treshold=1.0)


def test_cpu_tensors_are_refused():
    o, p = torch.zeros((20, 3), dtype=torch.float64), torch.zeros((20, 2), dtype=torch.float64)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        ransac_pnp(o, p.numpy(), K)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        solve_pnp_ransac(o.numpy(), p, K)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        lift_pixels(p, np.ones((10, 12), np.float32), K)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        lift_pixels(p.numpy(), torch.ones((10, 12)), K)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        localize(p, p.numpy(), _capture(), K)


def test_zoom_engine_localize_host_logic(monkeypatch):
    from cotr_amd.inference import FasterSparseEngine, SparseEngine, ZoomEngine, pnp
    assert SparseEngine.localize is ZoomEngine.localize and FasterSparseEngine.localize is ZoomEngine.localize
    want = np.random.default_rng(0).uniform(0, 100, (12, 4))
    calls = []

    def fake(pa, pb, cap, K_b, **kw):
        calls.append((pa.copy(), pb.copy(), cap, K_b, kw))
        return 'c2w', 'mask'
    monkeypatch.setattr(pnp, 'localize', fake)

    class Spy(ZoomEngine):
        def __init__(self):
            self.calls = []

        def cotr_corr_multiscale(self, img_a, img_b, zoom_ins=(1.0,), converge_iters=1, max_corrs=1000, queries_a=None, **kw):
            self.calls.append((img_a, img_b, tuple(zoom_ins), converge_iters, max_corrs, None if queries_a is None else queries_a.shape, kw))
            return want
    from cotr_amd.data import Capture
    cap = Capture('image', 'depth', 'K', 'c2w')
    spy, zooms = Spy(), np.linspace(0.5, 0.0625, 4)
    c2w, corrs, mask = spy.localize(cap, 'b', 'Kb', max_corrs=77, seed=3)
    assert (c2w, mask) == ('c2w', 'mask') and np.array_equal(corrs, want)
    c2w, corrs, mask = spy.localize(cap, 'b', 'Kb', queries_a=np.zeros((12, 2)), converge_iters=2, threshold=2.0)
    assert (c2w, mask) == ('c2w', 'mask') and np.array_equal(corrs, want)
    assert spy.calls == [('image', 'b', tuple(zooms), 1, 77, None, {}), ('image', 'b', tuple(zooms), 2, 1000, (12, 2), {'force': True})]
    assert [c[2:] for c in calls] == [(cap, 'Kb', {'seed': 3}), (cap, 'Kb', {'threshold': 2.0})]
    assert all(np.array_equal(c[0], want[:, :2]) and np.array_equal(c[1], want[:, 2:]) for c in calls)
