"""N-view triangulation without a GPU: the numpy restatement (tests/structure_oracle.py) against ground truth, against
central differences and against a second route through the demo's own steps, the pair vote's order and tie rules, robust
recovery on planted outlier views, the dependence of the fit on the order of its sums, and the argument checks of the C ABI
(they run before any HIP call) and of the Python wrappers."""
import ctypes
import os

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.build import declared_symbols
from cotr_amd.inference import stack_views, triangulate_points, triangulate_views
from cotr_amd.inference.structure import reconstruct_tensors, triangulate_points_tensors
from tests import structure_oracle as so

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'structure_demo.npz')


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_dyadic_scenes_reproduce_the_points():
    # Pixels, cameras and poses are dyadic, so the true point has residual exactly 0 in every view.  The rays are normalised
    # (a square root), so the ray least squares is not exact: three views a unit apart at depth 4 give the 3 x 3 system a
    # condition number of some tens, and 1000 eps |X| bounds X0.  Gauss-Newton then converges onto the zero-residual point:
    # 64 eps |X|.  No step from the exact point is kept: the error cannot fall below 0.
    d = so.dyadic_scene()
    tab = so.prepare(d['cams'], d['poses'])
    for v in range(3):
        r = so.project(tab, v, d['points'][v, :, 0], d['points'][v, :, 1], list(d['X'].T))
        assert (r['e'] == 0).all() and (r['z'] > 0).all()
    eps, size = np.finfo(np.float64).eps, np.abs(d['X']).max()
    r0 = so.triangulate(d['points'], d['cams'], d['poses'], robust=False, refine_iters=0)
    r10 = so.triangulate(d['points'], d['cams'], d['poses'], robust=False, refine_iters=10)
    rr = so.triangulate(d['points'], d['cams'], d['poses'], robust=True, refine_iters=10)
    assert np.abs(r0['X'] - d['X']).max() <= 1000 * eps * size
    assert np.abs(r10['X'] - d['X']).max() <= 64 * eps * size and np.abs(rr['X'] - d['X']).max() <= 64 * eps * size
    assert r10['mask'].all() and r10['used'].all() and rr['used'].all() and list(r10['info'][:7]) == [1, 40, 0, 0, 0, 0, 0]
    sets = np.ones((3, 40), bool)
    err, front, A, g = so.normal(tab, d['points'], sets, list(d['X'].T))
    assert (err == 0).all() and front.all() and all((x == 0).all() for x in g)


def test_jacobian_agrees_with_central_differences():
    sc = so.scene(4, 30, noise=1.0, seed=2)
    tab, pix, sets = so.prepare(sc['cams'], sc['poses']), sc['points'], np.ones((4, 30), bool)
    X = [sc['X'][:, i] + 0.01 for i in range(3)]
    err, _, A, g = so.normal(tab, pix, sets, X)
    h = 1e-6
    J = np.zeros((4, 30, 2, 3))
    for k in range(3):
        lo, hi = [x.copy() for x in X], [x.copy() for x in X]
        lo[k] -= h
        hi[k] += h
        e_lo, e_hi = so.normal(tab, pix, sets, lo)[0], so.normal(tab, pix, sets, hi)[0]
        # d(err)/dX = 2 g: central differences of a smooth function, relative error h^2 ~ 1e-12 plus eps / h ~ 2e-10 of cancellation
        assert np.abs((e_hi - e_lo) / (2 * h) - 2 * g[k]).max() <= 1e-6 * np.abs(2 * g[k]).max()
        for v in range(4):
            a, b = so.project(tab, v, pix[v, :, 0], pix[v, :, 1], lo), so.project(tab, v, pix[v, :, 0], pix[v, :, 1], hi)
            J[v, :, 0, k], J[v, :, 1, k] = (b['du'] - a['du']) / (2 * h), (b['dv'] - a['dv']) / (2 * h)
    JtJ = np.einsum('vnik,vnil->nkl', J, J)
    for i, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        assert np.abs(JtJ[:, a, b] - A[i]).max() <= 1e-6 * np.abs(JtJ).max()


@pytest.mark.parametrize('V,frac', [(2, 0.0), (5, 0.0), (8, 0.25)])
def test_the_error_never_rises_over_kept_steps(V, frac):
    sc = so.scene(V, 200, noise=1.0, outlier_frac=frac, seed=V)
    trace = []
    r = so.triangulate(sc['points'], sc['cams'], sc['poses'], refine_iters=10, trace=trace)
    assert len(trace) >= 2 and r['info'][7] > 0
    for before, after in zip(trace, trace[1:]):
        kept = ~np.isnan(after)
        assert (after[kept] < before[kept]).all()
    # the steps help: refined mean error below the ray least squares' on most points
    r0 = so.triangulate(sc['points'], sc['cams'], sc['poses'], refine_iters=0)
    assert (r['quality'][:, 0] <= r0['quality'][:, 0]).all() and (r['quality'][:, 0] < r0['quality'][:, 0]).mean() > 0.9


def _two_clusters(order):
    """views that see point P and views that see point Q, listed in ``order`` ('P' / 'Q' per view)"""
    base = so.scene(len(order), 12, noise=0.0, seed=6)
    other = so.scene(len(order), 12, noise=0.0, seed=8)   # (a seed at which no third view falls within the threshold by accident)
    seen_q = so.f32(so.observe(other['X'], base['cams'], base['poses'])[0])       # Q through the SAME cameras
    pts = np.stack([(base['points'] if o == 'P' else seen_q)[v] for v, o in enumerate(order)])
    return pts, base, other


def test_pair_order_and_tie_rules():
    kw = dict(robust=True, refine_iters=0, threshold=1.0)
    # two views agree on P, two on Q: a tie at 2 views, and the first pair in lexicographic order keeps it
    for order in ('PPQQ', 'QQPP', 'PQPQ', 'PQQP'):
        pts, base, other = _two_clusters(order)
        r = so.triangulate(pts, base['cams'], base['poses'], **kw)
        first = order[0]
        want = np.array([o == first for o in order])
        assert (r['used'].astype(bool) == want[:, None]).all(), order
        truth = (base if first == 'P' else other)['X']
        assert np.abs(r['X'] - truth).max() < 1e-4                                # float32 pixels
    # the larger count wins wherever its pair stands
    for order in ('QQPPP', 'PQPQP', 'QPPQP'):
        pts, base, other = _two_clusters(order)
        r = so.triangulate(pts, base['cams'], base['poses'], **kw)
        assert (r['used'].astype(bool) == np.array([o == 'P' for o in order])[:, None]).all(), order
    # nothing agrees: one view each of three points -> too few views, or a pair that only fits itself
    base = so.scene(3, 12, noise=0.0, seed=6)
    pts = np.stack([so.f32(so.observe(so.scene(3, 12, noise=0.0, seed=s)['X'], base['cams'], base['poses'])[0])[v] for v, s in enumerate((6, 7, 8))])
    r = so.triangulate(pts, base['cams'], base['poses'], **kw)
    assert (r['used'].sum(axis=0) <= 2).all()
    # robust = 0 takes every visible view
    pts, base, _ = _two_clusters('PPQQ')
    vis = np.ones((4, 12), np.uint8)
    vis[2, :5] = 0
    r = so.triangulate(pts, base['cams'], base['poses'], visible=vis, robust=False)
    assert np.array_equal(r['used'], vis)


@pytest.mark.parametrize('V,frac,noise', [(5, 0.2, 1.0), (8, 0.25, 0.5), (16, 0.25, 0.5)])
def test_robust_mode_recovers_the_planted_views(V, frac, noise):
    sc = so.scene(V, 300, noise=noise, outlier_frac=frac, seed=1)
    assert sc['bad'].any() and not sc['bad'][0].any() and sc['bad'].sum(axis=0).max() <= int(frac * V)
    r = so.triangulate(sc['points'], sc['cams'], sc['poses'], threshold=4.0)
    right = (r['used'].astype(bool) == ~sc['bad']).all(axis=0)
    print(f'V={V}: the planted views recovered on {right.sum()} of 300 points')
    assert right.mean() >= 0.95
    assert np.median(np.linalg.norm(r['X'] - sc['X'], axis=1)) < 0.1


def test_demo_rule_against_the_demos_own_route():
    g = np.load(GOLDEN)
    cases = [tuple(g[k] for k in ('points_a', 'points_b', 'K_a', 'K_b', 'c2w_a', 'c2w_b'))]
    for seed in range(4):
        sc = so.scene(2, 100, noise=1.0, seed=seed)
        cases.append((sc['points'][0], sc['points'][1], so.camera_matrix(sc['cams'][0]), so.camera_matrix(sc['cams'][1]),
                      so.c2w_of(sc['poses'][0]), so.c2w_of(sc['poses'][1])))
    worst = 0.0
    for pa, pb, Ka, Kb, ca, cb in cases:
        cams = np.array([[K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]] for K in (Ka, Kb)])
        r = so.triangulate(np.stack([pa, pb]), cams, np.stack([so.pose_of_c2w(ca), so.pose_of_c2w(cb)]), rule=1, robust=False, refine_iters=0)
        ref = so.demo_route(pa, pb, Ka, Kb, ca, cb)
        assert r['info'][3] == 0 and np.isfinite(r['X']).all()
        worst = max(worst, np.abs(r['X'] - ref).max() / np.abs(ref).max())
    ref = so.nearest_on_ray_a(cases[0][4][:3, 3], g['rays_a'] - cases[0][4][:3, 3], cases[0][5][:3, 3], g['rays_b'] - cases[0][5][:3, 3])
    assert np.abs(ref - so.demo_route(*cases[0])).max() <= 1e-13                  # the recorded rays are the second route's
    print(f'rule 1 against the demo route: largest relative difference {worst:.3e}')
    assert worst <= so.DEMO_ROUTES
    # and the ray least squares of two views is the midpoint of the common perpendicular, not this point: they differ
    pa, pb, Ka, Kb, ca, cb = cases[1]
    cams = np.array([[K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]] for K in (Ka, Kb)])
    poses = np.stack([so.pose_of_c2w(ca), so.pose_of_c2w(cb)])
    mid = so.triangulate(np.stack([pa, pb]), cams, poses, robust=False, refine_iters=0)
    on_a = so.triangulate(np.stack([pa, pb]), cams, poses, rule=1, robust=False, refine_iters=0)
    assert np.abs(mid['X'] - on_a['X']).max() > 1e-4


def test_order_noise():
    # refine_iters = 0: the rounding of the sums through the 3 x 3 solve.  With the refit the last kept step is decided by an
    # error that has stopped falling but for its rounding, so the two orders may stop one step apart: the size of a last step.
    worst = {0: 0.0, 10: 0.0}
    for V, seed in ((3, 0), (5, 1), (8, 2), (16, 3), (32, 4)):
        sc = so.scene(V, 200, noise=0.7, seed=seed)
        for refine in (0, 10):
            up = so.triangulate(sc['points'], sc['cams'], sc['poses'], robust=False, refine_iters=refine)
            down = so.reversed_views(sc['points'], sc['cams'], sc['poses'], robust=False, refine_iters=refine)
            assert np.array_equal(up['used'], down['used']) and np.array_equal(up['mask'], down['mask'])
            worst[refine] = max(worst[refine], (np.abs(up['X'] - down['X']).max(axis=1) / np.abs(up['X']).max(axis=1)).max())
    print(f'ascending against descending sums: largest relative change of X {worst[0]:.3e} (ray least squares), {worst[10]:.3e} (refitted)')
    assert worst[0] <= so.ORDER_NOISE_RAYS and worst[10] <= so.ORDER_NOISE


def test_unsolvable_points_and_counters():
    sc = so.scene(3, 20, noise=0.0, seed=5)
    vis = np.ones((3, 20), np.uint8)
    vis[1:, 0] = 0
    vis[:, 1] = 0
    pts = sc['points'].copy()
    pts[2, 2] = np.nan
    r = so.triangulate(pts, sc['cams'], sc['poses'], visible=vis, robust=False)
    assert np.isnan(r['X'][:2]).all() and np.isnan(r['quality'][:2]).all() and not r['used'][:, :2].any() and not r['mask'][:2].any()
    assert list(r['info']) == [1, 18, 2, 0, 0, 0, 0, r['info'][7]] and list(r['used'][:, 2]) == [1, 1, 0]
    z = so.triangulate(pts, sc['cams'], sc['poses'], found=0)
    assert all((z[k] == 0).all() for k in z)
    poses = sc['poses'].copy()
    poses[1, 3] = np.inf
    r = so.triangulate(sc['points'], sc['cams'], poses, robust=False)
    assert not r['used'][1].any() and r['used'][[0, 2]].all()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
NAMES = ('cotr_triangulate_views', 'cotr_triangulate_views_scratch_bytes')


def test_symbols_are_declared_and_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and name in declared_symbols()
        assert getattr(_lib.load_library(), name) is not None


def test_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    b = ctypes.c_size_t()
    P = ctypes.c_void_p(4096)           # never dereferenced: every call below fails its checks before any HIP call
    for V, n, word in ((1, 10, b'[2, 32]'), (33, 10, b'[2, 32]'), (2, 0, b'[1, 2^24]'), (2, (1 << 24) + 1, b'[1, 2^24]')):
        assert lib.cotr_triangulate_views_scratch_bytes(V, n, ctypes.byref(b)) == -1 and word in lib.cotr_raster_last_error()
    assert lib.cotr_triangulate_views_scratch_bytes(2, 10, None) == -1 and b'NULL' in lib.cotr_raster_last_error()
    assert lib.cotr_triangulate_views_scratch_bytes(32, 1 << 24, ctypes.byref(b)) == 0 and b.value >= 32 * 21 * 8
    need = b.value

    def call(V=3, n=100, thr=4.0, cos=0.999, dist=50.0, refine=10, robust=1, rule=0, pts=P, vis=None, cams=P, poses=P, found=None, X=P,
             used=P, quality=P, mask=P, info=P, scratch=P, nbytes=need):
        return lib.cotr_triangulate_views(pts, vis, cams, poses, V, n, found, thr, cos, dist, refine, robust, rule, X, used, quality, mask, info,
                                          scratch, nbytes, None)
    for kw, word in ((dict(V=1), b'[2, 32]'), (dict(V=33), b'[2, 32]'), (dict(n=0), b'[1, 2^24]'), (dict(n=(1 << 24) + 1), b'[1, 2^24]'),
                     (dict(thr=0.0), b'threshold'), (dict(thr=-1.0), b'threshold'), (dict(thr=float('nan')), b'threshold'),
                     (dict(thr=float('inf')), b'threshold'), (dict(thr=1e30), b'squared threshold'), (dict(thr=1e-30), b'squared threshold'),
                     (dict(cos=1.5), b'max_cos'), (dict(cos=-1.5), b'max_cos'), (dict(cos=float('nan')), b'max_cos'),
                     (dict(dist=0.0), b'distance_thresh'), (dict(dist=float('inf')), b'distance_thresh'), (dict(dist=float('nan')), b'distance_thresh'),
                     (dict(refine=-1), b'refine_iters'), (dict(refine=65), b'refine_iters'), (dict(robust=2), b'robust'), (dict(robust=-1), b'robust'),
                     (dict(rule=2), b'rule'), (dict(rule=-1), b'rule'), (dict(rule=1), b'rule 1'), (dict(rule=1, V=2, robust=0), b'rule 1'),
                     (dict(rule=1, V=2, refine=0), b'rule 1'), (dict(rule=1, V=3, robust=0, refine=0), b'rule 1'),
                     (dict(pts=None), b'NULL'), (dict(cams=None), b'NULL'), (dict(poses=None), b'NULL'), (dict(X=None), b'NULL'),
                     (dict(used=None), b'NULL'), (dict(quality=None), b'NULL'), (dict(mask=None), b'NULL'), (dict(info=None), b'NULL'),
                     (dict(scratch=None), b'NULL'), (dict(pts=ctypes.c_void_p(4104)), b'aligned'), (dict(cams=ctypes.c_void_p(4100)), b'aligned'),
                     (dict(poses=ctypes.c_void_p(4100)), b'aligned'), (dict(X=ctypes.c_void_p(4100)), b'aligned'),
                     (dict(quality=ctypes.c_void_p(4100)), b'aligned'), (dict(info=ctypes.c_void_p(4098)), b'aligned'),
                     (dict(found=ctypes.c_void_p(4098)), b'aligned'), (dict(scratch=ctypes.c_void_p(4104)), b'aligned'),
                     (dict(nbytes=need - 1), b'smaller')):
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
K = np.array([[500.0, 0.5, 320.0], [0.0, 510.0, 240.0], [0.0, 0.0, 1.0]])


def test_wrapper_argument_errors_without_a_gpu():
    pts, cams, poses = np.zeros((3, 20, 2)), np.tile([500.0, 500.0, 320.0, 240.0, 0.0], (3, 1)), np.tile(np.eye(3, 4).reshape(12), (3, 1))
    for bad, word in ((dict(points=np.zeros((20, 2))), r'\[V, N, 2\]'), (dict(points=np.zeros((3, 20, 3))), r'\[V, N, 2\]'),
                      (dict(points=np.zeros((1, 20, 2))), 'between 2 and 32 views'), (dict(points=np.zeros((33, 20, 2))), 'between 2 and 32 views'),
                      (dict(points=np.zeros((3, 0, 2))), 'between 1 and'), (dict(cameras=cams[:2]), 'cameras must be'),
                      (dict(cameras=np.zeros((3, 4))), 'cameras must be'), (dict(cameras=np.eye(4)), 'cameras must be'),
                      (dict(cameras=np.diag([0.0, 500.0, 1.0])), 'focal'), (dict(cameras=np.tile([500.0, np.nan, 0, 0, 0], (3, 1))), 'focal'),
                      (dict(poses=poses[:2]), 'poses must be'), (dict(poses=np.zeros((3, 3, 3))), 'poses must be'),
                      (dict(visible=np.ones((3, 19))), 'visible must be'), (dict(threshold=0.0), 'threshold'), (dict(threshold=float('nan')), 'threshold'),
                      (dict(threshold=float('inf')), 'threshold'), (dict(threshold=1e30), 'squared'), (dict(min_angle=-1.0), 'min_angle'),
                      (dict(min_angle=181.0), 'min_angle'), (dict(min_angle=float('nan')), 'min_angle'), (dict(distance_thresh=0.0), 'distance_thresh'),
                      (dict(distance_thresh=float('inf')), 'distance_thresh'), (dict(refine_iters=-1), 'refine_iters'), (dict(refine_iters=65), 'refine_iters'),
                      (dict(refine_iters=1.5), 'refine_iters'), (dict(rule='midpoint'), 'rule must be'), (dict(rule='demo'), "rule='demo'"),
                      (dict(rule='demo', robust=False, refine_iters=0), "rule='demo'")):
        kw = dict(points=pts, cameras=cams, poses=poses)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            triangulate_views(**kw)
    p = np.zeros((20, 2))
    for fn in (triangulate_points, triangulate_points_tensors):
        for kw, word in ((dict(), 'either R and t'), (dict(R=np.eye(3)), 'either R and t'), (dict(c2w1=np.eye(4)), 'either R and t'),
                         (dict(R=np.eye(3), t=np.zeros(3), c2w1=np.eye(4), c2w2=np.eye(4)), 'either R and t'),
                         (dict(R=np.eye(4), t=np.zeros(3)), r'R must be \[3, 3\]'), (dict(R=np.eye(3), t=np.zeros(4)), 't must have 3'),
                         (dict(c2w1=np.eye(3), c2w2=np.eye(4)), r'c2w1 must be a finite \[4, 4\]'),
                         (dict(c2w1=np.eye(4), c2w2=np.full((4, 4), np.nan)), r'c2w2 must be a finite \[4, 4\]')):
            with pytest.raises(ValueError, match=word):
                fn(p, p, K, **kw)
        with pytest.raises(ValueError, match='same length'):
            fn(p, np.zeros((21, 2)), K, R=np.eye(3), t=np.zeros(3))
        with pytest.raises(ValueError, match=r'\[N, 2\]'):
            fn(np.zeros((20, 3)), p, K, R=np.eye(3), t=np.zeros(3))
        with pytest.raises(ValueError, match=r'\[3, 3\]'):
            fn(p, p, np.eye(4), R=np.eye(3), t=np.zeros(3))
        with pytest.raises(ValueError, match='focal'):
            fn(p, p, K, np.diag([0.0, 1.0, 1.0]), R=np.eye(3), t=np.zeros(3))
    img = np.zeros((10, 12, 3), np.uint8)
    for kw, word in ((dict(corrs=np.zeros((5, 3))), r'\[N, 4\]'), (dict(c2w_a=np.eye(4)), 'both c2w_a and c2w_b'), (dict(img_a=np.zeros((10, 12))), r'\[H, W, 3\]'),
                     (dict(img_b=np.zeros((10, 12, 4))), r'\[H, W, 3\]')):
        args = dict(corrs=np.zeros((5, 4)), img_a=img, img_b=img, K_a=K, K_b=K)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            reconstruct_tensors(**args)


def test_cpu_tensors_are_refused():
    pts, cams, poses = torch.zeros((3, 20, 2), dtype=torch.float64), np.tile([500.0, 500.0, 320.0, 240.0, 0.0], (3, 1)), np.tile(np.eye(3, 4).reshape(12), (3, 1))
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        triangulate_views(pts, cams, poses)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        triangulate_views(pts.numpy(), cams, torch.from_numpy(poses))
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        triangulate_views(pts.numpy(), cams, poses, visible=torch.ones((3, 20), dtype=torch.uint8))
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        triangulate_views(pts.numpy(), cams, poses, found=torch.ones(8, dtype=torch.int32))
    p = torch.zeros((20, 2), dtype=torch.float64)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        triangulate_points(p, p.numpy(), K, R=np.eye(3), t=np.zeros(3))
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        triangulate_points(p.numpy(), p.numpy(), K, R=torch.eye(3, dtype=torch.float64), t=np.zeros(3))


def test_stack_views():
    rng = np.random.default_rng(0)
    q = rng.uniform(0, 100, (15, 2))
    corrs = [np.concatenate([q, rng.uniform(0, 100, (15, 2))], axis=1) for _ in range(3)]
    pts = stack_views(corrs)
    assert pts.shape == (4, 15, 2) and pts.dtype == np.float64 and np.array_equal(pts[0], q)
    assert all(np.array_equal(pts[i + 1], c[:, 2:]) for i, c in enumerate(corrs))
    assert stack_views([c.astype(np.float32) for c in corrs]).dtype == np.float64
    with pytest.raises(ValueError, match='at least one'):
        stack_views([])
    with pytest.raises(ValueError, match=r'\[N, 4\]'):
        stack_views([corrs[0], corrs[1][:10]])
    with pytest.raises(ValueError, match=r'\[N, 4\]'):
        stack_views([corrs[0][:, :3]])
    with pytest.raises(ValueError, match='same rows'):
        stack_views([corrs[0], corrs[1][::-1]])


def test_zoom_engine_reconstruct_host_logic(monkeypatch):
    from cotr_amd.inference import FasterSparseEngine, SparseEngine, ZoomEngine, structure
    assert SparseEngine.reconstruct is ZoomEngine.reconstruct and FasterSparseEngine.reconstruct is ZoomEngine.reconstruct
    want = np.random.default_rng(0).uniform(0, 100, (12, 4))
    calls = []

    def fake(corrs, *args, **kw):
        calls.append((corrs.copy(), args, kw))
        return 'result'
    monkeypatch.setattr(structure, 'reconstruct_tensors', fake)

    class Spy(ZoomEngine):
        def __init__(self):
            self.calls = []

        def cotr_corr_multiscale(self, img_a, img_b, zoom_ins=(1.0,), converge_iters=1, max_corrs=1000, queries_a=None, **kw):
            self.calls.append((img_a, img_b, tuple(zoom_ins), converge_iters, max_corrs, None if queries_a is None else queries_a.shape, kw))
            return want
    spy, zooms = Spy(), np.linspace(0.5, 0.0625, 4)
    assert spy.reconstruct('a', 'b', 'Ka', 'Kb', 'ca', 'cb', max_corrs=77, rule='demo') == 'result'
    assert spy.reconstruct('a', 'b', 'Ka', 'Kb', queries_a=np.zeros((12, 2)), converge_iters=2, threshold=2.0, pose_kw=dict(seed=3)) == 'result'
    assert spy.calls == [('a', 'b', tuple(zooms), 1, 77, None, {}), ('a', 'b', tuple(zooms), 2, 1000, (12, 2), {'force': True})]
    assert [c[1:] for c in calls] == [(('a', 'b', 'Ka', 'Kb', 'ca', 'cb'), dict(rule='demo', pose_kw=None)),
                                      (('a', 'b', 'Ka', 'Kb', None, None), dict(rule='rays', pose_kw=dict(seed=3), threshold=2.0))]
    assert all(np.array_equal(c[0], want) for c in calls)
