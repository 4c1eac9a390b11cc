"""N-view triangulation on the MI355X (cotr_triangulate_views in cotr_amd/csrc/structure.hip) against the numpy restatement
tests/structure_oracle.py: every output bit for bit at every shape edge, view count and mode, the demo's rule against its
restatement and against ray points recorded from the reference's projector, degenerate input, repeatability, the chains after
``relative_pose_tensors`` and ``localize``, and the engine call built on it.

Every point is summed by one thread in the restatement's order and no product is contracted, so X, used, quality, mask and
info are expected to be the restatement's bits.  Measured on an MI355X: they are, in every case below, so the tests assert
equality and no bound from the order noise is used; the demo rule lies 2.8e-14 from the recorded rays (1.1e-10 allowed) and the
localize chain 2.9e-7 of the distance from the lifted points, as the restatement of the whole chain does."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import ZoomEngine, stack_views, triangulate_points, triangulate_views
from cotr_amd.inference.structure import reconstruct_tensors, triangulate_points_tensors
from tests import structure_oracle as so

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'structure_demo.npz')
KEYS = ('X', 'used', 'quality', 'mask', 'info')


def host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items() if torch.is_tensor(v)}


def same_bits(got, want, what=''):
    for k in KEYS:
        g, w = got[k], want[k]
        if g.dtype == bool:
            g = g.astype(np.uint8)
        if not np.array_equal(g, w, equal_nan=True):
            with np.errstate(all='ignore'):
                diff = np.nanmax(np.abs(g.astype(np.float64) - w.astype(np.float64)) / np.maximum(np.abs(w.astype(np.float64)), 1e-300))
            print(f'{what} {k}: {(g != w).sum()} entries differ, largest relative difference {diff:.3e}')
        assert np.array_equal(g, w, equal_nan=True), (what, k)


@functools.lru_cache(maxsize=None)
def _scene(V, N):
    return so.scene(V, N, noise=0.7, outlier_frac=0.34 if V >= 3 else 0.0, seed=100 * V + N)


def _visibles(V, N):
    rng = np.random.default_rng(V + N)
    rand = rng.random((V, N)) < 0.8
    few = rand.copy()
    few[1:, 0] = False                 # point 0: one view
    few[:, N // 2] = False             # and one point: none
    return (('all', None), ('random', rand.astype(np.uint8)), ('few', few.astype(np.uint8) * 3))


def _compare(V, N, modes):
    sc = _scene(V, N)
    for name, vis in _visibles(V, N):
        for robust, refine in modes:
            kw = dict(visible=vis, robust=bool(robust), refine_iters=refine)
            want = so.triangulate(sc['points'], sc['cams'], sc['poses'], **kw)
            got = host(triangulate_views(sc['points'], sc['cams'], sc['poses'], **kw))
            same_bits(got, want, f'V={V} N={N} visible={name} robust={robust} refine={refine}')
            assert want['info'][1] + want['info'][2:7].sum() == N
            if name == 'few':
                assert want['info'][2] >= min(2, N) and np.isnan(got['X'][0]).all() and not got['used'][:, N // 2].any()


ALL_MODES = [(r, k) for r in (0, 1) for k in (0, 1, 10)]


@pytest.mark.parametrize('V', [2, 3, 5])
@pytest.mark.parametrize('N', [1, 63, 64, 65, 255, 256, 257, 1025])
def test_every_output_bit_for_bit(N, V):
    _compare(V, N, ALL_MODES)


def test_thirty_two_views_bit_for_bit():
    sc = _scene(32, 65)
    vis = _visibles(32, 65)[1][1]
    for robust, refine in ((0, 0), (0, 10), (1, 10)):
        kw = dict(visible=vis, robust=bool(robust), refine_iters=refine)
        want = so.triangulate(sc['points'], sc['cams'], sc['poses'], **kw)
        same_bits(host(triangulate_views(sc['points'], sc['cams'], sc['poses'], **kw)), want, f'V=32 robust={robust} refine={refine}')
        if robust:
            assert (want['used'].astype(bool) == (~sc['bad'] & (vis != 0))).all(axis=0).mean() >= 0.95


def test_outputs_and_recovery():
    sc = so.scene(8, 300, noise=0.5, outlier_frac=0.25, seed=3)
    r = triangulate_views(sc['points'], sc['cams'].astype(np.float32).astype(np.float64), sc['poses'].reshape(8, 3, 4))
    assert all(v.is_cuda for v in r.values())
    assert (r['X'].dtype, tuple(r['X'].shape)) == (torch.float64, (300, 3)) and (r['used'].dtype, tuple(r['used'].shape)) == (torch.bool, (8, 300))
    assert (r['quality'].dtype, tuple(r['quality'].shape)) == (torch.float64, (300, 5)) and (r['mask'].dtype, tuple(r['mask'].shape)) == (torch.bool, (300,))
    assert (r['info'].dtype, tuple(r['info'].shape)) == (torch.int32, (8,))
    h = host(r)
    assert (h['used'] == ~sc['bad']).all(axis=0).mean() >= 0.95 and h['mask'].mean() >= 0.95
    # 0.5 px of noise at 500 px of focal length, depths up to 9, a baseline of 4.2 over 8 views: centimetres
    assert np.median(np.linalg.norm(h['X'] - sc['X'], axis=1)) < 0.05
    # [V,3,3] camera matrices and device tensors give the same call
    Ks = np.stack([so.camera_matrix(c) for c in sc['cams']])
    q = host(triangulate_views(torch.from_numpy(sc['points']).cuda(), torch.from_numpy(Ks).cuda(), torch.from_numpy(sc['poses']).cuda()))
    same_bits(q, so.triangulate(sc['points'], sc['cams'], sc['poses']), 'tensors')


def test_masks_and_counters_on_fixtures_with_a_margin():
    # every filter trips for some points, and no figure lies within 1e-6 (relative) of its threshold
    sc = so.scene(5, 257, noise=0.7, outlier_frac=0.0, seed=8)
    sc['points'][3, ::9] += 9.0                                                   # beyond 4 px in one view
    for kw in (dict(robust=False, distance_thresh=7.0, min_angle=20.0), dict(robust=True, distance_thresh=7.0, min_angle=20.0)):
        want = so.triangulate(sc['points'], sc['cams'], sc['poses'], **kw)
        q, max_cos = want['quality'], np.cos(np.deg2rad(kw['min_angle']))
        ok = ~np.isnan(q[:, 0])
        for figure, limit in ((q[ok, 1], 16.0), (q[ok, 3], 7.0), (q[ok, 4], max_cos)):
            assert (np.abs(figure / limit - 1) > 1e-6).all()
        assert want['info'][1] > 0 and want['info'][4] > 0 and want['info'][6] > 0 and (kw['robust'] or want['info'][5] > 0)
        same_bits(host(triangulate_views(sc['points'], sc['cams'], sc['poses'], **kw)), want, str(kw))


def test_demo_rule_against_its_restatement_and_the_recorded_rays():
    g = np.load(GOLDEN)
    pa, pb, Ka, Kb, ca, cb = (g[k] for k in ('points_a', 'points_b', 'K_a', 'K_b', 'c2w_a', 'c2w_b'))
    cams = np.array([[K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]] for K in (Ka, Kb)])
    poses = np.stack([so.pose_of_c2w(ca), so.pose_of_c2w(cb)])
    kw = dict(robust=False, refine_iters=0)
    want = so.triangulate(np.stack([pa, pb]), cams, poses, rule=1, **kw)
    got = host(triangulate_points_tensors(pa, pb, Ka, Kb, c2w1=ca, c2w2=cb, rule='demo', **kw))
    # the wrapper inverts c2w with LAPACK, the restatement's pose_of_c2w transposes: compare through the wrapper's own poses
    w2c = np.stack([np.linalg.inv(m)[:3].reshape(12) for m in (ca, cb)])
    same_bits(got, so.triangulate(np.stack([pa, pb]), cams, w2c, rule=1, **kw), 'demo')
    assert np.abs(got['X'] - want['X']).max() / np.abs(want['X']).max() <= 1000 * so.DEMO_ROUTES
    # the reference's ray points: the point on ray A nearest ray B
    ref = so.nearest_on_ray_a(ca[:3, 3], g['rays_a'] - ca[:3, 3], cb[:3, 3], g['rays_b'] - cb[:3, 3])
    diff = np.abs(got['X'] - ref).max() / np.abs(ref).max()
    print(f'demo rule against the recorded rays: largest relative difference {diff:.3e} (bound {1000 * so.DEMO_ROUTES:.1e})')
    assert diff <= 1000 * so.DEMO_ROUTES
    X, mask = triangulate_points(pa, pb, Ka, Kb, c2w1=ca, c2w2=cb, rule='demo', **kw)
    assert np.array_equal(X, got['X']) and mask.shape == (len(pa), 1) and mask.dtype == np.uint8 and np.array_equal(mask[:, 0], got['mask'])


def test_degenerate_input():
    sc = so.scene(3, 64, noise=0.0, seed=5)
    pts, cams, poses = sc['points'].copy(), sc['cams'].copy(), sc['poses'].copy()
    two = dict(robust=False, refine_iters=10)

    def both(p, c, q, **kw):
        want = so.triangulate(p, c, q, **kw)
        got = host(triangulate_views(p, c, q, **kw))
        same_bits(got, want, str(kw))
        return got
    # parallel rays: two views with one centre and one orientation see the same pixel
    par_poses = np.stack([poses[0], poses[0]])
    r = both(np.stack([pts[0], pts[0]]), np.stack([cams[0], cams[0]]), par_poses, **two)
    assert not r['mask'].any() and r['info'][1] == 0 and r['info'][3] + r['info'][4:7].sum() == 64
    # a point behind a camera: the rays of two views meet behind both
    behind = np.stack([pts[1], pts[0]])
    r = both(behind, cams[:2], poses[:2], **two)
    assert not r['mask'].any() and (r['quality'][~np.isnan(r['quality'][:, 2]), 2] <= 0).all() and r['info'][7] == 0
    # NaN and infinite coordinates: the view drops out for that point; with two views the point does
    bad = pts.copy()
    bad[1, 3], bad[2, 5, 0], bad[0, 7, 1] = np.nan, np.inf, 1e39
    for robust in (False, True):
        r = both(bad, cams, poses, robust=robust)
        assert not r['used'][1, 3] and not r['used'][2, 5] and not r['used'][0, 7] and np.isfinite(r['X']).all()
    r = both(bad[:2], cams[:2], poses[:2], **two)
    assert np.isnan(r['X'][3]).all() and np.isnan(r['X'][7]).all() and r['info'][2] == 2
    # a pose or a camera that is not finite: the view sees nothing
    for i, what in ((5, 'pose'), (2, 'cam')):
        c, q = cams.copy(), poses.copy()
        if what == 'pose':
            q[1, i] = np.nan
        else:
            c[1, i] = np.inf
        want = so.triangulate(pts, c, q, robust=False)
        r = host(triangulate_views(pts, torch.from_numpy(c).cuda(), q, robust=False))   # (a host array is refused before the call)
        same_bits(r, want, what)
        assert not r['used'][1].any() and r['used'][0].all() and r['used'][2].all()
    # found = 0: every output is zero
    r = host(triangulate_views(pts, cams, poses, found=torch.zeros(8, dtype=torch.int32, device='cuda')))
    assert all((r[k] == 0).all() for k in KEYS)
    same_bits(host(triangulate_views(pts, cams, poses, found=torch.ones(8, dtype=torch.int32, device='cuda'))),
              so.triangulate(pts, cams, poses), 'found=1')
    # one point 64 times
    rep = np.repeat(pts[:, 9:10], 64, axis=1)
    r = both(rep, cams, poses)
    assert (r['X'] == r['X'][0]).all() and (r['quality'] == r['quality'][0]).all() and r['mask'].all()


def test_same_bits_across_calls_streams_scratch_and_graph_replay():
    V, n = 6, 3000
    sc = so.scene(V, n, noise=0.7, outlier_frac=0.25, seed=4)
    d = [torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ('points', 'cams', 'poses')]
    first = host(triangulate_views(*d))
    again = host(triangulate_views(*d))
    assert first['info'][1] > 0.9 * n and first['info'][7] >= n
    for k in KEYS:
        assert np.array_equal(first[k], again[k], equal_nan=True), k
    lib = _lib.load_library()
    nbytes = ctypes.c_size_t()
    assert lib.cotr_triangulate_views_scratch_bytes(V, n, ctypes.byref(nbytes)) == 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    max_cos = float(np.cos(np.deg2rad(1.5)))

    def buffers():
        return dict(s=torch.full((nbytes.value + 4096,), 0xA5, dtype=torch.uint8, device='cuda'), X=torch.full((n, 3), -7.0, dtype=torch.float64, device='cuda'),
                    used=torch.full((V, n), 9, dtype=torch.uint8, device='cuda'), quality=torch.full((n, 5), -7.0, dtype=torch.float64, device='cuda'),
                    mask=torch.full((n,), 9, dtype=torch.uint8, device='cuda'), info=torch.full((8,), -3, dtype=torch.int32, device='cuda'))

    def enqueue(b, stream):
        rc = lib.cotr_triangulate_views(p(d[0]), None, p(d[1]), p(d[2]), V, n, None, 4.0, max_cos, 50.0, 10, 1, 0, p(b['X']), p(b['used']),
                                        p(b['quality']), p(b['mask']), p(b['info']), p(b['s']), nbytes.value + 4096, stream)
        assert rc == 0, lib.cotr_raster_last_error()

    def same(b):
        for k in KEYS:
            g = b[k].cpu().numpy()
            assert np.array_equal(g, first[k].astype(g.dtype), equal_nan=True), k
    b = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    enqueue(b, ctypes.c_void_p(side.cuda_stream))
    side.synchronize()
    same(b)
    # captured once (a single linear chain on the capture stream), replayed once
    b = buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue(b, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    graph.replay()
    torch.cuda.synchronize()
    same(b)


def test_relative_pose_into_triangulate_points():
    from cotr_amd.inference.essential import relative_pose_tensors
    from tests import essential_oracle as eo
    for seed in (0, 1):
        p1, p2, K1, K2 = eo.two_view_scene(300, 0.2, seed)[:4]
        kw = dict(threshold=1.0, confidence=0.999, max_iters=200, seed=seed, refine_rounds=4)
        pose = relative_pose_tensors(p1, p2, K1, K2, **kw)
        chained = host(triangulate_points_tensors(p1, p2, K1, K2, R=pose['R'], t=pose['t'], found=pose['info']))
        h = host(pose)
        assert h['info'][0]
        apart = host(triangulate_points_tensors(p1, p2, K1, K2, R=h['R'], t=h['t']))
        same_bits(chained, apart, 'chain')
        cams = np.array([[K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]] for K in (K1, K2)])
        poses = np.stack([so.pose_rows(np.eye(3), np.zeros(3)), so.pose_rows(h['R'], h['t'])])
        same_bits(chained, so.triangulate(np.stack([p1, p2]), cams, poses), 'chain against the restatement')
        # the pose's inliers (Sampson error within 1 px, in front of both cameras) that pass the filters re-project within the threshold
        inl = h['mask'] & chained['mask']
        assert inl.sum() >= 0.9 * h['mask'].sum()
        pix, z = so.observe(chained['X'][inl], cams, poses)
        assert (z > 0).all() and (((pix - so.f32(np.stack([p1, p2]))[:, inl]) ** 2).sum(axis=2) <= 16.0).all()


def test_localized_pose_triangulates_back_onto_the_lifted_depth():
    from cotr_amd.data import depth_corrs
    from cotr_amd.inference.pnp import localize
    from cotr_amd.utils.synth import synth_scene
    from tests import pnp_oracle as po
    cap_a, cap_b = synth_scene(25, 4, 96, 128)[:2]
    H, W = cap_a.depth.shape
    corrs = depth_corrs(cap_a, cap_b, subset=np.random.default_rng(5).permutation(H * W)[:600].astype(np.int64)).cpu().numpy()
    pa, pb = corrs[:, :2], corrs[:, 2:]
    assert len(pa) >= 200
    rk = dict(threshold=1.0, confidence=0.999, max_iters=100, seed=2)
    c2w_b, mask = localize(pa, pb, cap_a, cap_b.K, **rk)
    assert c2w_b is not None and mask.mean() > 0.9
    lifted = po.lift(pa, cap_a.depth, cap_a.K, cap_a.c2w)
    kw = dict(threshold=1.0, min_angle=0.5)
    X, m = triangulate_points(pa, pb, cap_a.K, cap_b.K, c2w1=cap_a.c2w, c2w2=c2w_b, **kw)
    # the bound: the restatement of the whole chain (its own P3P RANSAC and refit, then its own triangulation), times 10
    o = po.ransac(lifted, pb, cap_b.K, rk['threshold'], rk['confidence'], rk['max_iters'], rk['seed'])
    assert o['info'][0]
    cams = np.array([[K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]] for K in (cap_a.K, cap_b.K)])
    want = so.triangulate(np.stack([pa, pb]), cams, np.stack([so.pose_of_c2w(cap_a.c2w), so.pose_rows(o['R'], o['t'])]), **kw)
    ok = (m[:, 0] != 0) & (want['mask'] != 0)
    assert ok.mean() >= 0.9
    dist = lambda Y: np.linalg.norm(Y[ok] - lifted[ok], axis=1) / np.linalg.norm(lifted[ok] - cap_a.c2w[:3, 3], axis=1)   # noqa: E731
    d_dev, d_ref = dist(X).max(), dist(want['X']).max()
    print(f'triangulated against lifted points, relative to the distance: device {d_dev:.3e}, restatement {d_ref:.3e}')
    assert d_dev <= 10 * d_ref


def test_stack_views_many_view_call():
    sc = so.scene(4, 50, noise=0.3, seed=2)
    corrs = [np.concatenate([sc['points'][0], sc['points'][v]], axis=1) for v in (1, 2, 3)]
    pts = stack_views(corrs)
    assert pts.shape == (4, 50, 2) and np.array_equal(pts, sc['points'])
    same_bits(host(triangulate_views(pts, sc['cams'], sc['poses'])), so.triangulate(sc['points'], sc['cams'], sc['poses']), 'stacked')


def test_zoom_engine_reconstruct():
    from tests.engine_fixtures import CyclicFakeModel, synthetic_pair
    img_a, img_b = synthetic_pair(1)
    (Ha, Wa), (Hb, Wb) = img_a.shape[:2], img_b.shape[:2]
    K_a = np.array([[300.0, 0.5, Wa / 2], [0.0, 310.0, Ha / 2], [0.0, 0.0, 1.0]])
    K_b = np.array([[280.0, -0.5, Wb / 2], [0.0, 290.0, Hb / 2], [0.0, 0.0, 1.0]])
    c2w_a, c2w_b = so.c2w_of(so.pose_rows(np.eye(3), np.zeros(3))), so.c2w_of(so.pose_rows(so.rotation([0.0, 0.2, 0.0]), [-1.0, 0.0, 0.1]))
    eng = ZoomEngine(CyclicFakeModel().cuda())
    rng = np.random.default_rng(0)
    q = np.stack([rng.uniform(5, Wa - 5, 40), rng.uniform(5, Ha - 5, 40)], 1).astype(np.float32)
    with torch.no_grad():
        want = np.asarray(eng.cotr_corr_multiscale(img_a, img_b, np.linspace(0.5, 0.0625, 4), 1, max_corrs=1000, queries_a=q, force=True))
        posed = eng.reconstruct(img_a, img_b, K_a, K_b, c2w_a, c2w_b, queries_a=q, threshold=50.0)
        demo = eng.reconstruct(img_a, img_b, K_a, K_b, c2w_a, c2w_b, queries_a=q, rule='demo')
        free = eng.reconstruct(img_a, img_b, K_a, K_b, queries_a=q, threshold=50.0, pose_kw=dict(threshold=20.0, max_iters=100, seed=3))
    for r in (posed, demo, free):
        assert np.array_equal(r['corrs'].cpu().numpy(), want.astype(np.float64)) and want.shape == (40, 4)
        assert (r['X'].dtype, tuple(r['X'].shape)) == (torch.float64, (40, 3)) and (r['mask'].dtype, tuple(r['mask'].shape)) == (torch.bool, (40,))
        assert (r['colors'].dtype, tuple(r['colors'].shape)) == (torch.float64, (40, 3)) and r['X'].is_cuda and r['colors'].is_cuda
    pa, pb = want[:, :2].astype(np.float64), want[:, 2:].astype(np.float64)
    same_bits(host(posed), host(triangulate_points_tensors(pa, pb, K_a, K_b, c2w1=c2w_a, c2w2=c2w_b, threshold=50.0)) | {'mask': host(posed)['mask']}, 'posed')
    inside = (np.floor(pb)[:, 0] >= 0) & (np.floor(pb)[:, 0] < Wb) & (np.floor(pb)[:, 1] >= 0) & (np.floor(pb)[:, 1] < Hb)
    fa, fb = np.floor(pa).astype(int), np.floor(np.where(inside[:, None], pb, 0)).astype(int)
    col = (img_a[fa[:, 1], fa[:, 0]] / 255 + img_b[fb[:, 1], fb[:, 0]] / 255) / 2
    col[~inside] = 0
    for r in (posed, demo, free):
        assert np.array_equal(r['colors'].cpu().numpy(), col) and not r['mask'].cpu().numpy()[~inside].any()
    plain = host(triangulate_points_tensors(pa, pb, K_a, K_b, c2w1=c2w_a, c2w2=c2w_b, threshold=50.0))
    assert np.array_equal(host(posed)['mask'], plain['mask'] & inside)
    d = host(triangulate_points_tensors(pa, pb, K_a, K_b, c2w1=c2w_a, c2w2=c2w_b, rule='demo', robust=False, refine_iters=0))
    assert np.array_equal(host(demo)['X'], d['X'], equal_nan=True)
    # without poses: the relative pose and the triangulation as one sequence equal the two calls made one by one
    from cotr_amd.inference.essential import relative_pose_tensors
    pose = host(relative_pose_tensors(pa, pb, K_a, K_b, threshold=20.0, max_iters=100, seed=3, refine_rounds=4))
    assert np.array_equal(host(free['pose'])['R'], pose['R'])
    if pose['info'][0]:
        one = host(triangulate_points_tensors(pa, pb, K_a, K_b, R=pose['R'], t=pose['t'], threshold=50.0))
        assert np.array_equal(host(free)['X'], one['X'], equal_nan=True) and np.array_equal(host(free)['mask'], one['mask'] & inside)
    else:
        assert (host(free)['X'] == 0).all() and not host(free)['mask'].any()
    # an index outside an image: colour 0 and mask 0
    out = want.astype(np.float64).copy()
    out[3, 2], out[5, 1] = Wb + 2.0, -1.0
    r = reconstruct_tensors(out, img_a, img_b, K_a, K_b, c2w_a, c2w_b, threshold=50.0)
    cols, m = r['colors'].cpu().numpy(), r['mask'].cpu().numpy()
    assert (cols[[3, 5]] == 0).all() and not m[[3, 5]].any() and (cols[[0, 1, 2, 4]] > 0).any()
