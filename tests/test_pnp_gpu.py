"""The absolute-pose estimator on the MI355X (cotr_amd/csrc/pnp.hip) against the numpy restatement tests/pnp_oracle.py:
every stage of the RANSAC (samples, candidates, counts, selection, mask) against the same rule, the refit of the device's own
candidate and mask against the restatement's, the pose against the scene's, the lift bit for bit, ``localize`` on two
synthetic captures, degenerate input, repeatability, and the engine call built on it.

The candidate bound: the restatement reaches the candidates by another numerical route (companion-matrix eigenvalues, LAPACK
solves, the SVD rigid motion) than the device (bracketing and bisection, the adjugate, orthonormal frames); two accurate
routes agree to 1e-11 after the three Newton steps, and 1e-7 (the bound of DESIGN.md 3h) is allowed, on at most 1 % of the
iterations not at all.  The refit bound: 1000 times the restatement's own dependence on the order of its sums
(po.ORDER_NOISE = 4.3e-10 -> po.REFIT_BOUND = 4.3e-7 on the entries of R and on t over its norm).
Measured on an MI355X over the seventeen scenes: no iteration differs, the candidates agree within 1.2e-15 to 6.95e-12 (worst
agreement), the device's candidates put their sample points back within 1.08e-10 px (worst residual), and the refit differs
from the restatement's by at most 9.0e-11 in R and 4.23e-10 in t / |t| (n = 63, where the device kept 4 steps and the
restatement 3), below 1e-15 where both keep the same steps."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.data import Capture, depth_corrs
from cotr_amd.inference import ZoomEngine, lift_pixels, localize, ransac_pnp, solve_pnp_ransac
from cotr_amd.inference.pnp import localize_tensors, rodrigues
from tests import pnp_oracle as po

pytestmark = pytest.mark.gpu


def host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _proper(R, tol=1e-12):
    return np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max() < tol and np.abs(np.linalg.det(R) - 1).max() < tol


def check_every_stage(scene):
    n, outl, noise, thr, conf, iters, seed = scene
    ref = po.reference(scene)
    obj, img, K, o = ref['obj'], ref['img'], ref['K'], ref['ransac']
    r = host(ransac_pnp(obj, img, K, thr, conf, iters, seed, refine_iters=0, hypotheses=True))
    smp = o['samples']
    assert np.array_equal(r['samples'], smp)
    # candidates: NaN with count -1 exactly where the restatement has none; rotations; the sample put back; the same pose
    dev, cnt = r['hyp_pose'], r['hyp_count']
    has = cnt >= 0
    assert np.isnan(dev[~has]).all() and np.isfinite(dev[has]).all()
    bad, worst, w_res = 0, 0.0, 0.0
    for it in range(iters):
        if has[it]:   # every device candidate, whatever it is matched to
            Rd, _ = po.expand(dev[it])
            assert _proper(Rd), it
            w_res = max(w_res, po.sample_residual_px(dev[it], obj, img, K, smp[it]))
        if has[it] != o['has'][it]:
            bad += 1
        elif has[it]:
            d = po.pose_distance(dev[it], o['hyp_pose'][it])
            bad += d > 1e-7
            worst = max(worst, d) if d <= 1e-7 else worst
    print(f'n={n} iters={iters}: {bad} iterations differ, worst agreement {worst:.2e}, worst sample residual {w_res:.2e} px, '
          f'no candidate on {(~has).mean():.2f}')
    assert w_res <= 1e-9
    assert bad <= iters // 100, f'{bad} of {iters} iterations differ from the oracle'
    # counts recomputed in numpy from the device's own candidates: exact
    ref_cnt = po.counts(dev, has, obj, img, K, thr)
    assert np.array_equal(cnt, ref_cnt)
    # the selection: the sequential loop's answer on the device's counts
    info = [int(v) for v in r['info']]
    assert tuple(info[:4]) == po.select(cnt, iters, n, conf) == po.select_sequential(cnt, iters, n, conf)
    found, best, runs, slot = info[:4]
    assert found and best >= 4 and info[4:] == [0, 0, 0, 0]
    R0, t0 = po.expand(dev[slot])
    assert np.array_equal(r['R'], R0) and np.array_equal(r['t'], t0)              # the chosen slot, bit for bit
    mask = r['mask']
    assert mask.sum() == best and np.array_equal(mask, po.inliers(dev[slot], obj, img, K, thr)[0])
    # the refit: from the device's own candidate and mask, against the restatement's
    q = host(ransac_pnp(obj, img, K, thr, conf, iters, seed, refine_iters=10))
    assert list(q['info'][:4]) == info[:4] and np.array_equal(q['mask'], mask) and q['info'][5:].tolist() == [0, 0, 0]
    Rr, tr, kept, margin = po.refit(obj, img, mask, K, R0, t0, 10)
    dR, dt = np.abs(q['R'] - Rr).max(), np.abs(q['t'] - tr).max() / np.linalg.norm(tr)
    print(f'  refit: device - oracle R {dR:.2e}, t {dt:.2e} (bound {po.REFIT_BOUND:.1e}), kept {q["info"][4]} / oracle {kept}, '
          f'margin of the last decision {margin:.1e}')
    assert dR <= po.REFIT_BOUND and dt <= po.REFIT_BOUND and _proper(q['R'])
    assert 0 <= q['info'][4] <= 10
    if margin > 1e-6:                                                             # a clear last decision: the same number of steps
        assert q['info'][4] == kept
    sq = lambda R, t: po.refit_sums(np.asarray(R), np.asarray(t), obj[mask], po.f32(img)[mask], K)[27]   # noqa: E731
    assert sq(q['R'], q['t']) <= sq(R0, t0)
    return ref, r, q


@pytest.mark.parametrize('scene', po.SCENES, ids=lambda s: f'n{s[0]}-it{s[5]}')
def test_every_stage_against_the_oracle_and_the_pose_against_the_scene(scene):
    ref, r, q = check_every_stage(scene)
    n, outl, noise, thr, conf, iters, seed = scene
    # end to end against ground truth: within 1.5 times the restatement's own error on noisy scenes (another, equally good
    # sample may win a near-tie in the count), within 10 times on noise-free ones
    ok, rvec, tvec, inl = solve_pnp_ransac(ref['obj'], ref['img'], ref['K'], None, iters, thr, conf, seed)
    assert ok and rvec.shape == (3, 1) and tvec.shape == (3, 1) and inl.shape == (q['mask'].sum(), 1) and inl.dtype == np.int32
    assert np.array_equal(inl[:, 0], np.flatnonzero(q['mask'])) and np.array_equal(tvec[:, 0], q['t']) and np.array_equal(rvec, rodrigues(q['R']))
    o = ref['ransac']
    o_rot, o_t = po.rotation_error(o['R'], ref['R']), po.translation_error(o['t'], ref['t'])
    d_rot, d_t = po.rotation_error(q['R'], ref['R']), po.translation_error(q['t'], ref['t'])
    factor = 1.5 if noise > 0 else 10.0
    print(f'  rotation error {d_rot:.3e} (oracle {o_rot:.3e}), translation error {d_t:.3e} (oracle {o_t:.3e})')
    assert d_rot <= factor * o_rot and d_t <= factor * o_t


@pytest.mark.parametrize('scene', po.EDGES, ids=lambda s: f'n{s[0]}-it{s[5]}')
def test_wavefront_chunk_and_workgroup_edges(scene):
    check_every_stage(scene)


def _lift_case():
    H, W = 37, 53
    rng = np.random.default_rng(3)
    depth = rng.uniform(2, 9, (H, W)).astype(np.float32)
    depth[5, 7], depth[6, 7], depth[7, 7], depth[8, 7], depth[0, 0] = 0.0, -2.0, np.nan, np.inf, 0.0
    K = np.array([[60.0, 0.4, W / 2.0], [0.0, 61.5, H / 2.0], [0.0, 0.0, 1.0]])
    grid = np.stack(np.meshgrid(np.arange(-1, W + 1, dtype=np.float64), np.arange(-1, H + 1, dtype=np.float64)), -1).reshape(-1, 2)
    pts = np.concatenate([grid, grid + 0.5, grid + [0.5, 0.0], rng.uniform([-2, -2], [W + 1, H + 1], (500, 2)),
                          [[-0.5, 3.0], [-0.5000001, 3.0], [W - 0.5, 3.0], [W - 0.5000001, 3.0], [3.0, H - 0.5], [3.0, H - 0.5000001],
                           [7.0, 5.0], [7.0, 6.0], [7.0, 7.0], [7.0, 8.0], [7.4, 6.6], [np.nan, 3.0], [3.0, np.inf], [1e30, 1.0]]])
    return depth, K, pts


def test_lift_pixels_bit_for_bit():
    depth, K, pts = _lift_case()
    c2w = po.pose_matrix((10.0, -20.0, 30.0), (1.0, -2.0, 0.5))
    for m in (None, c2w):
        want = po.lift(pts, depth, K, m)
        got = lift_pixels(pts, depth, K, m)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (len(pts), 3)
        got = got.cpu().numpy()
        assert np.array_equal(got, want, equal_nan=True)
        assert 0.05 < np.isnan(want[:, 0]).mean() < 0.5
    # device tensors stay where they are; float32 points are widened exactly
    got = lift_pixels(torch.from_numpy(pts.astype(np.float32)).cuda(), torch.from_numpy(depth).cuda(), K)
    assert np.array_equal(got.cpu().numpy(), po.lift(pts.astype(np.float32), depth, K), equal_nan=True)


def _localize_case(outliers):
    (da, Ka, ca), (db, Kb, cb) = po.capture_pair()
    H, W = da.shape
    cap_a, cap_b = Capture(np.zeros((H, W, 3), np.uint8), da, Ka, ca), Capture(np.zeros((H, W, 3), np.uint8), db, Kb, cb)
    rng = np.random.default_rng(5)
    corrs = depth_corrs(cap_a, cap_b, subset=rng.permutation(H * W)[:600].astype(np.int64)).cpu().numpy()
    assert len(corrs) >= 300 and np.array_equal(corrs[:, :2], np.rint(corrs[:, :2]))
    pa, pb = corrs[:, :2].copy(), corrs[:, 2:].copy()
    bad = np.zeros(len(pa), bool)
    if outliers:
        bad = np.arange(len(pa)) % 4 == 0
        pb[bad] = rng.uniform([0, 0], [W, H], (int(bad.sum()), 2))
    return cap_a, Kb, cb, pa, pb, bad


@pytest.mark.parametrize('outliers', [False, True], ids=['exact', 'quarter-noise'])
def test_localize_recovers_the_pose_of_the_second_capture(outliers):
    cap_a, Kb, c2w_true, pa, pb, bad = _localize_case(outliers)
    kw = dict(threshold=1.0, confidence=0.999, max_iters=100, seed=2)
    c2w, mask = localize(pa, pb, cap_a, Kb, **kw)
    assert c2w.shape == (4, 4) and c2w.dtype == np.float64 and mask.shape == (len(pa), 1) and mask.dtype == np.uint8
    assert np.array_equal(c2w[3], [0, 0, 0, 1]) and _proper(c2w[:3, :3])
    # the restatement on the same correspondences: lift, RANSAC, refit
    obj = po.lift(pa, cap_a.depth, cap_a.K, cap_a.c2w)
    o = po.ransac(obj, pb, Kb, kw['threshold'], kw['confidence'], kw['max_iters'], kw['seed'])
    assert o['info'][0]
    w2c = np.linalg.inv(c2w_true)
    err = lambda R, t: (po.rotation_error(R, w2c[:3, :3]), po.translation_error(t, w2c[:3, 3]))   # noqa: E731
    R, t = c2w[:3, :3].T, -c2w[:3, :3].T @ c2w[:3, 3]
    (d_rot, d_t), (o_rot, o_t) = err(R, t), err(o['R'], o['t'])
    print(f'localize: rotation error {d_rot:.3e} (oracle {o_rot:.3e}), translation error {d_t:.3e} (oracle {o_t:.3e}), {mask.sum()} of {len(pa)} inliers')
    assert d_rot <= 10 * o_rot and d_t <= 10 * o_t
    assert not mask[bad].any() and mask[~bad].all()
    # the two calls back to back are the two calls apart
    r = host(localize_tensors(pa, pb, cap_a.depth, cap_a.K, cap_a.c2w, Kb, **kw))
    assert np.array_equal(r['object_points'], obj, equal_nan=True)
    q = host(ransac_pnp(obj, pb, Kb, **kw))
    assert all(np.array_equal(r[k], q[k]) for k in q) and np.array_equal(r['R'].T, c2w[:3, :3])


def test_degenerate_input():
    X, p, K, _, _, _ = po.pnp_scene(300, 0.0, 0, 0.0)
    line = X[0] + np.arange(300)[:, None] * (X[1] - X[0])                        # all object points on one line
    for obj in (line, np.full((300, 3), np.nan)):
        for refine in (0, 10):
            r = host(ransac_pnp(obj, p, K, 8.0, 0.99, 65, 0, refine, hypotheses=True))
            assert list(r['info']) == [0, 0, 65, -1, 0, 0, 0, 0] and (r['R'] == 0).all() and (r['t'] == 0).all() and not r['mask'].any()
            assert (r['hyp_count'] == -1).all() and np.isnan(r['hyp_pose']).all()
        assert solve_pnp_ransac(obj, p, K, iterations_count=65) == (False, None, None, None)
    # n = 4 exact: found with 4 inliers
    X4, p4, K4, R4, t4, _ = po.pnp_scene(4, 0.0, 7, 0.0)
    r = host(ransac_pnp(X4, p4, K4, 2.0, 0.99, 20, 0))
    assert r['info'][0] == 1 and r['info'][1] == 4 and r['mask'].all()
    assert po.rotation_error(r['R'], R4) < 1e-5 and po.translation_error(r['t'], t4) < 1e-5
    # a third of the object points NaN (lifted without depth): never inliers, and the pose is that of the valid points
    Xn = X.copy()
    Xn[::3] = np.nan
    valid = ~np.isnan(Xn[:, 0])
    r = host(ransac_pnp(Xn, p, K, 2.0, 0.99, 100, 1, hypotheses=True))
    assert r['info'][0] and not r['mask'][~valid].any() and r['mask'][valid].all() and r['info'][1] == valid.sum()
    o = po.ransac(Xn, p, K, 2.0, 0.99, 100, 1)
    assert np.array_equal(r['hyp_count'] < 0, ~o['has']) and list(r['info'][:4]) == list(o['info'][:4])
    q = host(ransac_pnp(X[valid], p[valid], K, 2.0, 0.99, 100, 1))
    assert max(np.abs(r['R'] - q['R']).max(), np.abs(r['t'] - q['t']).max()) < 1e-6   # both within float32 pixel rounding of the scene
    _, _, _, R, t, _ = po.pnp_scene(300, 0.0, 0, 0.0)
    assert po.rotation_error(r['R'], R) < 1e-6 and po.translation_error(r['t'], t) < 1e-6


def test_same_bits_across_calls_streams_scratch_and_graph_replay():
    n, thr, conf, iters, seed = 3000, 3.0, 0.99, 300, 5
    obj, img, K, _, _, _ = po.pnp_scene(n, 0.4, seed, 1.0)
    d1, d2 = torch.from_numpy(obj).cuda(), torch.from_numpy(img).cuda()
    first = host(ransac_pnp(d1, d2, K, thr, conf, iters, seed))
    again = host(ransac_pnp(d1, d2, K, thr, conf, iters, seed))
    assert first['info'][0] and first['info'][4] >= 1
    for k in first:
        assert np.array_equal(first[k], again[k]), k
    # the C ABI directly: a side stream, a larger caller scratch full of garbage, no optional outputs
    lib = _lib.load_library()
    nbytes = ctypes.c_size_t()
    assert lib.cotr_ransac_pnp_scratch_bytes(n, iters, ctypes.byref(nbytes)) == 0
    k9 = (ctypes.c_double * 9)(*K.reshape(9))
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def buffers():
        return dict(s=torch.full((nbytes.value + 4096,), 0xA5, dtype=torch.uint8, device='cuda'), R=torch.full((9,), -7.0, dtype=torch.float64, device='cuda'),
                    t=torch.full((3,), -7.0, dtype=torch.float64, device='cuda'), mask=torch.full((n,), 9, dtype=torch.uint8, device='cuda'),
                    info=torch.full((8,), -3, dtype=torch.int32, device='cuda'))

    def enqueue(b, stream):
        rc = lib.cotr_ransac_pnp(p(d1), p(d2), n, k9, thr, conf, iters, seed, 10, p(b['R']), p(b['t']), p(b['mask']), p(b['info']), None, None, None,
                                 p(b['s']), nbytes.value + 4096, stream)
        assert rc == 0, lib.cotr_raster_last_error()

    def same(b):
        assert np.array_equal(b['R'].cpu().numpy(), first['R'].reshape(9)) and np.array_equal(b['t'].cpu().numpy(), first['t'])
        assert np.array_equal(b['mask'].cpu().numpy().astype(bool), first['mask']) and np.array_equal(b['info'].cpu().numpy(), first['info'])
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


def test_cv2_shaped_call():
    scene = po.SCENES[0]
    ref = po.reference(scene)
    n, outl, noise, thr, conf, iters, seed = scene
    obj32, img32 = ref['obj'].astype(np.float32), ref['img'].astype(np.float32)
    ok, rvec, tvec, inl = solve_pnp_ransac(obj32.reshape(-1, 1, 3), img32.reshape(-1, 1, 2), ref['K'], np.zeros(5), iters, thr, conf, seed)
    assert ok is True and rvec.shape == (3, 1) and tvec.shape == (3, 1) and rvec.dtype == tvec.dtype == np.float64
    assert inl.dtype == np.int32 and inl.ndim == 2 and inl.shape[1] == 1 and (np.diff(inl[:, 0]) > 0).all()
    r = host(ransac_pnp(obj32.astype(np.float64), ref['img'], ref['K'], thr, conf, iters, seed))
    assert np.array_equal(rodrigues(r['R']), rvec) and np.array_equal(r['t'], tvec[:, 0]) and np.array_equal(np.flatnonzero(r['mask']), inl[:, 0])
    t = ransac_pnp(torch.from_numpy(ref['obj']).cuda(), torch.from_numpy(ref['img']).cuda(), ref['K'], thr, conf, iters, seed)
    assert all(v.is_cuda for v in t.values()) and t['mask'].dtype == torch.bool and tuple(t['R'].shape) == (3, 3)


def test_zoom_engine_localize():
    from tests.engine_fixtures import CyclicFakeModel, synthetic_pair
    img_a, img_b = synthetic_pair(1)
    H, W = img_a.shape[:2]
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    depth = (4.0 + xs / 64.0 + ys / 128.0).astype(np.float32)
    depth[::7, ::5] = 0.0
    K_a = np.array([[300.0, 0.5, W / 2], [0.0, 310.0, H / 2], [0.0, 0.0, 1.0]])
    K_b = np.array([[280.0, -0.5, img_b.shape[1] / 2], [0.0, 290.0, img_b.shape[0] / 2], [0.0, 0.0, 1.0]])
    cap_a = Capture(img_a, depth, K_a, po.pose_matrix((5.0, -3.0, 2.0), (0.3, 0.1, -0.2)))
    eng = ZoomEngine(CyclicFakeModel().cuda())
    rng = np.random.default_rng(0)
    q = np.stack([rng.uniform(5, W - 5, 40), rng.uniform(5, H - 5, 40)], 1).astype(np.float32)
    kw = dict(threshold=20.0, max_iters=100, seed=3)
    with torch.no_grad():
        want = eng.cotr_corr_multiscale(img_a, img_b, np.linspace(0.5, 0.0625, 4), 1, max_corrs=1000, queries_a=q, force=True)
        c2w, corrs, mask = eng.localize(cap_a, img_b, K_b, queries_a=q, **kw)
    assert np.array_equal(corrs, want) and corrs.shape == (40, 4)
    cw, mw = localize(want[:, :2], want[:, 2:], cap_a, K_b, **kw)
    assert (c2w is None) == (cw is None) == (mask is None)
    if c2w is not None:
        assert np.array_equal(c2w, cw) and np.array_equal(mask, mw)
        assert c2w.shape == (4, 4) and np.isfinite(c2w).all() and mask.shape == (40, 1) and mask.dtype == np.uint8
