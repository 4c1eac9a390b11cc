"""The essential-matrix estimator and recover_pose on the MI355X (cotr_amd/csrc/essential.hip) against the numpy restatement
tests/essential_oracle.py: every stage of the RANSAC (samples, candidates, counts, selection, mask) against the same rule,
the pose of the device's own E and mask against the restatement's, the pose against the scene's, degenerate input,
repeatability, and the engine call built on it.

The candidate bound: the restatement reaches the candidates by another numerical route (SVD null space, LAPACK solve and
eigenvectors) than the device (full-pivot null space, Gauss-Jordan, Hessenberg + QR); two accurate routes agree to 1e-12
after the three polish steps, and 1e-7 (the bound of DESIGN.md 3h) is allowed, on at most 1 % of the iterations not at all.
Measured on an MI355X over the fifteen scenes: no iteration differs, the candidates agree within 1.9e-15 to 1.0e-11, the
device's candidates have residuals of at most 4.3e-16 and 3.9e-12, and R and t of recover_pose equal the restatement's bit for
bit."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import ZoomEngine, find_essential_mat, ransac_essential, recover_pose, relative_pose
from cotr_amd.inference.essential import pose_of_essential, relative_pose_tensors
from tests import essential_oracle as eo

pytestmark = pytest.mark.gpu


def host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize('n,iters,seed', [(5, 33, 0), (6, 64, 2), (100, 500, 1), (2049, 63, (1 << 63) + 5)])
def test_samples_are_the_oracles(n, iters, seed):
    rng = np.random.default_rng(n)
    p1, p2 = rng.uniform(0, 640, (n, 2)), rng.uniform(0, 480, (n, 2))
    r = host(ransac_essential(p1, p2, np.diag([500.0, 500.0, 1.0]), None, 1.0, 0.999, iters, seed, hypotheses=True))
    assert np.array_equal(r['samples'], eo.samples(n, iters, seed))


def check_every_stage(scene):
    n, outl, noise, thr, conf, iters, seed = scene
    ref = eo.reference(scene)
    p1, p2, K1, K2, o = ref['p1'], ref['p2'], ref['K1'], ref['K2'], ref['ransac']
    r = host(ransac_essential(p1, p2, K1, K2, thr, conf, iters, seed, hypotheses=True))
    smp = o['samples']
    assert np.array_equal(r['samples'], smp)
    xn1, xn2, sthr = eo.normalise(p1, K1), eo.normalise(p2, K2), eo.scaled_threshold(thr, K1, K2)
    # candidates: as many per iteration (0: no model), the used slots first, and the same set within 1e-7
    dev_E, cnt = r['hyp_E'], r['hyp_count']
    used = cnt >= 0
    nc = used.reshape(iters, 10).sum(axis=1)
    assert np.array_equal(used, eo.slots_used(nc))
    assert np.isnan(dev_E[~used]).all() and np.isfinite(dev_E[used]).all()
    bad, worst, w_epi, w_trace = 0, 0.0, 0.0, 0.0
    for it in range(iters):
        a = [dev_E[10 * it + k] for k in range(nc[it])]
        b = [o['hyp_E'][10 * it + k] for k in range(o['ncand'][it])]
        d = eo.set_distance(a, b)
        bad += d > 1e-7
        worst = max(worst, d) if d <= 1e-7 else worst
        for E in a:   # every device candidate, whatever it is matched to: unit norm, signed, and its equations hold
            epi, trace = eo.residuals(E, xn1[smp[it]], xn2[smp[it]])
            w_epi, w_trace = max(w_epi, epi), max(w_trace, trace)
            assert abs(np.linalg.norm(E) - 1) < 1e-14 and E[np.argmax(np.abs(E))] > 0
    print(f'n={n} iters={iters}: {bad} iterations differ, worst agreement {worst:.2e}, {nc.mean():.2f} candidates per sample, '
          f'residuals {w_epi:.1e} / {w_trace:.1e}')
    assert bad <= iters // 100, f'{bad} of {iters} iterations differ from the oracle'
    assert w_epi <= 1e-12 and w_trace <= 1e-10
    # counts recomputed in numpy from the device's own candidates: exact
    ref_cnt = eo.counts(dev_E, used, xn1, xn2, sthr)
    assert np.array_equal(cnt, ref_cnt)
    # the selection: the sequential loop's answer on the device's counts
    info = [int(v) for v in r['info']]
    assert tuple(info[:4]) == eo.select(cnt, iters, n, conf) == eo.select_sequential(cnt, iters, n, conf)
    found, best, runs, slot = info[:4]
    assert found and best >= 5 and info[4:] == [0, 0, 0, 0]
    E, mask = r['E'].reshape(9), r['mask']
    assert np.array_equal(E, dev_E[slot])                                         # the chosen slot, bit for bit
    assert mask.sum() == best and np.array_equal(mask, eo.inliers(E, xn1, xn2, sthr)[0])
    # the pose of the device's E on the device's mask against the restatement's
    q = host(pose_of_essential(E.reshape(3, 3), p1, p2, K1, K2, mask))
    want = eo.recover_pose(E, p1, p2, K1, K2, mask)
    assert want['margin'] > 1e-9                                                  # no point has to be excluded
    print(f'  pose: info {list(q["info"][:6])}, R {np.abs(q["R"] - want["R"]).max():.1e}, t {np.abs(q["t"] - want["t"]).max():.1e}')
    assert np.array_equal(q['info'], want['info'])
    assert np.abs(q['R'] - want['R']).max() <= 1e-9 and np.abs(q['t'] - want['t']).max() <= 1e-9
    assert np.array_equal(q['mask'], want['mask']) and q['mask'].sum() == q['info'][0]
    return ref, r, q


@pytest.mark.parametrize('scene', eo.SCENES, ids=lambda s: f'n{s[0]}-it{s[5]}')
def test_every_stage_against_the_oracle_and_the_pose_against_the_scene(scene):
    ref, r, q = check_every_stage(scene)
    noise = scene[2]
    # end to end against ground truth: within 1.5 times the restatement's own error on noisy scenes (another, equally good
    # sample may win a near-tie in the count), within 10 times on noise-free ones
    R, t, mask = relative_pose(ref['p1'], ref['p2'], ref['K1'], ref['K2'], threshold=scene[3], confidence=scene[4], max_iters=scene[5],
                               seed=scene[6])
    assert R.shape == (3, 3) and t.shape == (3, 1) and mask.shape == (scene[0], 1) and mask.dtype == np.uint8
    assert np.array_equal(R, q['R']) and np.array_equal(t[:, 0], q['t']) and np.array_equal(mask[:, 0].astype(bool), q['mask'])
    o_rot, o_dir = eo.rotation_error_deg(ref['pose']['R'], ref['R']), eo.direction_error_deg(ref['pose']['t'], ref['t'])
    d_rot, d_dir = eo.rotation_error_deg(R, ref['R']), eo.direction_error_deg(t, ref['t'])
    factor = 1.5 if noise > 0 else 10.0
    print(f'  rotation error {d_rot:.3e} deg (oracle {o_rot:.3e}), translation direction {d_dir:.3e} deg (oracle {o_dir:.3e})')
    assert d_rot <= factor * o_rot and d_dir <= factor * o_dir


@pytest.mark.parametrize('scene', eo.EDGES, ids=lambda s: f'n{s[0]}-it{s[5]}')
def test_wavefront_chunk_and_workgroup_edges(scene):
    check_every_stage(scene)


def test_cv2_shaped_calls():
    scene = eo.SCENES[1]
    ref = eo.reference(scene)
    p1, p2, K1, K2 = ref['p1'].astype(np.float32), ref['p2'].astype(np.float32), ref['K1'], ref['K2']
    E, mask = find_essential_mat(p1, p2, K1, K2, scene[4], scene[3], scene[5], scene[6])
    assert E.shape == (3, 3) and E.dtype == np.float64 and mask.shape == (scene[0], 1) and mask.dtype == np.uint8
    r = host(ransac_essential(ref['p1'], ref['p2'], K1, K2, scene[3], scene[4], scene[5], scene[6]))
    assert np.array_equal(E, r['E']) and np.array_equal(mask[:, 0].astype(bool), r['mask'])
    n_good, R, t, pmask = recover_pose(E, p1, p2, K1, K2, mask=mask)
    want = eo.recover_pose(E.reshape(9), ref['p1'], ref['p2'], K1, K2, mask)
    assert n_good == want['info'][0] == pmask.sum() and R.shape == (3, 3) and t.shape == (3, 1) and pmask.shape == (scene[0], 1)
    assert abs(np.linalg.norm(t) - 1) < 1e-12 and np.array_equal(pmask[:, 0].astype(bool), want['mask'])
    # without a mask every point is judged; device tensors stay on the device
    q = pose_of_essential(torch.from_numpy(E).cuda(), torch.from_numpy(ref['p1']).cuda(), torch.from_numpy(ref['p2']).cuda(), K1, K2)
    assert all(v.is_cuda for v in q.values())
    assert np.array_equal(host(q)['info'], eo.recover_pose(E.reshape(9), ref['p1'], ref['p2'], K1, K2)['info'])
    # the same camera for both views when the second is not given
    a, b = host(ransac_essential(ref['p1'], ref['p2'], K1, None, 1.0, 0.999, 50, 1)), host(ransac_essential(ref['p1'], ref['p2'], K1, K1, 1.0, 0.999, 50, 1))
    assert all(np.array_equal(a[k], b[k]) for k in a)


def _proper(R):
    return np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12


def test_degenerate_input():
    K = np.array([[800.0, 1.5, 320.0], [0.0, 780.0, 240.0], [0.0, 0.0, 1.0]])
    # all points identical: every sample is degenerate, nothing is found
    p1, p2 = np.repeat([[300.0, 200.0]], 300, 0), np.repeat([[310.0, 205.0]], 300, 0)
    r = host(ransac_essential(p1, p2, K, None, 1.0, 0.999, 65, 0, hypotheses=True))
    assert list(r['info']) == [0, 0, 65, -1, 0, 0, 0, 0] and (r['E'] == 0).all() and not r['mask'].any()
    assert (r['hyp_count'] == -1).all() and np.isnan(r['hyp_E']).all()
    assert find_essential_mat(p1, p2, K, max_iters=65) == (None, None)
    assert relative_pose(p1, p2, K, max_iters=65) == (None, None, None)
    t = host(relative_pose_tensors(p1, p2, K, max_iters=65))
    assert list(t['pose_info']) == [0, -1, 0, 0, 0, 0, 0, 0] and (t['R'] == 0).all() and (t['t'] == 0).all() and not t['mask'].any()
    z = host(pose_of_essential(np.zeros((3, 3)), p1, p2, K))                      # E = 0 cannot be decomposed
    assert list(z['info']) == [0, -1, 0, 0, 0, 0, 0, 0] and (z['R'] == 0).all() and not z['mask'].any()
    # a pure rotation (t = 0) with half a pixel of noise: some model, and its pose has a proper rotation close to the scene's.
    # The same without noise: the ten constraints vanish on a plane of the null space, the 10 x 10 block has rank ratios of
    # 1e-15 and the rank rule leaves every sample without a model, in the restatement too; nothing may fault.
    q1, _, K1, K2, R, _, _ = eo.two_view_scene(300, 0.0, 5, 0.0)
    h = np.c_[eo.normalise(q1, K1), np.ones(300)] @ R.T @ K2.T
    exact = h[:, :2] / h[:, 2:]
    noisy = eo.f32(exact + np.random.default_rng(1).normal(0, 0.5, (300, 2)))
    E, mask = find_essential_mat(q1, noisy, K1, K2, max_iters=100)
    assert E is not None and mask.sum() >= 5
    n_good, Rd, td, _ = recover_pose(E, q1, noisy, K1, K2, mask=mask)
    assert _proper(Rd) and abs(np.linalg.norm(td) - 1) < 1e-12 and eo.rotation_error_deg(Rd, R) < 1.0
    E, mask = find_essential_mat(q1, eo.f32(exact), K1, K2, max_iters=100)
    if E is not None:
        assert _proper(recover_pose(E, q1, eo.f32(exact), K1, K2, mask=mask)[1])


def test_same_bits_across_calls_streams_scratch_and_graph_replay():
    n, thr, conf, iters, seed = 3000, 1.0, 0.999, 150, 5
    p1, p2, K1, K2, _, _, _ = eo.two_view_scene(n, 0.4, seed, 1.0)
    d1, d2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
    first = host(relative_pose_tensors(d1, d2, K1, K2, thr, conf, iters, seed))
    again = host(relative_pose_tensors(d1, d2, K1, K2, thr, conf, iters, seed))
    assert first['info'][0] and first['pose_info'][0] > 0
    for k in first:
        assert np.array_equal(first[k], again[k]), k
    # the C ABI directly: a side stream, larger caller scratches full of garbage, no optional outputs
    lib = _lib.load_library()
    nb, nbp = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.cotr_ransac_essential_scratch_bytes(n, iters, ctypes.byref(nb)) == 0 and lib.cotr_recover_pose_scratch_bytes(n, ctypes.byref(nbp)) == 0
    K9 = ctypes.c_double * 9
    k1, k2 = K9(*K1.reshape(9)), K9(*K2.reshape(9))
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def buffers():
        g = lambda size, dt: torch.full((size,), 0xA5 if dt == torch.uint8 else -7, dtype=dt, device='cuda')   # noqa: E731
        return dict(s1=g(nb.value + 4096, torch.uint8), s2=g(nbp.value + 4096, torch.uint8), E=g(9, torch.float64), mask=g(n, torch.uint8),
                    info=g(8, torch.int32), R=g(9, torch.float64), t=g(3, torch.float64), mask2=g(n, torch.uint8), info2=g(8, torch.int32))

    def enqueue(b, stream):
        rc = lib.cotr_ransac_essential(p(d1), p(d2), n, k1, k2, thr, conf, iters, seed, p(b['E']), p(b['mask']), p(b['info']), None, None, None,
                                       p(b['s1']), nb.value + 4096, stream)
        assert rc == 0, lib.cotr_raster_last_error()
        rc = lib.cotr_recover_pose(p(b['E']), p(d1), p(d2), n, k1, k2, 50.0, p(b['mask']), p(b['info']), p(b['R']), p(b['t']), p(b['mask2']),
                                   p(b['info2']), p(b['s2']), nbp.value + 4096, stream)
        assert rc == 0, lib.cotr_raster_last_error()

    def same(b):
        for mine, theirs in (('E', 'E'), ('R', 'R'), ('t', 't'), ('info', 'info'), ('info2', 'pose_info')):
            assert np.array_equal(b[mine].cpu().numpy().reshape(first[theirs].shape), first[theirs]), mine
        assert np.array_equal(b['mask2'].cpu().numpy().astype(bool), first['mask'])
    b = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    enqueue(b, ctypes.c_void_p(side.cuda_stream))
    side.synchronize()
    same(b)
    # both calls captured once (a single linear chain on the capture stream), replayed once
    b = buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue(b, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    graph.replay()
    torch.cuda.synchronize()
    same(b)


def test_zoom_engine_relative_pose():
    from tests.engine_fixtures import CyclicFakeModel, synthetic_pair
    img_a, img_b = synthetic_pair(1)
    eng = ZoomEngine(CyclicFakeModel().cuda())
    rng = np.random.default_rng(0)
    q = np.stack([rng.uniform(5, img_a.shape[1] - 5, 40), rng.uniform(5, img_a.shape[0] - 5, 40)], 1).astype(np.float32)
    K_a = np.array([[300.0, 0.5, img_a.shape[1] / 2], [0.0, 310.0, img_a.shape[0] / 2], [0.0, 0.0, 1.0]])
    K_b = np.array([[280.0, -0.5, img_b.shape[1] / 2], [0.0, 290.0, img_b.shape[0] / 2], [0.0, 0.0, 1.0]])
    kw = dict(threshold=20.0, max_iters=100, seed=3)
    with torch.no_grad():
        want = eng.cotr_corr_multiscale(img_a, img_b, np.linspace(0.5, 0.0625, 4), 1, max_corrs=1000, queries_a=q, force=True)
        R, t, corrs, mask = eng.relative_pose(img_a, img_b, K_a, K_b, queries_a=q, **kw)
    assert np.array_equal(corrs, want) and corrs.shape == (40, 4)
    Rw, tw, mw = relative_pose(want[:, :2], want[:, 2:], K_a, K_b, **kw)
    assert (R is None) == (Rw is None)
    if R is not None:
        assert np.array_equal(R, Rw) and np.array_equal(t, tw) and np.array_equal(mask, mw)
        assert _proper(R) and mask.shape == (40, 1) and mask.dtype == np.uint8
