"""The relative-pose refit on the MI355X (cotr_refine_pose in cotr_amd/csrc/essential.hip) against the numpy restatement
tests/pose_refit_oracle.py: one accumulation, every round's re-counted mask and fit from the device's own
pose of the round before, the whole call, degenerate input, repeatability, the calls built on it, and the pose against the scene.

Bounds.  The device adds its sums in another order than the restatement.  What the order decides was measured on the CPU with
the restatement forwards against backwards (tests/test_pose_refit_cpu.py holds both figures): 2.5e-15 of a group's largest sum
for one accumulation, 5.1e-9 in an entry of R or t for a whole refit (a marginal step kept one way and not the other).  The
device is allowed 1000 times each, the margin of DESIGN.md 3h-2 and 3h-4 for the same effect: SUMS_BOUND = 2.5e-12,
REFIT_BOUND = 5.1e-6.  Masks are compared exactly, on fixtures whose errors and depths keep a relative margin above 1e-6 from
the thresholds.  Most tests start from ``start``: the scene's pose turned by 0.05 / 0.15 degrees and its Sampson mask, so no
RANSAC runs.

Measured on an MI355X: a round's R, t within 5.0e-9 of the restatement at n = 63 (the steps kept differ) and within 1e-15 to
7.5e-10 elsewhere; the 22 sums within 1.2e-16 to 2.0e-15; every re-counted mask identical; on the quality scenes the device's
errors equal the restatement's to three digits."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import ZoomEngine, refine_pose_tensors, refine_relative_pose, relative_pose
from cotr_amd.inference.essential import pose_of_essential, ransac_essential, relative_pose_tensors
from tests import essential_oracle as eo
from tests import pose_refit_oracle as po

pytestmark = pytest.mark.gpu
ids = lambda s: f'n{s[0]}-seed{s[6]}'   # noqa: E731
ROUNDS, ITERS = (1, 2, 4, 8), (0, 1, 10)
# rotation_error_deg and direction_error_deg go through arccos near 1, whose argument moves in steps of 1.1e-16: they cannot
# tell errors below sqrt(2 * 2.2e-16) rad = 1.2e-6 degrees apart
RESOLUTION_DEG = 2e-6


def host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _proper(R):
    return np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12


def device_refit(s, rounds, iters, **kw):
    a = dict(mask=s['mask0'], threshold=s['thr'], rounds=rounds, refine_iters=iters)
    a.update(kw)
    return host(refine_pose_tensors(s['R0'], s['t0'], s['p1'], s['p2'], s['K1'], s['K2'], **a))


@pytest.mark.parametrize('scene', po.SIZES, ids=ids)
def test_every_round_against_the_restatement(scene):
    s = po.start(scene)
    n = scene[0]
    xn1, xn2 = eo.normalise(s['p1'], s['K1']), eo.normalise(s['p2'], s['K2'])
    sthr = eo.scaled_threshold(s['thr'], s['K1'], s['K2'])
    worst = 0.0
    for iters in ITERS:
        R, t, mask, total = s['R0'], po.unit(s['t0']), s['mask0'], 0
        for rounds in range(1, max(ROUNDS) + 1):                # 1, 2, 4, 8 and between: the call with k rounds ends where round k + 1 starts
            q = device_refit(s, rounds, iters)
            if rounds > 1:                                      # the mask of this round from the device's own pose before it
                mask, margin = po.recount(R, t, xn1, xn2, sthr)
                assert margin > 1e-6, (n, iters, rounds, margin)
            assert np.array_equal(q['mask'], mask), (n, iters, rounds)
            want = po.fit(R, t, xn1[mask], xn2[mask], iters)    # one round of the restatement from the device's inputs
            d = max(np.abs(q['R'] - want['R']).max(), np.abs(q['t'] - want['t']).max())
            worst = max(worst, d)
            assert d <= po.REFIT_BOUND, (n, iters, rounds, d)
            if want['margin'] > 1e-6:
                assert q['info'][4] == want['kept'], (n, iters, rounds, q['info'], want['kept'], want['margin'])
            total += int(q['info'][4])
            assert list(q['info']) == [1, mask.sum(), rounds, total, q['info'][4], want['skipped'], 0, 0]
            assert _proper(q['R']) and abs(np.linalg.norm(q['t']) - 1) < 1e-15
            assert np.array_equal(q['E'].reshape(9), po.unit_signed(po.cross_mat(q['t'], q['R'])))
            if iters == 0:
                assert np.array_equal(q['R'], s['R0']) and np.array_equal(q['t'], po.unit(s['t0']))   # the input bit for bit
            R, t = q['R'], q['t']
    print(f'n={n}: R, t within {worst:.2e} of the restatement')


@pytest.mark.parametrize('scene', po.SIZES, ids=ids)
def test_one_accumulation_against_the_restatement(scene):
    """rounds = 1, refine_iters = 0 is one accumulate / finish pair at the input pose; the caller's scratch then ends with the
    per-chunk sums [chunks][22] (256-byte aligned), which the finish kernel adds in chunk order"""
    s = po.start(scene)
    n = scene[0]
    lib = _lib.load_library()
    nb = ctypes.c_size_t()
    assert lib.cotr_refine_pose_scratch_bytes(n, ctypes.byref(nb)) == 0
    chunks = (n + 2047) // 2048
    parts_at = nb.value - (chunks * 22 * 8 + 255) // 256 * 256
    K9 = ctypes.c_double * 9
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()   # noqa: E731
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    R, t, d1, d2 = dev(s['R0'].reshape(9), torch.float64), dev(s['t0'], torch.float64), dev(s['p1'], torch.float64), dev(s['p2'], torch.float64)
    m = dev(s['mask0'], torch.uint8)
    scratch = torch.full((nb.value,), 0xA5, dtype=torch.uint8, device='cuda')
    out = dict(R=torch.empty(9, dtype=torch.float64, device='cuda'), t=torch.empty(3, dtype=torch.float64, device='cuda'),
               E=torch.empty(9, dtype=torch.float64, device='cuda'), mask=torch.empty(n, dtype=torch.uint8, device='cuda'),
               info=torch.empty(8, dtype=torch.int32, device='cuda'))
    rc = lib.cotr_refine_pose(p(R), p(t), p(d1), p(d2), n, K9(*s['K1'].reshape(9)), K9(*s['K2'].reshape(9)), s['thr'], 50.0, 1, 0, p(m), None,
                              p(out['R']), p(out['t']), p(out['E']), p(out['mask']), p(out['info']), p(scratch), nb.value,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.cotr_raster_last_error()
    torch.cuda.synchronize()
    parts = scratch[parts_at:parts_at + chunks * 22 * 8].cpu().numpy().view(np.float64).reshape(chunks, 22)
    got = np.zeros(22)
    for c in range(chunks):
        got = got + parts[c]
    xn1, xn2 = eo.normalise(s['p1'], s['K1'])[s['mask0']], eo.normalise(s['p2'], s['K2'])[s['mask0']]
    want = po.sums(s['R0'], po.unit(s['t0']), xn1, xn2)
    d = po.sums_distance(got, want)
    print(f'n={n}: the 22 sums within {d:.2e} (relative to the largest of their group)')
    assert d <= po.SUMS_BOUND
    assert out['info'].cpu().numpy()[5] == want[21] == 0


def test_documented_outputs_of_degenerate_input_and_no_fault():
    s = po.start(po.SIZES[3])
    n = 64

    def zero(q):
        return not q['R'].any() and not q['t'].any() and not q['E'].any() and not q['mask'].any() and not q['info'].any()
    assert zero(device_refit(s, 4, 10, found=torch.zeros(1, dtype=torch.int32, device='cuda')))
    assert device_refit(s, 4, 10, found=torch.ones(1, dtype=torch.int32, device='cuda'))['info'][0] == 1
    for R0, t0 in ((s['R0'] * np.nan, s['t0']), (s['R0'], np.zeros(3)), (s['R0'], np.array([np.inf, 0.0, 0.0])), (s['R0'], np.array([0.0, np.nan, 1.0]))):
        assert zero(host(refine_pose_tensors(R0, t0, s['p1'], s['p2'], s['K1'], s['K2'], s['mask0'], s['thr'])))
    # fewer than 5 masked points: round 1 takes no step; the later rounds re-count from the unchanged pose
    few = np.zeros(n, bool)
    few[np.flatnonzero(s['mask0'])[:4]] = True
    q = device_refit(s, 1, 10, mask=few)
    assert list(q['info']) == [1, 4, 1, 0, 0, 0, 0, 0] and np.array_equal(q['R'], s['R0']) and np.array_equal(q['mask'], few)
    q = device_refit(s, 2, 10, mask=few)
    want = po.refine(s['R0'], s['t0'], s['p1'], s['p2'], s['K1'], s['K2'], few, s['thr'], 50.0, 2, 10)
    assert np.array_equal(q['mask'], want['mask']) and max(np.abs(q['R'] - want['R']).max(), np.abs(q['t'] - want['t']).max()) <= po.REFIT_BOUND
    none = device_refit(s, 1, 10, mask=np.zeros(n, bool))
    assert list(none['info']) == [1, 0, 1, 0, 0, 0, 0, 0] and np.array_equal(none['R'], s['R0']) and not none['mask'].any()
    # one point 64 times: the normal equations are singular, no step, the pose stays
    K = np.array([[800.0, 1.5, 320.0], [0.0, 780.0, 240.0], [0.0, 0.0, 1.0]])
    p1, p2 = np.repeat([[300.0, 200.0]], n, 0), np.repeat([[310.0, 205.0]], n, 0)
    q = host(refine_pose_tensors(s['R0'], s['t0'], p1, p2, K, None, None, 1.0, 50.0, 2, 10))
    want = po.refine(s['R0'], s['t0'], p1, p2, K, None, None, 1.0, 50.0, 2, 10)
    assert q['info'][3] == 0 and np.array_equal(q['R'], s['R0']) and np.array_equal(q['mask'], want['mask']) and list(q['info']) == list(want['info'])
    # without a mask every point is fitted; the cv2-shaped call
    R, t, mask = refine_relative_pose(s['R0'], s['t0'], s['p1'], s['p2'], s['K1'], s['K2'], rounds=1, refine_iters=0, threshold=s['thr'])
    assert R.shape == (3, 3) and t.shape == (3, 1) and mask.shape == (n, 1) and mask.dtype == np.uint8 and mask.all()
    assert np.array_equal(R, s['R0']) and np.array_equal(t[:, 0], po.unit(s['t0']))


def test_same_bits_across_calls_streams_scratch_and_graph_replay():
    n, thr, conf, iters, seed = 3000, 1.0, 0.999, 150, 5
    p1, p2, K1, K2, _, _, _ = eo.two_view_scene(n, 0.4, seed, 1.0)
    d1, d2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
    kw = dict(refine_rounds=4, refine_iters=10)
    first = host(relative_pose_tensors(d1, d2, K1, K2, thr, conf, iters, seed, **kw))
    again = host(relative_pose_tensors(d1, d2, K1, K2, thr, conf, iters, seed, **kw))
    assert first['info'][0] and first['refine_info'][0] == 1 and first['refine_info'][3] > 0
    for k in first:
        assert np.array_equal(first[k], again[k]), k
    # refine_rounds = 0 is the call as it was: the same bits as without the argument and as the two calls made one by one
    plain = host(relative_pose_tensors(d1, d2, K1, K2, thr, conf, iters, seed))
    zero = host(relative_pose_tensors(d1, d2, K1, K2, thr, conf, iters, seed, refine_rounds=0, refine_iters=3))
    assert sorted(plain) == sorted(zero) == ['E', 'R', 'info', 'mask', 'pose_info', 't']
    r = ransac_essential(d1, d2, K1, K2, thr, conf, iters, seed)
    q = host(pose_of_essential(r['E'], d1, d2, K1, K2, r['mask']))
    for k in plain:
        assert np.array_equal(plain[k], zero[k]), k
    assert np.array_equal(plain['R'], q['R']) and np.array_equal(plain['t'], q['t']) and np.array_equal(plain['mask'], q['mask'])
    for k in ('E', 'R', 't', 'mask'):
        assert np.array_equal(first[k + '_ransac'], plain[k]), k
    a, b = relative_pose(p1, p2, K1, K2, threshold=thr, confidence=conf, max_iters=iters, seed=seed), \
        relative_pose(p1, p2, K1, K2, threshold=thr, confidence=conf, max_iters=iters, seed=seed, refine_rounds=0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[0], plain['R'])
    c = relative_pose(p1, p2, K1, K2, threshold=thr, confidence=conf, max_iters=iters, seed=seed, **kw)
    assert np.array_equal(c[0], first['R']) and np.array_equal(c[1][:, 0], first['t']) and np.array_equal(c[2][:, 0].astype(bool), first['mask'])
    # the refit as a call of its own from the unrefined pose: the same bits
    own = host(refine_pose_tensors(plain['R'], plain['t'], d1, d2, K1, K2, plain['mask'], thr, 50.0, 4, 10))
    for k in ('R', 't', 'E', 'mask'):
        assert np.array_equal(own[k], first[k]), k
    assert np.array_equal(own['info'], first['refine_info'])
    # the C ABI directly: a side stream, a larger caller scratch full of garbage
    lib = _lib.load_library()
    nb = ctypes.c_size_t()
    assert lib.cotr_refine_pose_scratch_bytes(n, ctypes.byref(nb)) == 0
    K9 = ctypes.c_double * 9
    k1, k2 = K9(*K1.reshape(9)), K9(*K2.reshape(9))
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    Rin, tin = torch.from_numpy(plain['R'].reshape(9)).cuda(), torch.from_numpy(plain['t']).cuda()
    min_ = torch.from_numpy(plain['mask'].astype(np.uint8)).cuda()
    g = lambda size, dt: torch.full((size,), 0xA5 if dt == torch.uint8 else -7, dtype=dt, device='cuda')   # noqa: E731
    b = dict(s=g(nb.value + 4096, torch.uint8), R=g(9, torch.float64), t=g(3, torch.float64), E=g(9, torch.float64), mask=g(n, torch.uint8),
             info=g(8, torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rc = lib.cotr_refine_pose(p(Rin), p(tin), p(d1), p(d2), n, k1, k2, thr, 50.0, 4, 10, p(min_), None, p(b['R']), p(b['t']), p(b['E']), p(b['mask']),
                              p(b['info']), p(b['s']), nb.value + 4096, ctypes.c_void_p(side.cuda_stream))
    assert rc == 0, lib.cotr_raster_last_error()
    side.synchronize()
    for mine, theirs in (('R', 'R'), ('t', 't'), ('E', 'E'), ('info', 'refine_info')):
        assert np.array_equal(b[mine].cpu().numpy().reshape(first[theirs].shape), first[theirs]), mine
    assert np.array_equal(b['mask'].cpu().numpy().astype(bool), first['mask'])
    # the whole sequence captured once (a single linear chain on the capture stream), replayed once
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = relative_pose_tensors(d1, d2, K1, K2, thr, conf, iters, seed, **kw)
    graph.replay()
    replayed = host(captured)
    for k in first:
        assert np.array_equal(first[k], replayed[k]), k


def test_zoom_engine_relative_pose_with_the_refit():
    from tests.engine_fixtures import CyclicFakeModel, synthetic_pair
    img_a, img_b = synthetic_pair(1)
    eng = ZoomEngine(CyclicFakeModel().cuda())
    rng = np.random.default_rng(0)
    q = np.stack([rng.uniform(5, img_a.shape[1] - 5, 40), rng.uniform(5, img_a.shape[0] - 5, 40)], 1).astype(np.float32)
    K_a = np.array([[300.0, 0.5, img_a.shape[1] / 2], [0.0, 310.0, img_a.shape[0] / 2], [0.0, 0.0, 1.0]])
    K_b = np.array([[280.0, -0.5, img_b.shape[1] / 2], [0.0, 290.0, img_b.shape[0] / 2], [0.0, 0.0, 1.0]])
    kw = dict(threshold=20.0, max_iters=100, seed=3, refine_rounds=4, refine_iters=10)
    with torch.no_grad():
        R, t, corrs, mask = eng.relative_pose(img_a, img_b, K_a, K_b, queries_a=q, **kw)
    Rw, tw, mw = relative_pose(corrs[:, :2], corrs[:, 2:], K_a, K_b, **kw)
    assert corrs.shape == (40, 4) and (R is None) == (Rw is None)
    if R is not None:
        assert np.array_equal(R, Rw) and np.array_equal(t, tw) and np.array_equal(mask, mw)
        assert _proper(R) and abs(np.linalg.norm(t) - 1) < 1e-12 and mask.shape == (40, 1) and mask.dtype == np.uint8


@pytest.mark.parametrize('scene', po.QUALITY, ids=lambda s: f'n{s[0]}-it{s[5]}')
def test_pose_against_the_scene_after_four_rounds(scene):
    """The scenes of po.QUALITY: there the restatement alone, from its own RANSAC pose, ends below the unrefined errors
    (tests/test_pose_refit_cpu.py checks it; no scene has noise at n < 1000).  The device's whole sequence, RANSAC, pose and 4
    rounds of 10: both its errors within 1.5 times the restatement's on noisy scenes and within 10 times on noise-free ones, the
    margins of DESIGN.md 3h-3, each no finer than the measure resolves."""
    n, outl, noise, thr, conf, iters, seed = scene
    ref = eo.reference(scene)
    pose = ref['pose']
    want = po.refine(pose['R'], pose['t'], ref['p1'], ref['p2'], ref['K1'], ref['K2'], pose['mask'], thr, 50.0, 4, 10)
    before = eo.rotation_error_deg(pose['R'], ref['R']), eo.direction_error_deg(pose['t'], ref['t'])
    o_rot, o_dir = eo.rotation_error_deg(want['R'], ref['R']), eo.direction_error_deg(want['t'], ref['t'])
    assert o_rot < before[0] and o_dir < before[1]
    q = host(relative_pose_tensors(ref['p1'], ref['p2'], ref['K1'], ref['K2'], thr, conf, iters, seed, refine_rounds=4, refine_iters=10))
    assert q['info'][0] and q['refine_info'][0] == 1 and q['refine_info'][2] == 4 and _proper(q['R'])
    u_rot, u_dir = eo.rotation_error_deg(q['R_ransac'], ref['R']), eo.direction_error_deg(q['t_ransac'], ref['t'])
    d_rot, d_dir = eo.rotation_error_deg(q['R'], ref['R']), eo.direction_error_deg(q['t'], ref['t'])
    factor = 1.5 if noise > 0 else 10.0
    print(f'n={n}: unrefined {u_rot:.3g} / {u_dir:.3g} deg (oracle {before[0]:.3g} / {before[1]:.3g}), 4 rounds {d_rot:.3g} / {d_dir:.3g} deg '
          f'(oracle {o_rot:.3g} / {o_dir:.3g}), steps kept {q["refine_info"][3]}')
    assert d_rot <= factor * max(o_rot, RESOLUTION_DEG) and d_dir <= factor * max(o_dir, RESOLUTION_DEG)
