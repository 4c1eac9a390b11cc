"""Bundle adjustment on the MI355X (cotr_bundle_adjust in cotr_amd/csrc/bundle.hip) against the numpy restatement
tests/bundle_oracle.py: one iteration at every shape edge, damping and observation set, the largest reduced system, full runs,
the quality of the poses, degenerate input, repeatability, and the chains built on it.

The device sums the same terms as the restatement but per thread, wavefront and chunk, a third order, so poses, X and the costs
are held to 1000 times the order noise the CPU tests measured between two orders (bundle_oracle.STEP_BOUND after one iteration,
RUN_BOUND after a run), not to bit equality; the integers (info, used, the frozen views, the landmarks) are compared exactly, and
a keep/reject decision only where the restatement's costs differ by more than 1e-6 relatively."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import ZoomEngine, bundle_adjust, bundle_adjust_tensors
from cotr_amd.inference.structure import reconstruct_tensors, triangulate_points_tensors
from tests import bundle_oracle as bo
from tests import structure_oracle as so

pytestmark = pytest.mark.gpu
ROWS = {(3, 64): (0.0, 0.0), (5, 257): (0.7, 0.0), (8, 1025): (0.7, 0.25), (32, 65): (0.7, 0.25)}


def host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items() if torch.is_tensor(v)}


@functools.lru_cache(maxsize=None)
def fixture(V, N):
    return bo.fixture(V, N, *ROWS[(V, N)])


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    if not ok.any():
        return 0.0
    assert np.array_equal(np.isinf(a[ok]), np.isinf(b[ok]))
    ok &= np.isfinite(b)
    return float(np.abs(a[ok] - b[ok]).max() / max(np.abs(b[ok]).max(), 1e-300)) if ok.any() else 0.0


def both(fx, vis='used', **kw):
    a = dict(visible=fx['used'] if isinstance(vis, str) else vis, fixed_views=fx['fixed'])
    a.update(kw)
    trace = []
    want = bo.bundle_adjust(fx['points'], fx['cams'], fx['poses0'], fx['X0'], trace=trace, **a)
    got = bundle_adjust(fx['points'], fx['cams'], fx['poses0'], fx['X0'], **a)
    return got, want, trace


def clear(trace):
    """every decision of the restatement clears the margin"""
    return all(t['solved'] and t['front'] and abs(t['cand'] - t['cost']) > bo.DECISION_MARGIN * t['cost'] for t in trace)


def compare(got, want, trace, bound, what):
    """the integers exactly; poses, X, the start cost and the end cost, each relative to itself, within the bound whatever the
    decisions were (the run noise was measured with the decisions at the floor in it); the counters of the steps and lambda where
    every decision of the restatement clears the margin"""
    V = got['poses'].shape[0]
    d = dict(poses=rel(got['poses'].reshape(V, 12), want['poses']), X=rel(got['X'], want['X']), start=rel(got['stats'][0], want['stats'][0]),
             cost=rel(got['stats'][1], want['stats'][1]))
    print(f'{what}: info {list(got["info"])}, relative differences {d}, bound {bound:.1e}')
    assert np.array_equal(got['used'], want['used']), what
    assert np.array_equal(got['info'][:5], want['info'][:5]) and got['info'][7] == want['info'][7], (what, got['info'], want['info'])
    if clear(trace):
        assert np.array_equal(got['info'], want['info']) and got['stats'][2] == want['stats'][2], (what, got['info'], want['info'])
    assert max(d.values()) <= bound, (what, d)
    return d


# ---- one iteration --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 4, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097])
@pytest.mark.parametrize('V', [2, 3, 5])
def test_one_iteration(V, N):
    fx = bo.step_fixture(V, N)
    for lam in (1e-3, 1e3):
        for name, vis in fx['visibles']:
            got, want, trace = both(fx, vis, iters=1, lambda0=lam)
            assert clear(trace), (V, N, lam, name)               # (chosen on the CPU: every fixture's decision clears the margin)
            compare(got, want, trace, bo.STEP_BOUND, f'V={V} N={N} lambda0={lam} visible={name}')
            assert got['info'][5] + got['info'][6] == len(trace)


# ---- the largest system ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [65, 257])
def test_all_31_views_free(N):
    fx = bo.big_fixture(N)
    got, want, trace = both(fx, iters=1)
    assert want['info'][2] == 31 and want['info'][3] == 0 and clear(trace) and trace[0]['kept']
    compare(got, want, trace, bo.STEP_BOUND, f'V=32 N={N}, 186 unknowns')
    assert (got['poses'][1:].reshape(31, 12) != fx['poses0'][1:]).any(axis=1).all()
    assert np.array_equal(got['poses'][0].reshape(12).view(np.uint64), fx['poses0'][0].view(np.uint64))


def test_three_starved_views_of_32():
    fx = fixture(32, 65)
    got, want, trace = both(fx, iters=1)
    assert list(np.flatnonzero(want['frozen'])) == [6, 19, 23] and clear(trace)
    compare(got, want, trace, bo.STEP_BOUND, 'V=32 N=65, views 6, 19 and 23 frozen')
    assert list(got['info'][1:5]) == [1052, 27, 3, 0]
    for v in (0, 1, 6, 19, 23):
        assert np.array_equal(got['poses'][v].reshape(12).view(np.uint64), fx['poses0'][v].view(np.uint64)), v
    got, want, trace = both(fx, iters=15)
    compare(got, want, trace, bo.RUN_BOUND, 'V=32 N=65, 15 iterations')


# ---- full runs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(3, 64), (5, 257), (8, 1025)])
@pytest.mark.parametrize('rounds', [1, 2, 4])
def test_full_runs(shape, rounds):
    fx = fixture(*shape)
    got, want, trace = both(fx, iters=15, rounds=rounds)
    assert want['margin'] > bo.DECISION_MARGIN                  # (chosen on the CPU: no observation sits on a threshold)
    # poses, X and both costs (the end cost relative to itself, the 1.27e-8 of the noise-free row included) within the bound
    # whatever the decisions at the floor were
    compare(got, want, trace, bo.RUN_BOUND, f'{shape} rounds={rounds}')
    assert got['info'][5] + got['info'][6] <= 15 * rounds and got['info'][5] > 0


# ---- quality --------------------------------------------------------------------------------------------------------------
def test_pose_quality():
    for shape, factor in (((5, 257), 1.5), ((8, 1025), 1.5), ((3, 64), 10.0)):
        fx = fixture(*shape)
        got, want, _ = both(fx, iters=15)
        truth = fx['sc']['poses']
        e0, eo, eg = bo.pose_errors(fx['poses0'], truth), bo.pose_errors(want['poses'], truth), bo.pose_errors(got['poses'].reshape(-1, 12), truth)
        print(f'{shape}: rotation {e0[0]:.3g} -> device {eg[0]:.3g}, restatement {eo[0]:.3g} deg; centre {e0[1]:.3g} -> {eg[1]:.3g}, {eo[1]:.3g}')
        assert eo[0] < 0.1 * e0[0]
        assert eg[0] <= max(factor * eo[0], 2e-6) and eg[1] <= factor * eo[1]


# ---- degenerate input -----------------------------------------------------------------------------------------------------
def test_degenerate_input():
    fx = fixture(5, 257)
    V, N = 5, 257
    args = (fx['points'], fx['cams'], fx['poses0'], fx['X0'])
    kw = dict(visible=fx['used'], fixed_views=fx['fixed'], iters=3)
    r = bundle_adjust(*args, found=torch.zeros(8, dtype=torch.int32, device='cuda'), **kw)
    assert all(not r[k].any() for k in ('poses', 'X', 'used', 'stats', 'info'))
    on = bundle_adjust(*args, found=torch.ones(8, dtype=torch.int32, device='cuda'), **kw)
    plain = bundle_adjust(*args, **kw)
    assert all(np.array_equal(on[k], plain[k]) for k in on)
    # iters = 0: the input bits, the set and the cost of the input state
    r = bundle_adjust(*args, **dict(kw, iters=0))
    want = bo.bundle_adjust(*args, **dict(kw, iters=0))
    assert np.array_equal(r['poses'].reshape(V, 12).view(np.uint64), fx['poses0'].view(np.uint64)) and np.array_equal(r['X'].view(np.uint64), fx['X0'].view(np.uint64))
    assert np.array_equal(r['info'], want['info']) and np.array_equal(r['used'], want['used']) and r['stats'][0] == r['stats'][1]
    assert rel(r['stats'][:1], want['stats'][:1]) <= 1000 * bo.ORDER_NOISE_SUMS and r['stats'][2] == 1e-3
    # NaN and infinite points and X, a NaN and an infinite pose entry, a point behind a camera: defined by the rules, compared as
    # any other input
    pts, X0, poses = fx['points'].copy(), fx['X0'].copy(), fx['poses0'].copy()
    pts[2, 3, 0], pts[2, 4, 1], pts[0, 5] = np.nan, np.inf, -np.inf
    X0[7, 1], X0[8, 2], X0[9] = np.nan, np.inf, np.nan
    X0[10] = -fx['X0'][10]                                        # behind every camera: no observation of it is in the set
    poses[4, 5] = np.nan                                          # views 4 (a NaN in R) and 3 (an infinite t) are not valid:
    poses[3, 7] = np.inf                                          # frozen, their bits kept
    a = dict(kw, visible=None)
    got = bundle_adjust(pts, fx['cams'], poses, X0, **a)
    trace = []
    want = bo.bundle_adjust(pts, fx['cams'], poses, X0, trace=trace, **a)
    assert list(np.flatnonzero(want['frozen'])) == [3, 4] and want['info'][2] == 1 and want['info'][3] == 2 and want['info'][5] > 0
    assert want['info'][4] >= 4 and not want['used'][:, [7, 8, 9, 10]].any() and not want['used'][[3, 4]].any()
    compare(got, want, trace, bo.RUN_BOUND, 'NaN and infinite input')
    assert np.array_equal(got['X'][[7, 8, 9, 10]].view(np.uint64), X0[[7, 8, 9, 10]].view(np.uint64))
    for v in (3, 4):
        assert np.array_equal(got['poses'][v].reshape(12).view(np.uint64), poses[v].view(np.uint64)), v
    # one point 64 times: every view's block has rank 2.  At lambda0 = 1e3 the damped system is well conditioned and one iteration
    # is compared with the restatement like any other input (its order noise is in the CPU measurement)
    rep = bo.repeated_fixture()
    got, want, trace = both(rep, None, iters=1, lambda0=1e3)
    assert clear(trace) and list(want['info'][1:5]) == [320, 3, 0, 0]
    compare(got, want, trace, bo.STEP_BOUND, 'one point 64 times, lambda0 = 1e3')
    # at lambda0 = 1e-3 the reduced system stands on its damping alone and which steps are kept is decided by rounding; what does
    # not depend on it: the set, the counters before the first step, the start cost, a cost that never rises and finite output
    got = bundle_adjust(rep['points'], fx['cams'], fx['poses0'], rep['X0'], fixed_views=fx['fixed'], iters=5)
    want = bo.bundle_adjust(rep['points'], fx['cams'], fx['poses0'], rep['X0'], fixed_views=fx['fixed'], iters=5)
    assert np.array_equal(got['used'], want['used']) and np.array_equal(got['info'][:5], want['info'][:5])
    assert rel(got['stats'][:1], want['stats'][:1]) <= 1000 * bo.ORDER_NOISE_SUMS and got['stats'][1] <= got['stats'][0]
    assert np.isfinite(got['poses']).all() and np.isfinite(got['X']).all() and got['info'][5] + got['info'][6] <= 5

# ---- repeatability --------------------------------------------------------------------------------------------------------
def test_same_bits_across_calls_streams_scratch_and_graph_replay():
    fx = fixture(8, 1025)
    V, n, rounds, iters = 8, 1025, 2, 6
    d = [torch.from_numpy(np.ascontiguousarray(fx[k])).cuda() for k in ('points', 'cams', 'poses0', 'X0', 'used')]
    kw = dict(visible=d[4], fixed_views=(0, 1), rounds=rounds, iters=iters)
    first = host(bundle_adjust_tensors(d[0], d[1], d[2], d[3], **kw))
    again = host(bundle_adjust_tensors(d[0], d[1], d[2], d[3], **kw))
    assert first['info'][5] > 0 and first['info'][7] == rounds
    for k in first:
        assert np.array_equal(first[k], again[k], equal_nan=True), k
    lib = _lib.load_library()
    nbytes = ctypes.c_size_t()
    assert lib.cotr_bundle_adjust_scratch_bytes(V, n, ctypes.byref(nbytes)) == 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    fixed = (ctypes.c_uint8 * V)(1, 1, 0, 0, 0, 0, 0, 0)

    def buffers():
        return dict(s=torch.full((nbytes.value + 4096,), 0xA5, dtype=torch.uint8, device='cuda'), poses=torch.full((V, 12), -7.0, dtype=torch.float64, device='cuda'),
                    X=torch.full((n, 3), -7.0, dtype=torch.float64, device='cuda'), used=torch.full((V, n), 9, dtype=torch.uint8, device='cuda'),
                    stats=torch.full((4,), -7.0, dtype=torch.float64, device='cuda'), info=torch.full((8,), -3, dtype=torch.int32, device='cuda'))

    def enqueue(b, stream):
        rc = lib.cotr_bundle_adjust(p(d[0]), p(d[4]), p(d[1]), p(d[2]), p(d[3]), fixed, V, n, None, 4.0, 50.0, rounds, iters, 1e-3, p(b['poses']),
                                    p(b['X']), p(b['used']), p(b['stats']), p(b['info']), p(b['s']), nbytes.value + 4096, stream)
        assert rc == 0, lib.cotr_raster_last_error()

    def same(b):
        for k in first:
            g = b[k].cpu().numpy()
            assert np.array_equal(g.reshape(first[k].shape), first[k].astype(g.dtype), equal_nan=True), k
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


# ---- the chains -----------------------------------------------------------------------------------------------------------
def _two_views(n=300, seed=1):
    sc = so.scene(2, n, noise=0.5, seed=seed)
    K = [so.camera_matrix(c) for c in sc['cams']]
    img = np.random.default_rng(seed).integers(0, 255, (480, 640, 3), dtype=np.uint8)
    return np.concatenate([sc['points'][0], sc['points'][1]], axis=1), img, K, [so.c2w_of(p) for p in sc['poses']], sc


def test_reconstruct_with_bundle_rounds_equals_the_calls_one_by_one():
    corrs, img, K, c2w, sc = _two_views()
    plain = reconstruct_tensors(corrs, img, img, K[0], K[1], c2w[0], c2w[1])
    zero = reconstruct_tensors(corrs, img, img, K[0], K[1], c2w[0], c2w[1], bundle_rounds=0)
    tri = triangulate_points_tensors(corrs[:, :2], corrs[:, 2:], K[0], K[1], c2w1=c2w[0], c2w2=c2w[1])
    assert set(zero) == set(plain) and 'poses' not in zero and 'bundle' not in zero
    hp, hz, ht = host(plain), host(zero), host(tri)
    for k in hp:
        assert np.array_equal(hp[k], hz[k], equal_nan=True), k
    for k in ('X', 'used', 'quality', 'info'):           # what the call returned before it could run a bundle adjustment
        assert np.array_equal(hz[k], ht[k], equal_nan=True), k
    chained = reconstruct_tensors(corrs, img, img, K[0], K[1], c2w[0], c2w[1], bundle_rounds=2)
    poses = np.stack([np.linalg.inv(m)[:3].reshape(12) for m in c2w])
    apart = host(bundle_adjust_tensors(np.stack([corrs[:, :2], corrs[:, 2:]]), sc['cams'], poses, ht['X'], visible=ht['used'] & ht['mask'][None],
                                       fixed_views=(0,), rounds=2))
    hc = host(chained)
    assert np.array_equal(hc['X'], apart['X'], equal_nan=True) and np.array_equal(hc['poses'], apart['poses'])
    hb = host(chained['bundle'])
    assert all(np.array_equal(hb[k], apart[k]) for k in ('used', 'stats', 'info')) and hb['info'][7] == 2 and hb['info'][5] > 0
    assert np.array_equal(hc['mask'], hp['mask']) and np.array_equal(hc['colors'], hp['colors'])
    assert np.array_equal(hc['poses'][0].reshape(12), poses[0]) and (hc['poses'][1].reshape(12) != poses[1]).any()
    # without poses: the found flag of the pose estimate is chained through the triangulation into the bundle adjustment
    free = reconstruct_tensors(corrs, img, img, K[0], K[1], bundle_rounds=1, pose_kw=dict(threshold=1.0, max_iters=100, seed=3))
    hf, pose = host(free), host(free['pose'])
    assert pose['info'][0] and host(free['bundle'])['info'][0] == 1 and np.array_equal(hf['poses'][0].reshape(12), np.eye(3, 4).reshape(12))
    tri = host(triangulate_points_tensors(corrs[:, :2], corrs[:, 2:], K[0], K[1], R=pose['R'], t=pose['t']))
    start = np.stack([np.eye(3, 4).reshape(12), np.concatenate([pose['R'].reshape(3, 3), pose['t'].reshape(3, 1)], axis=1).reshape(12)])
    one = host(bundle_adjust_tensors(np.stack([corrs[:, :2], corrs[:, 2:]]), sc['cams'], start, tri['X'], visible=tri['used'] & tri['mask'][None],
                                     fixed_views=(0,), rounds=1))
    assert np.array_equal(hf['X'], one['X'], equal_nan=True) and np.array_equal(hf['poses'], one['poses'])


def test_zoom_engine_reconstruct_with_bundle_rounds():
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
        r = eng.reconstruct(img_a, img_b, K_a, K_b, c2w_a, c2w_b, queries_a=q, threshold=50.0, bundle_rounds=2)
        r0 = eng.reconstruct(img_a, img_b, K_a, K_b, c2w_a, c2w_b, queries_a=q, threshold=50.0)
    assert 'poses' not in r0 and tuple(r['poses'].shape) == (2, 3, 4) and r['poses'].is_cuda
    free = reconstruct_tensors(r['corrs'].cpu().numpy(), img_a, img_b, K_a, K_b, c2w_a, c2w_b, threshold=50.0, bundle_rounds=2)
    hr, hf = host(r), host(free)
    for k in hf:
        assert np.array_equal(hr[k], hf[k], equal_nan=True), k
    assert all(np.array_equal(a, b) for a, b in zip(host(r['bundle']).values(), host(free['bundle']).values()))
