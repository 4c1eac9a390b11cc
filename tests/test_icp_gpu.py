"""The dense point-to-plane ICP on the MI355X (cotr_amd/csrc/icp.hip) against the numpy restatement tests/icp_oracle.py: the
maps bit for bit, every evaluation from the device's own pose (association exactly, pair count exactly, the other sums and one
step within io.STEP_BOUND), the stop reasons, the plane scenes, the result against the scene, the gate, c2w_a,
repeatability, ``register_captures(..., icp_iters=10)`` and the engine call.

The bounds: io.STEP_BOUND = 1000 io.ORDER_NOISE = 1.6e-11, the restatement's own dependence on the order of its sums times
the family's margin, on the sums relative to the sums of their absolute terms and on the pose after
one step (entries of R, t relative to its norm).  Source pixels the restatement flags as near a decision (within 1e-9) may be
left out of the association comparison, at most 0.1 % of the usable ones.  Measured figures: DESIGN.md 3h-9."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.data import Capture, depth_corrs
from cotr_amd.inference import ZoomEngine, icp_depth, refine_registration, register_captures
from cotr_amd.inference import _args, icp as icp_mod
from cotr_amd.inference.rigid3d import register_captures_tensors
from tests import icp_oracle as io
from tests import pnp_oracle as po

pytestmark = pytest.mark.gpu

ITERS = 3   # the restatement has converged after 3 steps wherever it solves


def host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def dev(sc, iters, **kw):
    args = dict(max_dist=0.25, edge=sc['edge'], tables=True)
    args.update(kw)
    return host(icp_depth(sc['depth_a'], sc['K_a'], sc['depth_b'], sc['K_b'], sc['R0'], sc['t0'], iters=iters, **args))


def check_against_restatement(sc, stride=1, src_mask=None, iters=ITERS, what=''):
    kw = dict(stride=stride, src_mask=src_mask)
    runs = [dev(sc, k, **kw) for k in range(iters + 2)]
    # the maps: bit for bit, NaN exactly where the restatement has NaN
    assert np.array_equal(runs[0]['maps_a'], sc['maps_a'], equal_nan=True) and np.array_equal(runs[0]['maps_b'], sc['maps_b'], equal_nan=True)
    worst_sum, worst_step, left_out, usable = 0.0, 0.0, 0, 0
    for k in range(iters + 1):
        r, nxt = runs[k], runs[k + 1]
        e = io.evaluate(sc['maps_a'], sc['K_a'], sc['maps_b'], r['R'], r['t'], 0.25, 0.5, stride, src_mask)
        near = e['near']
        usable = int(e['usable'].sum())
        left_out = max(left_out, int(near.sum()))
        assert near.sum() <= 0.001 * usable
        assert r['assoc'].shape == e['assoc'].shape and np.array_equal(r['assoc'][~near], e['assoc'][~near]), (what, k)
        row = r['hist'][r['info'][1]]   # the evaluation at the returned pose: one evaluation follows each step
        assert (r['hist'][r['info'][1] + 1:] == 0).all()
        if np.array_equal(r['assoc'], e['assoc']):
            assert row[28] == e['sums'][28] == r['info'][2], (what, k)
        rel = np.abs(row[:28] - e['sums'][:28]) / np.where(e['abs'][:28] > 0, e['abs'][:28], 1.0)
        worst_sum = max(worst_sum, rel.max())
        assert (rel <= io.STEP_BOUND).all(), (what, k, rel.max())
        assert r['stats'][0] == row[27] and abs(r['stats'][1] - (np.sqrt(row[27] / row[28]) if row[28] else 0.0)) <= 1e-15 * max(1.0, r['stats'][1])
        # one step of the restatement from the device's pose
        reason, d, lmin, lmax = io.step(e['sums'])
        if reason == 0:
            R1, t1 = io.apply(r['R'], r['t'], d)
            dist = io.pose_distance(nxt['R'], nxt['t'], R1, t1)
            worst_step = max(worst_step, dist)
            assert dist <= io.STEP_BOUND, (what, k, dist)
            assert nxt['info'][1] == r['info'][1] + 1
            assert abs(nxt['hist'][k, 29] - lmin) <= 1e-9 * lmax and abs(nxt['hist'][k, 30] - lmax) <= 1e-12 * lmax
        else:
            assert np.array_equal(nxt['R'], r['R']) and np.array_equal(nxt['t'], r['t']) and nxt['info'][3] == reason, (what, k)
    o = io.icp(sc['maps_a'], sc['K_a'], sc['maps_b'], sc['R0'], sc['t0'], iters=iters, stride=stride, src_mask=src_mask)
    r = runs[iters]
    assert list(r['info']) == list(o['info']), (what, r['info'], o['info'])
    print(f'{what}: info {r["info"][:6].tolist()}, sums within {worst_sum:.2e}, a step within {worst_step:.2e} (bound {io.STEP_BOUND:.1e}), '
          f'{left_out} of {usable} usable source pixels near a decision ({100.0 * left_out / max(usable, 1):.3f} %)')
    return r, o


# ---- every size ------------------------------------------------------------------------------------------------------------
SWEEP = [((96, 128), b) for b in io.SIZES_B] + [((24, 32), b) for b in io.SIZES_B_SMALL_A]


@pytest.mark.parametrize('case', SWEEP, ids=lambda c: f'a{c[0][0]}x{c[0][1]}-b{c[1][0]}x{c[1][1]}')
def test_every_stage_at_every_size(case):
    (Ha, Wa), (Hb, Wb) = case
    sc = io.scene(Ha, Wa, Hb, Wb, 3, io.SWEEP_EDGE)
    r, o = check_against_restatement(sc, what=f'A {Ha}x{Wa}, B {Hb}x{Wb}')
    solves = (Ha, Wa, Hb, Wb) in io.solving_cases()
    assert (r['info'][3] == 0) == solves and (r['info'][1] == ITERS) == solves
    if Hb * Wb <= 25:
        assert r['info'][3] in (1, 2) and r['info'][2] <= 9


@pytest.mark.parametrize('stride', [1, 2, 3])
def test_every_stage_at_every_stride(stride):
    sc = io.corner_scene()
    r, _ = check_against_restatement(sc, stride=stride, what=f'stride {stride}')
    assert list(r['info'][[0, 1, 3]]) == [1, ITERS, 0] and len(r['assoc']) == -(-96 // stride) * -(-128 // stride)


@pytest.mark.parametrize('keep', [5, 6, 64])
def test_every_stage_with_a_source_mask(keep):
    sc = io.corner_scene()
    first = io.evaluate(sc['maps_a'], sc['K_a'], sc['maps_b'], sc['R0'], sc['t0'])
    pairs = np.flatnonzero(first['pairs'])
    mask = np.zeros(sc['depth_b'].shape, np.uint8)
    mask.reshape(-1)[pairs[:: len(pairs) // keep][:keep]] = 1
    assert mask.sum() == keep
    r, _ = check_against_restatement(sc, src_mask=mask, what=f'a source mask of {keep} pixels')
    assert r['info'][4] == keep and (r['info'][3] == 1) == (keep < 6)
    # a bool mask on the device is the same mask
    q = dev(sc, ITERS, src_mask=torch.from_numpy(mask.astype(bool)).cuda())
    assert all(np.array_equal(q[k], r[k], equal_nan=True) for k in r)


# ---- stops, the scene, the gate, c2w_a ----------------------------------------------------------------------------------
@pytest.mark.parametrize('planes', [1, 2])
def test_one_and_two_planes_return_the_start_bit_for_bit(planes):
    sc = io.scene(96, 128, 96, 128, planes)
    r = dev(sc, 5)
    o = io.icp(sc['maps_a'], sc['K_a'], sc['maps_b'], sc['R0'], sc['t0'], iters=5)
    ratio = r['hist'][0, 29] / r['hist'][0, 30]
    print(f'{planes} plane(s): l_min / l_max = {ratio:.2e} (restatement {o["hist"][0, 29] / o["hist"][0, 30]:.2e}), info {r["info"][:6].tolist()}')
    assert np.array_equal(r['R'], sc['R0']) and np.array_equal(r['t'], sc['t0'])
    assert list(r['info']) == list(o['info']) and r['info'][3] == 2 and r['info'][0] == 0 and r['info'][1] == 0
    assert ratio < 1e-7 and (r['hist'][1:] == 0).all() and np.array_equal(r['assoc'], o['assoc'])


def test_against_the_scene_at_96x128():
    sc = io.corner_scene()
    r = host(icp_depth(sc['depth_a'], sc['K_a'], sc['depth_b'], sc['K_b'], sc['R0'], sc['t0'], 0.25, iters=10))
    o = io.icp(sc['maps_a'], sc['K_a'], sc['maps_b'], sc['R0'], sc['t0'], iters=10)
    assert sorted(r) == ['R', 'info', 'stats', 't'] and r['R'].shape == (3, 3)
    d, w, s = io.errors(r['R'], r['t'], sc), io.errors(o['R'], o['t'], sc), io.errors(sc['R0'], sc['t0'], sc)
    print(f'96 x 128 from {s[0]:.3e} / {s[1]:.3e}: rotation {d[0]:.3e} (restatement {w[0]:.3e}), translation {d[1]:.3e} ({w[1]:.3e}), '
          f'{r["info"][2]} pairs, rmse {r["stats"][1]:.3e}')
    assert list(r['info']) == list(o['info']) and list(r['info'][[0, 1, 3]]) == [1, 10, 0]
    assert d[0] <= 1.5 * w[0] and d[1] <= 1.5 * w[1]
    assert np.abs(r['R'] @ r['R'].T - np.eye(3)).max() < 1e-14


def _device_args(sc):
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    return dict(depth_a=cu(sc['depth_a']), depth_b=cu(sc['depth_b']), R0=cu(sc['R0'].reshape(9)), t0=cu(sc['t0']),
                ka=_args.camera(sc['K_a'], 'K_a'), kb=_args.camera(sc['K_b'], 'K_b'))


def _enqueue(a, found, iters=ITERS, tables=True):
    return icp_mod._enqueue_icp(_lib.load_library(), a['depth_a'], a['ka'], a['depth_b'], a['kb'], a['R0'], a['t0'], None, found, None, 0.25, 0.5,
                                0.05, 1e-6, iters, 1, tables, torch.device('cuda', torch.cuda.current_device()))


def test_found_gates_the_chain():
    sc = io.corner_scene()
    a = _device_args(sc)
    off = host(_enqueue(a, torch.zeros(8, dtype=torch.int32, device='cuda')))
    for k in ('R', 't', 'info', 'stats', 'hist'):
        assert (off[k] == 0).all(), k
    assert (off['assoc'] == -1).all()
    on_, free = host(_enqueue(a, torch.tensor([1, 0, 0, 0], dtype=torch.int32, device='cuda'))), host(_enqueue(a, None))
    assert on_['info'][0] == 1 and all(np.array_equal(on_[k], free[k], equal_nan=True) for k in free)


def test_c2w_a_is_the_camera_frame_result_composed_on_the_host():
    sc = io.corner_scene()
    cam = dev(sc, ITERS)
    A = sc['c2w_a']
    start = A @ np.vstack([np.hstack([sc['R0'], sc['t0'][:, None]]), [0, 0, 0, 1]])
    w = host(icp_depth(sc['depth_a'], sc['K_a'], sc['depth_b'], sc['K_b'], start[:3, :3], start[:3, 3], 0.25, iters=ITERS, c2w_a=A, tables=True))
    assert np.abs(w['R'] - A[:3, :3] @ cam['R']).max() <= 1e-12 and np.abs(w['t'] - (A[:3, :3] @ cam['t'] + A[:3, 3])).max() <= 1e-12
    assert list(w['info']) == list(cam['info']) and np.array_equal(w['assoc'], cam['assoc'])
    # and refine_registration is that call with host results
    c2w, info = refine_registration(Capture(None, sc['depth_a'], sc['K_a'], A), Capture(None, sc['depth_b'], sc['K_b'], None), start, 0.25,
                                    iters=ITERS)
    assert np.array_equal(c2w[:3, :3], w['R']) and np.array_equal(c2w[:3, 3], w['t']) and np.array_equal(c2w[3], [0, 0, 0, 1])
    assert info == dict(ok=True, steps=ITERS, pairs=int(w['info'][2]), stop='ran all', source_pixels=int(w['info'][4]),
                        target_pixels=int(w['info'][5]), sum_r2=float(w['stats'][0]), rmse=float(w['stats'][1]))


def test_same_bits_across_calls_streams_scratch_and_graph_replay():
    sc = io.corner_scene()
    first, again = dev(sc, 4), dev(sc, 4)
    assert first['info'][0] == 1 and first['info'][1] == 4
    for k in first:
        assert np.array_equal(first[k], again[k], equal_nan=True), k
    # the C ABI directly: a side stream, a larger caller scratch full of garbage
    lib = _lib.load_library()
    a = _device_args(sc)
    nbytes = ctypes.c_size_t()
    assert lib.cotr_icp_depth_scratch_bytes(96, 128, 96, 128, 1, ctypes.byref(nbytes)) == 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def buffers():
        return dict(s=torch.full((nbytes.value + 4096,), 0xA5, dtype=torch.uint8, device='cuda'), R=torch.full((9,), -7.0, dtype=torch.float64, device='cuda'),
                    t=torch.full((3,), -7.0, dtype=torch.float64, device='cuda'), info=torch.full((8,), -3, dtype=torch.int32, device='cuda'),
                    stats=torch.full((2,), -7.0, dtype=torch.float64, device='cuda'), hist=torch.full((5, 32), -7.0, dtype=torch.float64, device='cuda'),
                    assoc=torch.full((96 * 128,), -9, dtype=torch.int32, device='cuda'))

    def enqueue(b, stream):
        rc = lib.cotr_icp_depth(p(a['depth_a']), 96, 128, a['ka'], p(a['depth_b']), 96, 128, a['kb'], p(a['R0']), p(a['t0']), None, None, None, 0.25,
                                0.5, 0.05, 1e-6, 4, 1, p(b['R']), p(b['t']), p(b['info']), p(b['stats']), p(b['hist']), p(b['assoc']), None, None,
                                p(b['s']), nbytes.value + 4096, stream)
        assert rc == 0, lib.cotr_raster_last_error()

    def same(b):
        assert np.array_equal(b['R'].cpu().numpy(), first['R'].reshape(9))
        for k in ('t', 'info', 'stats', 'hist', 'assoc'):
            assert np.array_equal(b[k].cpu().numpy(), first[k]), k
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


# ---- behind the sparse registration ----------------------------------------------------------------------------------------
def _captures_case(outliers):
    sc = io.corner_scene()
    H, W = sc['depth_a'].shape
    blank = np.zeros((H, W, 3), np.uint8)
    cap_a, cap_b = Capture(blank, sc['depth_a'], sc['K_a'], sc['c2w_a']), Capture(blank, sc['depth_b'], sc['K_b'], sc['c2w_b'])
    rng = np.random.default_rng(5)
    corrs = depth_corrs(cap_a, cap_b, subset=rng.permutation(H * W)[:600].astype(np.int64)).cpu().numpy()
    assert len(corrs) >= 300
    pa, pb = corrs[:, :2].copy(), corrs[:, 2:].copy()
    if outliers:
        bad = np.arange(len(pa)) % 4 == 0
        pb[bad] = rng.uniform([0, 0], [W - 1, H - 1], (int(bad.sum()), 2))
    return sc, cap_a, cap_b, pa, pb


@pytest.mark.parametrize('outliers', [False, True], ids=['exact', 'quarter-noise'])
def test_register_captures_with_the_dense_step(outliers):
    sc, cap_a, cap_b, pa, pb = _captures_case(outliers)
    kw = dict(threshold=0.05, confidence=0.999, max_iters=100, seed=2)
    plain, plain_mask = register_captures(pa, pb, cap_a, cap_b, **kw)
    zero, zero_mask = register_captures(pa, pb, cap_a, cap_b, icp_iters=0, **kw)
    assert np.array_equal(plain, zero) and np.array_equal(plain_mask, zero_mask)
    c2w, mask = register_captures(pa, pb, cap_a, cap_b, icp_iters=10, **kw)
    assert c2w.shape == (4, 4) and np.array_equal(c2w[3], [0, 0, 0, 1]) and np.array_equal(mask, plain_mask)
    r = host({k: v for k, v in register_captures_tensors(pa, pb, cap_a.depth, cap_a.K, cap_a.c2w, cap_b.depth, cap_b.K, icp_iters=10, **kw).items()
              if k != 'icp'})
    assert np.array_equal(r['R_sparse'], plain[:3, :3]) and np.array_equal(r['t_sparse'], plain[:3, 3])
    assert np.array_equal(r['R'], c2w[:3, :3]) and np.array_equal(r['t'], c2w[:3, 3])
    # the restatement from the same sparse result, in A's camera frame, and back
    A = cap_a.c2w
    rel = np.linalg.inv(A) @ plain
    o = io.icp(sc['maps_a'], sc['K_a'], sc['maps_b'], rel[:3, :3], rel[:3, 3], iters=10, max_dist=kw['threshold'])
    ow = A @ np.vstack([np.hstack([o['R'], o['t'][:, None]]), [0, 0, 0, 1]])
    truth = dict(R=cap_b.c2w[:3, :3], t=cap_b.c2w[:3, 3])
    s, d, w = io.errors(plain[:3, :3], plain[:3, 3], truth), io.errors(c2w[:3, :3], c2w[:3, 3], truth), io.errors(ow[:3, :3], ow[:3, 3], truth)
    print(f'register_captures on the corner: sparse {s[0]:.3e} / {s[1]:.3e}, with icp_iters=10 {d[0]:.3e} / {d[1]:.3e} '
          f'(restatement {w[0]:.3e} / {w[1]:.3e}), stop reason {o["info"][3]}, {o["info"][2]} pairs')
    assert d[0] <= 1.5 * w[0] and d[1] <= 1.5 * w[1]


def test_zoom_engine_register_with_the_dense_step():
    from tests.engine_fixtures import CyclicFakeModel, synthetic_pair
    img_a, img_b = synthetic_pair(1)
    H, W = img_a.shape[:2]
    Hb, Wb = img_b.shape[:2]
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    depth_a = (4.0 + xs / 64.0 + ys / 128.0).astype(np.float32)
    xs, ys = np.meshgrid(np.arange(Wb), np.arange(Hb))
    depth_b = (3.5 + xs / 96.0 + ys / 80.0).astype(np.float32)
    K_a = np.array([[300.0, 0.5, W / 2], [0.0, 310.0, H / 2], [0.0, 0.0, 1.0]])
    K_b = np.array([[280.0, -0.5, Wb / 2], [0.0, 290.0, Hb / 2], [0.0, 0.0, 1.0]])
    cap_a = Capture(img_a, depth_a, K_a, po.pose_matrix((5.0, -3.0, 2.0), (0.3, 0.1, -0.2)))
    cap_b = Capture(img_b, depth_b, K_b, np.eye(4))
    eng = ZoomEngine(CyclicFakeModel().cuda())
    rng = np.random.default_rng(0)
    q = np.stack([rng.uniform(5, W - 5, 40), rng.uniform(5, H - 5, 40)], 1).astype(np.float32)
    kw = dict(threshold=0.5, max_iters=100, seed=3, icp_iters=2, icp_max_dist=0.3)
    with torch.no_grad():
        c2w, corrs, mask = eng.register(cap_a, cap_b, queries_a=q, **kw)
    cw, mw = register_captures(corrs[:, :2], corrs[:, 2:], cap_a, cap_b, **kw)
    assert corrs.shape == (40, 4) and (c2w is None) == (cw is None) == (mask is None)
    if c2w is not None:
        assert np.array_equal(c2w, cw) and np.array_equal(mask, mw) and c2w.shape == (4, 4) and np.isfinite(c2w).all()
