"""The rule of the joint point-to-plane ICP (cotr_icp_maps, cotr_icp_multiview) on the CPU: the numpy
restatement tests/icp_multi_oracle.py against the pairwise restatement, against central differences and on the four-view
corner scene; the figures the device bounds stand on, measured again; and every argument check of the ABI and the wrappers,
none of which needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import icp_multiview, refine_poses, vertex_normal_maps
from tests import icp_multi_oracle as mo
from tests import icp_oracle as io
from tests import pnp_oracle as po

NAMES = ('cotr_icp_maps', 'cotr_icp_multiview')
ALL4 = mo.all_pairs(4)
ISLAND = np.array([(0, 1), (1, 0), (2, 3), (3, 2)], np.int32)


def first_step(sc, edges=ALL4, **kw):
    ev = mo.evaluate(sc['maps'], sc['Ks'], sc['start'], edges, sc['centre'], found=kw.get('found'))
    return ev, mo.solve(ev['edge_out'], edges, len(sc['maps']), **kw)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_two_views_take_the_step_of_the_pairwise_restatement():
    sc = io.corner_scene()
    rel = np.eye(4)
    rel[:3, :3], rel[:3, 3] = sc['R0'], sc['t0']
    poses = [sc['c2w_a'], sc['c2w_a'] @ rel]
    maps, Ks = [sc['maps_a'], sc['maps_b']], [sc['K_a'], sc['K_b']]
    R, t = mo.relative(*poses)
    pair = io.evaluate(sc['maps_a'], sc['K_a'], sc['maps_b'], R, t)
    # about the centre of camera b the twist is the pairwise parameterisation (R <- exp([w]x) R, t <- t + dt) seen from the world
    # frame, so the two steps are the same step; about any other centre they differ in second order
    for centre in (poses[1][:3, 3],):
        ev = mo.evaluate(maps, Ks, poses, [(0, 1)], centre)
        tot = mo.edge_totals(ev['edge_out'])[0]
        assert np.array_equal(ev['assoc'][0], pair['assoc']) and tot[28] == pair['sums'][28] and tot[29] == pair['usable'].sum()
        assert abs(tot[27] - pair['sums'][27]) <= 1e-13 * pair['sums'][27]   # the same terms, added per band
        so = mo.solve(ev['edge_out'], [(0, 1)], 2)
        assert so['reason'] == 0 and list(so['free']) == [False, True] and so['F'] == 1
        new = mo.apply(poses, so['x'], centre)
        assert np.array_equal(new[0], poses[0])
        reason, d, _, _ = io.step(pair['sums'])
        R1, t1 = io.apply(R, t, d)
        got = np.linalg.inv(new[0]) @ new[1]
        dist = io.pose_distance(got[:3, :3], got[:3, 3], R1, t1)
        print('two views against the pairwise step:', dist)
        assert reason == 0 and dist <= io.STEP_BOUND


def test_jacobian_of_both_views_is_the_central_difference_of_the_residual_at_fixed_pairs():
    sc = mo.scene(16, 16)
    poses, centre = sc['start'], sc['centre']
    a, b = 1, 2
    R, t = mo.relative(poses[a], poses[b])
    e = io.evaluate(sc['maps'][a], sc['Ks'][a], sc['maps'][b], R, t, mo.MAX_DIST)
    idx = np.flatnonzero(e['pairs'])[::7]
    assert len(idx) >= 10
    X = sc['maps'][b].reshape(-1, 6)[idx, :3]
    A = sc['maps'][a].reshape(-1, 6)[e['assoc'][idx]]

    def residual(pa, pb):
        Y = (X @ pb[:3, :3].T + pb[:3, 3] - pa[:3, 3]) @ pa[:3, :3]
        return ((Y - A[:, :3]) * A[:, 3:]).sum(axis=1)

    J = mo.jacobian(poses[a], centre, (X @ R.T + t), A[:, 3:])
    eps, worst = 1e-5, 0.0
    for i in range(6):
        d = np.zeros(6)
        d[i] = eps
        db = (residual(poses[a], mo.twist(poses[b], d, centre)) - residual(poses[a], mo.twist(poses[b], -d, centre))) / (2 * eps)
        da = (residual(mo.twist(poses[a], d, centre), poses[b]) - residual(mo.twist(poses[a], -d, centre), poses[b])) / (2 * eps)
        scale = np.abs(J[:, i]).max()
        worst = max(worst, np.abs(db - J[:, i]).max() / scale, np.abs(da + J[:, i]).max() / scale)
    print('jacobian against central differences, relative:', worst)
    assert worst <= 1e-8   # eps^2 of truncation, 1e-16 / eps of rounding


def test_convergence_to_a_plateau_on_the_four_views():
    sc = mo.scene(96, 128)
    true, start = sc['true'], sc['start']
    r = mo.multiview(sc['maps'], sc['Ks'], start, ALL4, iters=9, centre=sc['centre'])
    assert list(r['info']) == [1, 9, r['info'][2], 0, 12, 12, 3, 0] and r['info'][2] > 100000
    late = [mo.pose_distance(r['poses'][k], r['poses'][k - 1]) for k in (8, 9)]
    print('moves of the last two steps:', late)
    assert max(late) < 1e-9
    assert not any(ev['near'].any() for ev in r['evals'])
    for v in range(1, 4):
        before = po.rotation_error(start[v][:3, :3], true[v][:3, :3]), po.translation_error(start[v][:3, 3], true[v][:3, 3])
        after = po.rotation_error(r['c2w'][v][:3, :3], true[v][:3, :3]), po.translation_error(r['c2w'][v][:3, 3], true[v][:3, 3])
        print('view', v, before, '->', after)
        assert after[0] < before[0] / 20 and after[1] < before[1] / 20
    s = mo.multiview(sc['maps'], sc['Ks'], start, mo.star(4), iters=9, centre=sc['centre'])
    joint, star = (mo.all_edge_rmse(sc['maps'], sc['Ks'], list(x['c2w'])) for x in (r, s))
    print('all-edge rmse: joint', joint, 'star', star)
    assert joint <= star
    assert min(r['hist'][:-1, 2]) >= 0.1 and r['hist'][-1, 2] == 0.0


def test_three_by_three_has_no_edge_with_6_pairs_and_stops():
    sc = mo.scene(3, 3)
    r = mo.multiview(sc['maps'], sc['Ks'], sc['start'], ALL4, iters=3)
    assert list(r['info']) == [0, 0, 0, 1, 12, 0, 0, 0] and np.array_equal(r['c2w'], np.stack(sc['start']))
    assert not r['view_info'].any() and not r['hist'].any()


@pytest.mark.parametrize('H,W,least,kept', [(5, 5, 2, 6), (8, 8, 5, 10), (9, 8, 4, 10), (7, 9, 6, 12)])
def test_the_edge_gate_at_its_two_sides(H, W, least, kept):
    sc = mo.scene(H, W)
    ev, so = first_step(sc)
    pairs = mo.edge_totals(ev['edge_out'])[:, 28]
    assert pairs.min() == least and so['kept'].sum() == kept and np.array_equal(so['kept'], pairs >= 6)
    assert so['reason'] == 0 and so['F'] == 3 and so['pairs'] == pairs[pairs >= 6].sum()
    assert not ev['near'].any()


def test_an_island_is_singular_and_returns_the_start():
    sc = mo.scene(16, 16)
    r = mo.multiview(sc['maps'], sc['Ks'], sc['start'], ISLAND, iters=3)
    assert list(r['info'][[0, 1, 3, 4, 5, 6]]) == [0, 0, 2, 4, 4, 3] and np.array_equal(r['c2w'], np.stack(sc['start']))
    assert r['hist'][0, 2] == 0.0 and r['hist'][0, 1] == r['info'][2] > 0
    # tied to the fixed view by one edge, the same graph solves
    r = mo.multiview(sc['maps'], sc['Ks'], sc['start'], np.concatenate([ISLAND, [(1, 2)]]), iters=1)
    assert r['info'][3] == 0 and r['info'][1] == 1


def test_dead_edges_found_and_fixed_views():
    sc = mo.scene(16, 16)
    base = first_step(sc, ALL4[:8])[1]
    # a duplicate counts once, an index out of range and a == b not at all
    edges = np.concatenate([ALL4[:5], ALL4[2:3], [(0, 4)], [(-1, 2)], [(2, 2)], ALL4[5:8]])
    ev, so = first_step(sc, edges)
    assert list(np.flatnonzero(~ev['live'])) == [5, 6, 7, 8] and not ev['edge_out'][5:9].any() and (ev['assoc'][5:9] == -1).all()
    assert so['pairs'] == base['pairs'] and np.allclose(so['H'], base['H'], rtol=1e-13) and so['F'] == 3
    # a view that was not found takes no part
    for lost in (0, 2, 3):
        found = np.ones(4, np.int32)
        found[lost] = 0
        ev, so = first_step(sc, found=found)
        assert ev['live'].sum() == 6 and not so['free'][lost] and so['view_info'][lost].sum() == 0
        assert so['F'] == (3 if lost == 0 else 2) and so['reason'] == (2 if lost == 0 else 0)   # without view 0 nothing is tied down
    ev, so = first_step(sc, fixed=(0, 2))
    assert so['F'] == 2 and list(so['free']) == [False, True, False, True] and so['reason'] == 0 and sorted(so['x']) == [1, 3]


def test_the_pivot_ratio_gap_around_the_default():
    solvable, singular = [], []
    for H, W in mo.SIZES[1:]:
        sc = mo.scene(H, W)
        for edges in (ALL4, mo.star(4), mo.ring(4)):
            ev, so = first_step(sc, edges)
            if so['H'] is not None and so['F'] == 3 and so['kept'].sum() >= 3:
                solvable.append(mo.column_pivots(so['H']))
                assert abs(solvable[-1] - so['ratio']) <= 1e-9 * so['ratio']
        ev, so = first_step(sc, ISLAND)
        if so['H'] is not None:
            assert so['reason'] == 2
            singular.append(mo.column_pivots(so['H']))
    print('smallest solvable ratio', min(solvable), 'largest singular ratio', max(singular))
    assert len(solvable) >= 20 and len(singular) >= 8
    assert min(solvable) >= 100 * mo.PIVOT_TOL and max(singular) <= mo.PIVOT_TOL / 100


def test_order_noise_of_one_joint_step():
    worst, solving = 0.0, 0
    for H, W in mo.SIZES:
        sc = mo.scene(H, W)
        if first_step(sc)[1]['reason'] == 0:
            noise = mo.order_noise(sc)
            print(H, W, noise)
            worst, solving = max(worst, noise), solving + 1
    assert solving == len(mo.SIZES) - 1
    assert worst <= mo.ORDER_NOISE and mo.STEP_BOUND == 1000 * mo.ORDER_NOISE
    assert worst > mo.ORDER_NOISE / 100   # the bound is the noise measured, not a round number far above it


def test_order_noise_of_32_views():
    sc = mo.scene(16, 16, n=32)
    ring, full = mo.order_noise(sc, mo.ring(32)), mo.order_noise(sc, mo.all_pairs(32))
    print('32 views: ring', ring, 'all pairs', full)
    assert mo.ORDER_NOISE_RING32 / 100 < ring <= mo.ORDER_NOISE_RING32 and full <= mo.ORDER_NOISE
    assert mo.order_noise(mo.scene(16, 16, n=3), mo.all_pairs(3)) <= mo.ORDER_NOISE


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def declared_symbols():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cotr_hip.h')
    return set(re.findall(r'\b(cotr_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)))


def test_symbols_are_exported_and_declared():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and name in declared_symbols()
        assert getattr(_lib.load_library(), name) is not None


def test_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    P = ctypes.c_void_p(4096)           # never dereferenced: every call below fails its checks before any HIP call
    K = (ctypes.c_double * 36)(*([100.0, 0.5, 64.0, 0.0, 100.0, 48.0, 0.0, 0.0, 1.0] * 4))
    C = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    nan, inf = float('nan'), float('inf')
    odd8, odd4 = ctypes.c_void_p(4100), ctypes.c_void_p(4098)

    def bad_k(i, v):
        k = (ctypes.c_double * 36)(*K)
        k[i] = v
        return k

    def maps(d=P, n=4, H=96, W=128, Ks=K, edge=0.05, out=P, info=P):
        return lib.cotr_icp_maps(d, n, H, W, Ks, edge, out, info, None)

    for kw, word in ((dict(n=0), b'n must'), (dict(n=33), b'n must'), (dict(H=2), b'2^28'), (dict(W=2), b'2^28'), (dict(n=4, H=1 << 13, W=(1 << 13) + 1), b'2^28'),
                     (dict(edge=0.0), b'edge'), (dict(edge=inf), b'edge'), (dict(edge=nan), b'edge'), (dict(d=None), b'NULL'), (dict(Ks=None), b'NULL'),
                     (dict(out=None), b'NULL'), (dict(info=None), b'NULL'), (dict(Ks=bad_k(0, 0.0)), b'focal'), (dict(Ks=bad_k(27 + 4, 0.0)), b'focal'),
                     (dict(Ks=bad_k(11, nan)), b'focal'), (dict(d=odd4), b'aligned'), (dict(out=odd8), b'aligned'), (dict(info=odd4), b'aligned')):
        assert maps(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error() and b'cotr_icp_maps' in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())

    def call(m=P, n=4, H=96, W=128, Ks=K, c2w0=P, edges=P, E=12, fixed=1, centre=C, found=None, max_dist=0.25, normal_cos=0.5, pivot_tol=1e-9,
             iters=10, stride=1, c2w=P, info=P, view=P, stats=P, sums=P, hist=None, assoc=None):
        return lib.cotr_icp_multiview(m, n, H, W, Ks, c2w0, edges, E, fixed, centre, found, max_dist, normal_cos, pivot_tol, iters, stride, c2w,
                                      info, view, stats, sums, hist, assoc, None)

    for kw, word in ((dict(n=1), b'n must'), (dict(n=33), b'n must'), (dict(H=2), b'2^28'), (dict(W=2), b'2^28'), (dict(H=1 << 13, W=(1 << 13) + 1), b'2^28'),
                     (dict(E=0), b'E must'), (dict(E=13), b'E must'), (dict(n=2, E=3), b'E must'), (dict(fixed=0), b'fixed_mask'),
                     (dict(fixed=1 << 4), b'fixed_mask'), (dict(iters=-1), b'iters'), (dict(iters=65), b'iters'), (dict(stride=0), b'stride'),
                     (dict(stride=65), b'stride'), (dict(max_dist=0.0), b'max_dist'), (dict(max_dist=inf), b'max_dist'), (dict(max_dist=nan), b'max_dist'),
                     (dict(normal_cos=-1.5), b'normal_cos'), (dict(normal_cos=1.5), b'normal_cos'), (dict(normal_cos=nan), b'normal_cos'),
                     (dict(pivot_tol=0.0), b'pivot_tol'), (dict(pivot_tol=1.0), b'pivot_tol'), (dict(pivot_tol=nan), b'pivot_tol'),
                     (dict(m=None), b'NULL'), (dict(Ks=None), b'NULL'), (dict(c2w0=None), b'NULL'), (dict(edges=None), b'NULL'), (dict(centre=None), b'NULL'),
                     (dict(c2w=None), b'NULL'), (dict(info=None), b'NULL'), (dict(view=None), b'NULL'), (dict(stats=None), b'NULL'), (dict(sums=None), b'NULL'),
                     (dict(Ks=bad_k(4, 0.0)), b'focal'), (dict(Ks=bad_k(29, inf)), b'focal'),
                     (dict(centre=(ctypes.c_double * 3)(0.0, nan, 0.0)), b'centre'), (dict(centre=(ctypes.c_double * 3)(inf, 0.0, 0.0)), b'centre'),
                     (dict(m=odd8), b'aligned'), (dict(c2w0=odd8), b'aligned'), (dict(edges=odd4), b'aligned'), (dict(found=odd4), b'aligned'),
                     (dict(c2w=odd8), b'aligned'), (dict(info=odd4), b'aligned'), (dict(view=odd4), b'aligned'), (dict(stats=odd8), b'aligned'),
                     (dict(sums=odd8), b'aligned'), (dict(hist=odd8), b'aligned'), (dict(assoc=odd4), b'aligned')):
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error() and b'cotr_icp_multiview' in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
K = np.array([[100.0, 0.5, 6.0], [0.0, 100.0, 5.0], [0.0, 0.0, 1.0]])
D = np.ones((3, 10, 12), np.float32)
POSES = np.stack([np.eye(4)] * 3)


def _capture(depth=None, c2w=None):
    from cotr_amd.data import Capture
    return Capture(None, D[0] if depth is None else depth, K, np.eye(4) if c2w is None else c2w)


def test_wrapper_argument_errors_without_a_gpu():
    for kw, word in ((dict(depths=np.ones((3, 10, 12))), 'float32'), (dict(depths=D[0]), r'\[n, H, W\]'), (dict(depths=np.ones((33, 3, 3), np.float32)), '32'),
                     (dict(depths=np.ones((3, 2, 12), np.float32)), '3 x 3'), (dict(Ks=np.eye(4)), r'\[3, 3\]'), (dict(Ks=np.stack([K] * 2)), r'\[3, 3, 3\]'),
                     (dict(Ks=np.diag([0.0, 1.0, 1.0])), 'focal'), (dict(edge=0.0), 'edge'), (dict(edge=float('inf')), 'edge')):
        args = dict(depths=D, Ks=K)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            vertex_normal_maps(**args)
    for kw, word in ((dict(max_dist=0.0), 'max_dist'), (dict(max_dist=float('nan')), 'max_dist'), (dict(normal_cos=1.5), 'normal_cos'),
                     (dict(pivot_tol=0.0), 'pivot_tol'), (dict(pivot_tol=1.0), 'pivot_tol'), (dict(iters=-1), 'iters'), (dict(iters=65), 'iters'),
                     (dict(iters=1.5), 'iters'), (dict(stride=0), 'stride'), (dict(stride=65), 'stride'), (dict(edge=0.0), 'edge'),
                     (dict(maps_or_depths=D[:1]), 'between 2'), (dict(maps_or_depths=np.ones((3, 10, 12, 6), np.float32)), 'float64'),
                     (dict(maps_or_depths=np.ones((3, 10, 12, 5))), 'float64'), (dict(maps_or_depths=np.ones((3, 2, 12, 6))), '3 x 3'),
                     (dict(c2ws=POSES[:2]), 'c2ws'), (dict(c2ws=np.stack([np.eye(3)] * 3)), r'\[4, 4\]'), (dict(edges=np.zeros((0, 2), np.int32)), 'edges'),
                     (dict(edges=np.zeros((7, 2), np.int32)), 'edges'), (dict(edges=np.zeros((3, 3), np.int32)), 'edges'), (dict(fixed=()), 'fixed'),
                     (dict(fixed=(3,)), 'fixed'), (dict(fixed=(-1,)), 'fixed'), (dict(centre=(0.0, 1.0)), 'centre'), (dict(centre=(0.0, 1.0, float('nan'))), 'centre'),
                     (dict(found=np.ones(2, np.int32)), 'found'), (dict(Ks=np.eye(4)), r'\[3, 3\]')):
        args = dict(maps_or_depths=D, Ks=K, c2ws=POSES)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            icp_multiview(**args)
    caps = [_capture() for _ in range(3)]
    for args, kw, word in (((caps[:1],), {}, 'two captures'), ((caps[:2] + [_capture(np.ones((10, 13), np.float32))],), {}, 'one depth-map size'),
                           ((caps,), dict(edges=mo.star(3), min_overlap=0.1), 'not both'), ((caps, POSES[:2]), {}, 'c2ws'),
                           ((caps, [np.eye(4), None, np.eye(4)]), {}, r'\[4, 4\]'), ((caps,), dict(max_dist=0.0), 'max_dist'),
                           ((caps,), dict(iters=65), 'iters'), ((caps,), dict(fixed=(5,)), 'fixed'),
                           (([_capture(np.ones((2, 12), np.float32))] * 2,), {}, '3 x 3')):
        with pytest.raises(ValueError, match=word):
            refine_poses(*args, **kw)
    with pytest.raises(TypeError, match='unexpected keyword'):
        refine_poses(caps, max_dst=1.0)


def test_cpu_tensors_are_refused():
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        vertex_normal_maps(torch.ones((3, 10, 12)), K)
    for kw in (dict(maps_or_depths=torch.ones((3, 10, 12))), dict(maps_or_depths=torch.ones((3, 10, 12, 6), dtype=torch.float64)),
               dict(c2ws=torch.from_numpy(POSES)), dict(edges=torch.from_numpy(mo.star(3))), dict(found=torch.ones(3, dtype=torch.int32))):
        args = dict(maps_or_depths=D, Ks=K, c2ws=POSES)
        args.update(kw)
        with pytest.raises(_lib.CotrHipError, match='MI355X only'):
            icp_multiview(**args)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        refine_poses([_capture(torch.ones((10, 12))), _capture()])


def test_zoom_engine_fuse_hands_the_placed_captures_to_the_joint_step(monkeypatch):
    from cotr_amd.inference import ZoomEngine, icp_multi, tsdf
    caps = [_capture(c2w=np.eye(4) * 1.0) for _ in range(4)]
    placed = {id(caps[1]): np.eye(4) * 2.0, id(caps[2]): None, id(caps[3]): np.eye(4) * 3.0}
    calls = []
    engine = ZoomEngine.__new__(ZoomEngine)
    monkeypatch.setattr(ZoomEngine, 'register', lambda self, a, b, **kw: (placed[id(b)], None, None))
    monkeypatch.setattr(tsdf, 'fuse_captures', lambda caps, volume: calls.append(('fuse', [c.c2w[0, 0] for c in caps])))

    def fake(caps, c2ws, **kw):
        calls.append(('joint', [p[0, 0] for p in c2ws], kw))
        return [p + 0.5 for p in c2ws], {}
    monkeypatch.setattr(icp_multi, 'refine_poses', fake)
    _, poses, found = engine.fuse(caps, 'volume')
    assert calls == [('fuse', [1.0, 2.0, 3.0])] and found == [True, True, False, True] and poses[2] is None
    calls.clear()
    _, poses, found = engine.fuse(caps, 'volume', joint_iters=4, threshold=0.1)
    assert calls == [('joint', [1.0, 2.0, 3.0], dict(fixed=(0,), max_dist=0.1, iters=4)), ('fuse', [1.5, 2.5, 3.5])]
    assert found == [True, True, False, True] and poses[2] is None and poses[3][0, 0] == 3.5
    with pytest.raises(ValueError, match='one depth-map size'):
        engine.fuse(caps[:3] + [_capture(np.ones((10, 13), np.float32))], 'volume', joint_iters=4)
