"""cotr_icp_maps and cotr_icp_multiview on the device against the numpy restatement tests/icp_multi_oracle.py (DESIGN.md
3h-15): the maps bit for bit; from the device's own poses after k steps, every association and pair count exactly, every
other band sum within the bound of the sum of its absolute terms, the kept edges and free views exactly, and the poses after
k + 1 steps within the bound of one restatement step - or, where the restatement stops, the same poses bit for bit with its
stop reason.  The bound is 1000 times the order noise of one step measured on the CPU (tests/test_icp_multi_cpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.data import Capture
from cotr_amd.inference import TsdfVolume, ZoomEngine, fuse_captures, icp_depth, icp_multiview, refine_poses, vertex_normal_maps
from tests import icp_multi_oracle as mo
from tests import icp_oracle as io

pytestmark = pytest.mark.gpu

STEPS = 3   # k = 0 .. 3
ALL4 = mo.all_pairs(4)
ISLAND = np.array([(0, 1), (1, 0), (2, 3), (3, 2)], np.int32)


def host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def dev(sc, iters, edges, **kw):
    args = dict(max_dist=mo.MAX_DIST, edge=sc['edge'], centre=sc['centre'], tables=True)
    args.update(kw)
    return host(icp_multiview(sc['depths'], sc['Ks'], sc['start'], edges=edges, iters=iters, **args))


def check_against_restatement(sc, edges, steps=STEPS, stride=1, fixed=(0,), found=None, bound=mo.STEP_BOUND, chain=True, what=''):
    n = len(sc['maps'])
    edges = np.asarray(edges, np.int32).reshape(-1, 2)
    kw = dict(stride=stride, fixed=fixed, found=found)
    runs = [dev(sc, k, edges, **kw) for k in range(steps + 2)]
    assert np.array_equal(runs[0]['maps'], sc['maps'], equal_nan=True)
    n_src = runs[0]['assoc'].shape[1]
    worst_sum, worst_step, left_out = 0.0, 0.0, 0
    for k in range(steps + 1):
        r, nxt = runs[k], runs[k + 1]
        poses = list(r['c2w'])
        ev = mo.evaluate(sc['maps'], sc['Ks'], poses, edges, sc['centre'], found, stride=stride)
        near = ev['near']
        left_out = max(left_out, int(near.sum(axis=1).max()))
        assert (near.sum(axis=1) <= 0.001 * n_src).all()
        assert r['assoc'].shape == ev['assoc'].shape and np.array_equal(r['assoc'][~near], ev['assoc'][~near]), (what, k)
        sums = r['edge_sums']
        assert not sums[:, :, 30:].any() and np.array_equal(sums[:, :, 29], ev['edge_out'][:, :, 29]), (what, k)
        assert not sums[~ev['live']].any()
        if not near.any():
            assert np.array_equal(sums[:, :, 28], ev['edge_out'][:, :, 28]), (what, k)
        rel = np.abs(sums[:, :, :28] - ev['edge_out'][:, :, :28]) / np.where(ev['abs'][:, :, :28] > 0, ev['abs'][:, :, :28], 1.0)
        worst_sum = max(worst_sum, rel.max())
        assert (rel <= bound).all(), (what, k, rel.max())
        # the gate, the free views and the counts: from the device's own sums, exactly
        last = mo.solve(sums, edges, n, fixed, found, last=True)
        stopped = r['info'][3] != 0
        assert r['info'][2] == last['pairs'] and r['info'][4] == ev['live'].sum() and r['info'][5] == last['kept'].sum() and r['info'][6] == last['F']
        assert np.array_equal(r['view_info'], last['view_info']), (what, k)
        assert abs(r['stats'][0] - last['err']) <= 1e-13 * last['err'] and r['info'][7] == 0
        assert abs(r['stats'][1] - (np.sqrt(last['err'] / last['pairs']) if last['pairs'] else 0.0)) <= 1e-13 * max(1.0, r['stats'][1])
        row = r['hist'][r['info'][1]]
        assert row[0] == r['stats'][0] and row[1] == r['info'][2] and row[3] == 0 and (r['hist'][r['info'][1] + 1:] == 0).all()
        assert r['info'][0] == (0 if stopped else 1)
        # one step of the restatement from the device's poses
        so = mo.solve(ev['edge_out'], edges, n, fixed, found)
        assert np.array_equal(so['kept'], last['kept']) and np.array_equal(so['free'], last['free'])
        if so['reason'] == 0:
            want = mo.apply(poses, so['x'], sc['centre'])
            dist = mo.pose_distance(list(nxt['c2w']), want)
            worst_step = max(worst_step, dist)
            assert dist <= bound, (what, k, dist)
            assert nxt['info'][1] == r['info'][1] + 1 == k + 1
            assert abs(nxt['hist'][k, 2] - so['ratio']) <= 1e-9 * so['ratio']
            for v in range(n):
                if not so['free'][v]:
                    assert np.array_equal(nxt['c2w'][v], r['c2w'][v])
        else:
            assert np.array_equal(nxt['c2w'], r['c2w']) and nxt['info'][3] == so['reason'] and nxt['info'][0] == 0, (what, k)
            assert np.array_equal(nxt['c2w'], np.stack(sc['start'])) or k > 0
    r = runs[steps]
    if chain:
        o = mo.multiview(sc['maps'], sc['Ks'], sc['start'], edges, fixed, sc['centre'], found, iters=steps, stride=stride)
        assert list(r['info']) == list(o['info']), (what, r['info'], o['info'])
        assert np.array_equal(r['view_info'], o['view_info'])
    print(f'{what}: info {r["info"].tolist()}, sums within {worst_sum:.2e}, a step within {worst_step:.2e} (bound {bound:.1e}), '
          f'at most {left_out} of {n_src} source pixels of an edge near a decision')
    return r


# ---- the maps --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(3, 3), (7, 9), (8, 8), (17, 241), (96, 128)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_maps_bit_for_bit(size):
    H, W = size
    sc = mo.scene(H, W, 0.05, 32)
    zero = sc['depths'].copy()
    zero[:, H // 2, W // 2] = 0.0           # a pixel without a vertex, and its neighbours without a normal
    pair = None
    for n in (1, 2, 4, 32):
        maps, info = vertex_normal_maps(zero[:n], sc['Ks'][:n], 0.05)
        maps, info = maps.cpu().numpy(), info.cpu().numpy()
        want = np.stack([io.maps(zero[v], sc['Ks'][v], 0.05) for v in range(n)])
        assert maps.shape == (n, H, W, 6) and np.array_equal(maps, want, equal_nan=True)
        assert np.array_equal(info[:, 0], (~np.isnan(want[..., 0])).sum(axis=(1, 2))) and np.array_equal(info[:, 1], (~np.isnan(want[..., 3])).sum(axis=(1, 2)))
        assert not info[:, 2:].any() and info[0, 0] <= H * W - 1
        if pair is None:   # the pairwise call's own map of the same depth
            pair = host(icp_depth(zero[0], sc['Ks'][0], zero[0], sc['Ks'][0], np.eye(3), np.zeros(3), 0.25, iters=0, tables=True))['maps_a']
        assert np.array_equal(maps[0], pair, equal_nan=True)


# ---- every size ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', mo.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_every_stage_at_every_size(size):
    H, W = size
    r = check_against_restatement(mo.scene(H, W), ALL4, what=f'4 views at {H}x{W}')
    if size == (3, 3):
        assert list(r['info']) == [0, 0, 0, 1, 12, 0, 0, 0]
    else:
        assert r['info'][3] == 0 and r['info'][1] == STEPS and 6 <= r['info'][5] <= 12


@pytest.mark.parametrize('stride', [1, 2, 3])
def test_every_stage_at_every_stride(stride):
    r = check_against_restatement(mo.scene(96, 128), ALL4, stride=stride, what=f'4 views at 96x128, stride {stride}')
    assert r['info'][3] == 0 and r['assoc'].shape == (12, -(-96 // stride) * -(-128 // stride))


def test_two_views_are_the_pairwise_evaluation():
    sc = mo.scene(96, 128)
    two = dict(sc, depths=sc['depths'][:2], Ks=sc['Ks'][:2], start=sc['start'][:2], maps=sc['maps'][:2])
    r = check_against_restatement(two, [(0, 1)], what='2 views')
    first = dev(two, 0, [(0, 1)])
    R, t = mo.relative(*two['start'])
    p = host(icp_depth(two['depths'][0], two['Ks'][0], two['depths'][1], two['Ks'][1], R, t, mo.MAX_DIST, edge=sc['edge'], iters=0, tables=True))
    assert np.array_equal(first['assoc'][0], p['assoc']) and first['info'][2] == p['info'][2] and first['edge_sums'][0, :, 29].sum() == p['info'][4]
    assert abs(first['stats'][0] - p['stats'][0]) <= mo.STEP_BOUND * p['stats'][0]
    assert r['info'][6] == 1


def test_three_views():
    sc = mo.scene(16, 16, n=3)
    r = check_against_restatement(sc, mo.all_pairs(3), what='3 views at 16x16')
    assert r['info'][3] == 0 and r['info'][6] == 2


@pytest.mark.parametrize('graph', ['ring', 'all'])
def test_32_views(graph):
    sc = mo.scene(16, 16, n=32)
    edges, bound = (mo.ring(32), mo.STEP_BOUND_RING32) if graph == 'ring' else (mo.all_pairs(32), mo.STEP_BOUND)
    r = check_against_restatement(sc, edges, steps=0, bound=bound, chain=False, what=f'32 views at 16x16, {graph}')
    assert r['info'][6] == 31 and r['info'][4] == len(edges) and r['info'][5] == len(edges) and r['info'][3] == 0
    after = dev(sc, 1, edges)
    assert after['info'][1] == 1 and after['hist'][0, 2] > 1e-4


# ---- graphs that do not solve, and views that take no part ----------------------------------------------------------------------
def test_an_island_is_singular_and_returns_the_start():
    sc = mo.scene(16, 16)
    r = check_against_restatement(sc, ISLAND, what='island')
    assert list(r['info'][[0, 1, 3, 4, 5, 6]]) == [0, 0, 2, 4, 4, 3] and np.array_equal(r['c2w'], np.stack(sc['start']))
    assert (r['hist'][1:] == 0).all() and r['hist'][0, 2] == 0


def test_duplicate_and_dead_edges():
    sc = mo.scene(16, 16)
    edges = np.concatenate([ALL4[:5], ALL4[2:3], [(0, 4)], [(-1, 2)], [(2, 2)], ALL4[5:8]]).astype(np.int32)
    r = check_against_restatement(sc, edges, what='dead edges')
    plain = dev(sc, STEPS, ALL4[:8])
    assert r['info'][4] == 8 and (r['assoc'][5:9] == -1).all() and not r['edge_sums'][5:9].any()
    assert np.array_equal(r['edge_sums'][[0, 1, 2, 3, 4, 9, 10, 11]], plain['edge_sums'])
    assert np.array_equal(r['c2w'], plain['c2w'])   # the same system, entry for entry


@pytest.mark.parametrize('lost', [0, 2, 3])
def test_found_with_a_zero(lost):
    sc = mo.scene(16, 16)
    found = np.ones(4, np.int32)
    found[lost] = 0
    r = check_against_restatement(sc, ALL4, found=found, what=f'view {lost} not found')
    assert r['info'][4] == 6 and not r['view_info'][lost].any() and np.array_equal(r['c2w'][lost], sc['start'][lost])
    assert r['info'][3] == (2 if lost == 0 else 0)
    d = dev(sc, 2, ALL4, found=torch.from_numpy(found).cuda())
    assert np.array_equal(d['c2w'], dev(sc, 2, ALL4, found=found)['c2w'])


def test_two_fixed_views():
    sc = mo.scene(16, 16)
    r = check_against_restatement(sc, ALL4, fixed=(0, 2), what='views 0 and 2 fixed')
    assert r['info'][6] == 2 and list(r['view_info'][:, 0]) == [0, 1, 0, 1] and np.array_equal(r['c2w'][2], sc['start'][2])


# ---- the same bits -----------------------------------------------------------------------------------------------------------
def test_same_bits_across_calls_streams_garbage_and_graph_replay():
    sc = mo.scene(32, 64)
    first, again = dev(sc, 3, ALL4), dev(sc, 3, ALL4)
    assert first['info'][0] == 1 and first['info'][1] == 3
    for k in first:
        assert np.array_equal(first[k], again[k], equal_nan=True), k
    lib = _lib.load_library()
    n, H, W, E = 4, 32, 64, 12
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    depths = torch.from_numpy(sc['depths']).cuda()
    start, edges = torch.from_numpy(np.stack(sc['start'])).cuda(), torch.from_numpy(ALL4).cuda()
    K = (ctypes.c_double * 36)(*sc['Ks'].reshape(-1))
    C = (ctypes.c_double * 3)(*sc['centre'])

    def buffers():
        f = lambda shape: torch.full(shape, -7.0, dtype=torch.float64, device='cuda')   # noqa: E731
        i = lambda shape: torch.full(shape, -3, dtype=torch.int32, device='cuda')      # noqa: E731
        return dict(maps=f((n, H, W, 6)), minfo=i((n, 4)), c2w=f((n, 4, 4)), info=i((8,)), view_info=i((n, 4)), stats=f((2,)), edge_sums=f((E, 8, 32)),
                    hist=f((4, 4)), assoc=i((E, H * W)))

    def enqueue(b, stream):
        rc = lib.cotr_icp_maps(p(depths), n, H, W, K, sc['edge'], p(b['maps']), p(b['minfo']), stream)
        assert rc == 0, lib.cotr_raster_last_error()
        rc = lib.cotr_icp_multiview(p(b['maps']), n, H, W, K, p(start), p(edges), E, 1, C, None, mo.MAX_DIST, 0.5, 1e-9, 3, 1, p(b['c2w']), p(b['info']),
                                    p(b['view_info']), p(b['stats']), p(b['edge_sums']), p(b['hist']), p(b['assoc']), stream)
        assert rc == 0, lib.cotr_raster_last_error()

    def same(b):
        for k in ('maps', 'c2w', 'info', 'view_info', 'stats', 'edge_sums', 'hist', 'assoc'):
            assert np.array_equal(b[k].cpu().numpy(), first[k], equal_nan=True), k
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


# ---- on captures -------------------------------------------------------------------------------------------------------------
def _captures(sc, poses):
    H, W = sc['depths'].shape[1:]
    blank = np.zeros((H, W, 3), np.uint8)
    return [Capture(blank, sc['depths'][v], sc['Ks'][v], poses[v]) for v in range(len(poses))]


def test_refine_poses_with_min_overlap():
    from cotr_amd.inference.icp_multi import overlap_edges
    from cotr_amd.scene import overlap_matrix
    sc = mo.scene(32, 64)   # SWEEP_EDGE: with the default gate the coarse side walls have no normals, and the views slide on one plane
    caps = _captures(sc, sc['start'])
    dist = overlap_matrix(caps)
    cells = np.sort(dist.cpu().numpy()[~np.eye(4, dtype=bool)])
    cut = float((cells[3] + cells[4]) / 2)   # the four smallest cells go
    edges = overlap_edges(dist, cut).cpu().numpy()
    assert edges.shape == (12, 2) and (edges[:, 0] < 0).sum() == 4 and np.array_equal(edges[edges[:, 0] >= 0], ALL4[edges[:, 0] >= 0])
    poses, info = refine_poses(caps, min_overlap=cut, max_dist=mo.MAX_DIST, iters=6, edge=sc['edge'])
    o = mo.multiview(sc['maps'], sc['Ks'], sc['start'], edges, centre=mo.default_centre(sc['start']), iters=6)
    assert info['ok'] and info['steps'] == 6 and info['live_edges'] == 8 and info['pairs'] == o['info'][2] and info['stop'] == 'ran all'
    assert mo.pose_distance(poses, list(o['c2w'])) <= 6 * mo.STEP_BOUND
    everything, _ = refine_poses(caps, max_dist=mo.MAX_DIST, iters=6, edge=sc['edge'])
    before, after = (max(io.pose_distance(p[:3, :3], p[:3, 3], q[:3, :3], q[:3, 3]) for p, q in zip(x[1:], sc['true'][1:])) for x in (sc['start'], everything))
    print('refine_poses: the worst view from', before, 'to', after)
    assert after < before / 10


def test_zoom_engine_fuse_with_the_joint_step(monkeypatch):
    sc = mo.scene(96, 128, 0.05)
    caps = _captures(sc, sc['true'])
    placed = {id(cap.depth): pose for cap, pose in zip(caps, sc['start'])}
    monkeypatch.setattr(ZoomEngine, 'register', lambda self, a, b, **kw: (placed[id(b.depth)], None, None))
    engine = ZoomEngine.__new__(ZoomEngine)
    make = lambda: TsdfVolume((-4.0, -4.0, 2.0), 0.125, (64, 64, 48))   # noqa: E731
    vol0, poses0, found0 = engine.fuse(caps, make(), threshold=mo.MAX_DIST)
    assert found0 == [True] * 4 and np.array_equal(poses0[0], sc['true'][0]) and all(np.array_equal(p, q) for p, q in zip(poses0[1:], sc['start'][1:]))
    want, _ = fuse_captures([cap._replace(c2w=p) for cap, p in zip(caps, poses0)], make())
    assert torch.equal(vol0.tsdf, want.tsdf) and torch.equal(vol0.weight, want.weight)   # what the parent returns
    vol4, poses4, found4 = engine.fuse(caps, make(), joint_iters=4, threshold=mo.MAX_DIST)
    assert found4 == found0 and np.array_equal(poses4[0], poses0[0]) and (vol4.weight > 0).any()
    rmse0, rmse4 = (mo.all_edge_rmse(sc['maps'], sc['Ks'], list(x)) for x in (poses0, poses4))
    print('all-edge rmse of the fused poses: joint_iters=0', rmse0, 'joint_iters=4', rmse4)
    assert rmse4 <= rmse0
    with pytest.raises(ValueError, match='one depth-map size'):
        engine.fuse(caps[:3] + [caps[3]._replace(depth=sc['depths'][3][:, :120])], make(), joint_iters=4)
