"""Rotation averaging and the position solve on the MI355X (cotr_average_rotations, cotr_solve_positions in
cotr_amd/csrc/global_pose.hip) against the numpy restatement tests/global_pose_oracle.py: every shape edge, the dead edges, a
planted-outlier graph, one round and full runs of the position solve, the largest systems, degenerate input, repeatability, the
raw ABI between guard bands, and the chains built on both.

The device sums the same terms as the restatement in a third order, so R, C, X, the eigenvalues and the costs are held to 1000
times the order noise the CPU tests measured between two orders (global_pose_oracle.*_BOUND), not to bit equality; info,
view_info, located, used and the live and inlier flags are compared exactly."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import (ZoomEngine, average_rotations, average_rotations_host, bundle_adjust_tensors, reconstruct_views_tensors,
                                solve_positions, solve_positions_host, triangulate_views)
from cotr_amd.inference.essential import relative_pose_tensors
from tests import global_pose_oracle as go
from tests import structure_oracle as so
from tests.guard_arena import Arena

pytestmark = pytest.mark.gpu


def host(r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items() if torch.is_tensor(v)}


# ---- rotations ------------------------------------------------------------------------------------------------------------
def compare_rotations(got, want, bound, what):
    d = go.rotation_differences(got, want)
    print(f'{what}: info {list(got["info"])}, relative differences {d}, bound {bound:.1e}')
    assert np.array_equal(got['info'], want['info']) and np.array_equal(got['view_info'], want['view_info']), (what, got['info'], want['info'])
    assert np.array_equal(got['edge'][:, 2:], want['edge'][:, 2:]) and np.array_equal(got['located'], want['view_info'][:, 0]), what
    assert max(d.values()) <= bound, (what, d)


@pytest.mark.parametrize('n,E', go.AR_SHAPES)
def test_average_rotations_shapes(n, E):
    g = go.random_graph(n, E)
    for iters, bound in ((1, go.AR_STEP_BOUND), (12, go.AR_RUN_BOUND)):
        kw = dict(weights=g['weights'], found=g['found'], iters=iters)
        want = go.average_rotations(g['R_rel'], g['edges'], n, **kw)
        margin = np.abs(want['edge'][:, 0] / (3 * go.DEG) - 1)
        assert not (margin < 0.1).any()                          # (chosen on the CPU: no residual within 10 % of edge_thresh)
        got = average_rotations_host(g['R_rel'], g['edges'], n, weights=g['weights'], found=torch.from_numpy(g['found']).cuda(), iters=iters)
        compare_rotations(got, want, bound, f'n={n} E={E} iters={iters}')
        assert not got['live'][g['dead']].any() and got['info'][2] == E - len(g['dead'])


def test_average_rotations_root_weights_and_iters_0():
    g = go.random_graph(5, 20)
    for kw in (dict(root=3), dict(weights=None), dict(iters=0), dict(sigma0=8 * go.DEG, sigma_end=2 * go.DEG, edge_thresh=5 * go.DEG)):
        kw = dict(dict(weights=g['weights']), **kw)
        want = go.average_rotations(g['R_rel'], g['edges'], 5, **kw)
        got = average_rotations_host(g['R_rel'], g['edges'], 5, **kw)
        compare_rotations(got, want, go.AR_RUN_BOUND, f'{kw.keys()}')
        if kw.get('iters') == 0:                                 # the tree itself: products of the inputs, no sum to reorder
            assert go.rel(got['R'], want['tree']) <= go.AR_STEP_BOUND and got['info'][4] == 0 and np.array_equal(got['edge'][:, 1], np.where(got['live'] != 0, g['weights'], 0.0))


def test_average_rotations_planted_outliers_at_32_views():
    g = go.graph_fixture(32, 65)
    want = go.average_rotations(g['R_rel'], g['edges'], 32)
    got = average_rotations_host(g['R_rel'], g['edges'], 32)
    compare_rotations(got, want, go.AR_RUN_BOUND, 'graph_fixture(32, 65)')
    assert g['planted'].sum() == 11 and np.array_equal(got['inlier'] == 0, g['planted'])
    tree, avg = go.rotation_error_deg(want['tree'], g['truth']), go.rotation_error_deg(got['R'], g['truth'])
    print(f'32 views: the tree {tree:.2f} degrees off, the averaged rotations {avg:.2f}')
    assert tree > 20 and avg < 2


def test_average_rotations_unreached_view_and_dead_graph():
    g = go.random_graph(5, 3)                                     # the chain 0-1-2-3: view 4 is joined by no edge
    want = go.average_rotations(g['R_rel'], g['edges'], 5)
    got = average_rotations_host(g['R_rel'], g['edges'], 5)
    compare_rotations(got, want, go.AR_RUN_BOUND, 'view 4 unreached')
    assert list(got['located']) == [1, 1, 1, 1, 0] and np.isnan(got['R'][4]).all() and got['info'][0] == 1 and got['info'][1] == 4
    dead = average_rotations_host(g['R_rel'], g['edges'], 5, found=torch.zeros(3, dtype=torch.int32, device='cuda'))
    want = go.average_rotations(g['R_rel'], g['edges'], 5, found=np.zeros(3))
    compare_rotations(dead, want, go.AR_RUN_BOUND, 'every edge dead')
    assert list(dead['info']) == [0, 1, 0, 0, 0, 1, 0, 0] and np.array_equal(dead['R'][0], np.eye(3)) and np.isnan(dead['R'][1:]).all()


def test_average_rotations_refused_pivot_keeps_the_last_step():
    s = go.singular_graph()
    want = go.average_rotations(s['R_rel'], s['edges'], 3, weights=s['weights'])
    got = average_rotations_host(s['R_rel'], s['edges'], 3, weights=s['weights'])
    assert list(want['info']) == [0, 3, 3, 1, 2, 2, 0, 0]
    compare_rotations(got, want, go.AR_RUN_BOUND, 'stop reason 2')
    two = average_rotations_host(s['R_rel'], s['edges'], 3, weights=s['weights'], iters=2)   # the two steps that were taken, and no more
    assert two['info'][5] == 0 and np.array_equal(two['R'], got['R']) and np.array_equal(two['edge'], got['edge'])


# ---- positions ------------------------------------------------------------------------------------------------------------
def compare_positions(got, want, trace, bound, what):
    assert np.array_equal(got['used'], want['used']) and np.array_equal(got['info'], want['info']), (what, got['info'], want['info'])
    if not want['info'][0]:
        for k in ('C', 'X', 'poses', 'stats'):
            assert np.array_equal(got[k].reshape(want[k].shape), want[k], equal_nan=True), (what, k)
        return None
    V = got['C'].shape[0]
    scale = max(float(np.diag(trace[-1]['S']).max()), 1e-300)
    d = dict(lam0=abs(got['stats'][0] - want['stats'][0]) / scale, lam1=abs(got['stats'][1] - want['stats'][1]) / scale)
    if go.determined(trace[-1]) and all(go.determined(t) for t in trace):
        d.update(C=go.rel(got['C'], want['C']), poses=go.rel(got['poses'].reshape(V, 12), want['poses']), X=go.rel(got['X'], want['X']),
                 cost=go.rel(got['stats'][2:3], want['stats'][2:3]))
    print(f'{what}: info {list(got["info"])}, lambda {got["stats"][0]:.3e} {got["stats"][1]:.3e}, differences {d}, bound {bound:.1e}')
    assert max(d.values()) <= bound, (what, d)
    return d


def both_positions(fx, visible, **kw):
    trace = []
    want = go.solve_positions(fx['points'], fx['cams'], fx['R'], visible=visible, trace=trace, **kw)
    got = solve_positions_host(fx['points'], fx['cams'], fx['R'], visible=visible, **kw)
    return got, want, trace


@pytest.mark.parametrize('N', go.SP_NS)
@pytest.mark.parametrize('V', go.SP_VS)
def test_solve_positions_one_round(V, N):
    fx = go.step_fixture(V, N)
    for name, vis in fx['visibles']:
        got, want, trace = both_positions(fx, vis, rounds=1, min_obs=fx['min_obs'])
        # (chosen on the CPU: from 4 points on every fixture that succeeds is determined, so C, X, poses and the cost are compared)
        assert N < 4 or not want['info'][0] or go.determined(trace[0]), (V, N, name)
        assert N >= 4 or name != 'all' or want['info'][0] == 1   # one point seen by every view: the call succeeds, undetermined
        compare_positions(got, want, trace, go.SP_ROUND_BOUND, f'V={V} N={N} visible={name}')


@pytest.mark.parametrize('N', [65, 257])
def test_solve_positions_32_views(N):
    fx = go.step_fixture(32, N)
    got, want, trace = both_positions(fx, None, rounds=1)
    assert want['info'][2] == 32 and go.determined(trace[0])
    compare_positions(got, want, trace, go.SP_ROUND_BOUND, f'V=32 N={N}, 93 unknowns')


@pytest.mark.parametrize('shape', [(3, 64), (5, 257), (8, 300)])
def test_solve_positions_full_runs(shape):
    fx = go.position_fixture(*shape)
    got, want, trace = both_positions(fx, fx['visible'], rounds=3)
    assert min(t['margin'] for t in trace) >= 0.1 and all(go.determined(t) for t in trace)   # (met by the fixture's construction)
    assert np.array_equal(trace[1]['used'], trace[2]['used']) and want['info'][7] == 3
    d = compare_positions(got, want, trace, go.SP_RUN_BOUND, f'{shape} 3 rounds')
    assert d is not None and 'C' in d
    err, s = go.centre_error(got['C'], fx['sc']['poses'])
    print(f'{shape}: centre error {err / abs(s):.4f} of a baseline of 0.6')
    assert s > 0 and err / s < 0.03


def test_solve_positions_degenerate_input():
    fx = go.position_fixture(5, 257)
    args = (fx['points'], fx['cams'], fx['R'])
    zero = solve_positions_host(*args, visible=fx['visible'], found=torch.zeros(8, dtype=torch.int32, device='cuda'))
    assert all(not zero[k].any() for k in ('C', 'poses', 'X', 'used', 'stats', 'info'))
    on = solve_positions_host(*args, visible=fx['visible'], found=torch.ones(8, dtype=torch.int32, device='cuda'))
    plain = solve_positions_host(*args, visible=fx['visible'])
    assert all(np.array_equal(on[k], plain[k], equal_nan=True) for k in on)
    # NaN and infinite pixels, a NaN in a rotation (that view is not valid), a view that is not located, a starved view
    pts, R, vis = fx['points'].copy(), fx['R'].copy(), fx['visible'].copy()
    pts[2, 3, 0], pts[2, 4, 1], pts[0, 5] = np.nan, np.inf, -np.inf
    R[4, 1, 1] = np.nan
    vis[3, 5:] = False                                            # view 3 keeps at most 5 observations: below min_obs
    located = np.array([1, 1, 1, 1, 1], np.int32)
    trace = []
    want = go.solve_positions(pts, fx['cams'], R, visible=vis, located=located, trace=trace)
    got = solve_positions_host(pts, fx['cams'], R, visible=vis, located=torch.from_numpy(located).cuda())
    assert want['info'][0] == 1 and want['info'][2] == 3 and want['info'][3] == 1 and np.isnan(want['C'][[3, 4]]).all() and not want['used'][[3, 4]].any()
    compare_positions(got, want, trace, go.SP_RUN_BOUND, 'NaN, infinite, starved')
    located[2] = 0
    trace = []
    want = go.solve_positions(pts, fx['cams'], R, visible=vis, located=located, trace=trace)
    got = solve_positions_host(pts, fx['cams'], R, visible=vis, located=torch.from_numpy(located).cuda())
    assert want['info'][2] == 2 and np.isnan(want['C'][2]).all()
    compare_positions(got, want, trace, go.SP_RUN_BOUND, 'view 2 not located')
    # tracks that tie views 3 and 4 to each other but not to the root: ok stays 1, lambda1 says the solution is not determined
    vis = fx['visible'].copy()
    vis[:3, 128:], vis[3:, :128] = False, False
    got = solve_positions_host(*args, visible=vis, rounds=1)
    want = go.solve_positions(*args, visible=vis, rounds=1)
    assert got['info'][0] == 1 and np.array_equal(got['info'][:5], want['info'][:5]) and np.array_equal(got['used'], want['used'])
    big = np.abs(solve_positions_host(*args, visible=fx['visible'], rounds=1)['stats'][1])
    print(f'untied views: lambda0 {got["stats"][0]:.3e}, lambda1 {got["stats"][1]:.3e} against {big:.3e} with every track')
    assert abs(got['stats'][1]) < 1e-6 * big
    # two views: the baseline direction
    sc = so.scene(2, 64, seed=264)
    two = solve_positions_host(sc['points'], sc['cams'], go.true_rotations(sc))
    c_true = -(go.true_rotations(sc)[1].T @ sc['poses'][1].reshape(3, 4)[:, 3])
    assert two['info'][0] == 1 and abs(np.linalg.norm(two['C'][1]) - 1) < 1e-12 and two['C'][1] @ c_true / np.linalg.norm(c_true) > 0.999


# ---- repeatability and the raw ABI ----------------------------------------------------------------------------------------
def _raw_rotations(lib, d, n, E, out, stream):
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    rc = lib.cotr_average_rotations(p(d['R_rel']), p(d['edges']), p(d['weights']), p(d['found']), n, E, 0, 12, 32 * go.DEG, 1 * go.DEG, 3 * go.DEG,
                                    p(out['R']), p(out['edge']), p(out['view_info']), p(out['info']), p(out['stats']), stream)
    assert rc == 0, lib.cotr_raster_last_error()


def _raw_positions(lib, d, V, n, out, stream):
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    rc = lib.cotr_solve_positions(p(d['points']), p(d['visible']), p(d['cams']), p(d['R']), None, V, n, None, 0, 4.0, 3, 8, 16, p(out['C']),
                                  p(out['poses']), p(out['X']), p(out['used']), p(out['stats']), p(out['info']), p(out['work']), stream)
    assert rc == 0, lib.cotr_raster_last_error()


def _poisoned(spec):
    return {k: (torch.full(shape, 0xA5, dtype=torch.uint8, device='cuda') if dt == torch.uint8 else
                torch.full(shape, -7, dtype=dt, device='cuda')) for k, (shape, dt) in spec.items()}


@pytest.mark.parametrize('which', ['rotations', 'positions'])
def test_same_bits_across_calls_streams_work_and_graph_replay(which):
    lib = _lib.load_library()
    if which == 'rotations':
        g = go.graph_fixture(32, 65)
        n, E = 32, len(g['edges'])
        d = dict(R_rel=torch.from_numpy(g['R_rel']).cuda(), edges=torch.from_numpy(g['edges']).cuda(), weights=torch.ones(E, dtype=torch.float64, device='cuda'),
                 found=torch.ones(E, dtype=torch.int32, device='cuda'))
        first = host(average_rotations(d['R_rel'], d['edges'], n, weights=d['weights'], found=d['found']))
        again = host(average_rotations(d['R_rel'], d['edges'], n, weights=d['weights'], found=d['found']))
        spec = dict(R=((n, 9), torch.float64), edge=((E, 4), torch.float64), view_info=((n, 4), torch.int32), info=((8,), torch.int32),
                    stats=((2,), torch.float64))
        enqueue = lambda b, s: _raw_rotations(lib, d, n, E, b, s)   # noqa: E731
    else:
        fx = go.position_fixture(8, 300)
        V, n = 8, 300
        d = dict(points=torch.from_numpy(fx['points']).cuda(), visible=torch.from_numpy(fx['visible'].astype(np.uint8)).cuda(),
                 cams=torch.from_numpy(fx['cams']).cuda(), R=torch.from_numpy(np.ascontiguousarray(fx['R'])).cuda())
        first = host(solve_positions(d['points'], d['cams'], d['R'], visible=d['visible']))
        again = host(solve_positions(d['points'], d['cams'], d['R'], visible=d['visible']))
        count = ctypes.c_size_t()
        assert lib.cotr_solve_positions_work_doubles(V, n, ctypes.byref(count)) == 0
        spec = dict(C=((V, 3), torch.float64), poses=((V, 12), torch.float64), X=((n, 3), torch.float64), used=((V, n), torch.uint8),
                    stats=((4,), torch.float64), info=((8,), torch.int32), work=((count.value,), torch.float64))
        enqueue = lambda b, s: _raw_positions(lib, d, V, n, b, s)   # noqa: E731
    assert first['info'][0] == 1
    for k in first:
        assert np.array_equal(first[k], again[k], equal_nan=True), k

    def same(b):
        for k in spec:
            if k != 'work':
                g = b[k].cpu().numpy()
                assert np.array_equal(g.reshape(first[k].shape), first[k].astype(g.dtype), equal_nan=True), k
    b = _poisoned(spec)                                           # garbage in the work output, poisoned outputs, a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    enqueue(b, ctypes.c_void_p(side.cuda_stream))
    side.synchronize()
    same(b)
    b = _poisoned(spec)                                           # captured once (a single linear chain), replayed once
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue(b, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    graph.replay()
    torch.cuda.synchronize()
    same(b)


@pytest.mark.parametrize('n,E', [(2, 1), (32, 256), (32, 992)])
def test_average_rotations_between_guard_bands(n, E):
    g = go.random_graph(n, E)
    lib = _lib.load_library()
    for fill in (0xA5, 0x00):
        a = Arena('cuda', fill)
        a.add_input('R_rel', g['R_rel']).add_input('edges', g['edges']).add_input('weights', g['weights']).add_input('found', g['found'])
        a.add_output('R', np.float64, (n, 9)).add_output('edge', np.float64, (E, 4)).add_output('view_info', np.int32, (n, 4))
        a.add_output('info', np.int32, (8,)).add_output('stats', np.float64, (2,))
        a.build()
        rc = lib.cotr_average_rotations(a.ptr('R_rel'), a.ptr('edges'), a.ptr('weights'), a.ptr('found'), n, E, 0, 12, 32 * go.DEG, 1 * go.DEG, 3 * go.DEG,
                                        a.ptr('R'), a.ptr('edge'), a.ptr('view_info'), a.ptr('info'), a.ptr('stats'), None)
        assert rc == 0, lib.cotr_raster_last_error()
        torch.cuda.synchronize()
        a.check()
        want = average_rotations_host(g['R_rel'], g['edges'], n, weights=g['weights'], found=torch.from_numpy(g['found']).cuda())
        assert np.array_equal(a.view('R', np.float64, (n, 3, 3)), want['R'], equal_nan=True) and np.array_equal(a.view('info', np.int32, (8,)), want['info'])
        assert np.array_equal(a.view('edge', np.float64, (E, 4)), want['edge'], equal_nan=True)


@pytest.mark.parametrize('V,n', [(2, 1), (3, 256), (3, 257), (5, 2048), (5, 2049), (32, 65)])
def test_solve_positions_between_guard_bands(V, n):
    fx = go.step_fixture(V, n)
    vis = fx['visibles'][1][1].astype(np.uint8)
    lib = _lib.load_library()
    count = ctypes.c_size_t()
    assert lib.cotr_solve_positions_work_doubles(V, n, ctypes.byref(count)) == 0
    for fill in (0xA5, 0x00):
        a = Arena('cuda', fill)
        a.add_input('points', fx['points'], 'a16').add_input('visible', vis).add_input('cams', fx['cams']).add_input('R', np.ascontiguousarray(fx['R']))
        a.add_output('C', np.float64, (V, 3)).add_output('poses', np.float64, (V, 12)).add_output('X', np.float64, (n, 3)).add_output('used', np.uint8, (V, n))
        a.add_output('stats', np.float64, (4,)).add_output('info', np.int32, (8,)).add_output('work', np.float64, (count.value,))
        a.build()
        rc = lib.cotr_solve_positions(a.ptr('points'), a.ptr('visible'), a.ptr('cams'), a.ptr('R'), None, V, n, None, 0, 4.0, 2, fx['min_obs'], 16,
                                      a.ptr('C'), a.ptr('poses'), a.ptr('X'), a.ptr('used'), a.ptr('stats'), a.ptr('info'), a.ptr('work'), None)
        assert rc == 0, lib.cotr_raster_last_error()
        torch.cuda.synchronize()
        a.check()
        want = solve_positions_host(fx['points'], fx['cams'], fx['R'], visible=vis, rounds=2, min_obs=fx['min_obs'])
        for k, shape in (('C', (V, 3)), ('X', (n, 3)), ('stats', (4,))):
            assert np.array_equal(a.view(k, np.float64, shape), want[k], equal_nan=True), k
        assert np.array_equal(a.view('info', np.int32, (8,)), want['info']) and np.array_equal(a.view('used', np.uint8, (V, n)), want['used'])


# ---- the chains -----------------------------------------------------------------------------------------------------------
def _blocks(sc, V, span=2):
    """every view an anchor for the views within ``span``, every scene point a query of every anchor"""
    return [(a, [b for b in range(max(0, a - span), min(V, a + span + 1)) if b != a],
             np.stack([sc['points'][a]] + [sc['points'][b] for b in range(max(0, a - span), min(V, a + span + 1)) if b != a])) for a in range(V)]


def test_reconstruct_views_equals_the_calls_one_by_one():
    V, Q = 5, 257
    sc = so.scene(V, Q, seed=100 * V + Q)
    blocks = _blocks(sc, V)
    pose_kw = dict(threshold=2.0, max_iters=200, seed=3)
    r = reconstruct_views_tensors(blocks, sc['cams'], V, pose_kw=pose_kw, bundle_rounds=2)
    hr = host(r)
    assert hr['located'].all() and host(r['rotations'])['info'][0] == 1 and host(r['positions'])['info'][0] == 1
    # the same calls made one by one, with host arrays between them
    Ks = [so.camera_matrix(c) for c in sc['cams']]
    N = V * Q
    points, visible = np.full((V, N, 2), np.nan), np.zeros((V, N), bool)
    edges, R_rel, weights, found = [], [], [], []
    for i, (a, nbrs, pts) in enumerate(blocks):
        points[a, i * Q:(i + 1) * Q] = pts[0]
        for j, b in enumerate(nbrs):
            p = host(relative_pose_tensors(pts[0], pts[1 + j], Ks[a], Ks[b], refine_rounds=4, **pose_kw))
            points[b, i * Q:(i + 1) * Q] = pts[1 + j]
            visible[b, i * Q:(i + 1) * Q] = p['mask']
            visible[a, i * Q:(i + 1) * Q] |= p['mask']
            edges.append((a, b)), R_rel.append(p['R']), weights.append(float(p['mask'].sum())), found.append(p['info'][0])
    rot = average_rotations_host(np.stack(R_rel), np.array(edges, np.int32), V, weights=np.array(weights), found=torch.tensor(np.array(found), dtype=torch.int32).cuda())
    pos = solve_positions_host(points, sc['cams'], rot['R'], visible=visible, located=torch.from_numpy(rot['located']).cuda())
    tri = host(triangulate_views(points, sc['cams'], pos['poses'], visible=pos['used']))
    ba = host(bundle_adjust_tensors(points, sc['cams'], pos['poses'], tri['X'], visible=tri['used'] & tri['mask'][None], fixed_views=(0,), rounds=2))
    assert np.array_equal(host(r['rotations'])['R'], rot['R']) and np.array_equal(host(r['positions'])['C'], pos['C'])
    assert np.array_equal(hr['points'], points, equal_nan=True) and np.array_equal(hr['visible'], visible)
    assert np.array_equal(hr['poses'], ba['poses']) and np.array_equal(hr['X'], ba['X'], equal_nan=True) and np.array_equal(hr['mask'], tri['mask'])
    assert np.array_equal(hr['c2w'][:, :3, :3], np.transpose(ba['poses'][:, :, :3], (0, 2, 1))) and hr['c2w'].shape == (V, 4, 4)
    rot_err, (centre_err, s) = go.rotation_error_deg(hr['poses'][:, :, :3], go.true_rotations(sc)), go.centre_error(hr['c2w'][:, :3, 3], sc['poses'])
    print(f'(5, 257) at 0.5 px noise: rotations {rot_err:.3f} degrees, centres {centre_err / s:.4f} of a baseline of 0.6')
    assert rot_err < 0.5 and centre_err / s < 0.03


def test_reconstruct_views_noise_free_matches_ground_truth():
    """the bound: what the restatements reach on the same two-view results (rotation averaging and the position solve of
    tests/global_pose_oracle.py, then structure_oracle.triangulate and bundle_oracle.bundle_adjust), times 1000"""
    from tests import bundle_oracle as bo
    V, Q = 5, 257
    sc = so.scene(V, Q, seed=100 * V + Q, noise=0.0)
    r = reconstruct_views_tensors(_blocks(sc, V), sc['cams'], V, pose_kw=dict(threshold=1.0, max_iters=200, seed=3), bundle_rounds=2)
    hr = host(r)
    R_rel = np.stack([p['R'].cpu().numpy() for p in r['pairs']])
    weights = np.array([float(p['mask'].sum()) for p in r['pairs']])
    rot = go.average_rotations(R_rel, hr['edges'], V, weights=weights)
    pos = go.solve_positions(hr['points'], sc['cams'], rot['R'], visible=hr['visible'], located=rot['view_info'][:, 0])
    tri = so.triangulate(hr['points'], sc['cams'], pos['poses'], visible=pos['used'])
    ba = bo.bundle_adjust(hr['points'], sc['cams'], pos['poses'], tri['X'], visible=(tri['used'] != 0) & (tri['mask'] != 0)[None], fixed_views=(0,), rounds=2)

    def errors(poses):
        poses = np.asarray(poses).reshape(V, 3, 4)
        C = np.stack([-(p[:, :3].T @ p[:, 3]) for p in poses])
        e, s = go.centre_error(C, sc['poses'])
        return go.rotation_error_deg(poses[:, :, :3], go.true_rotations(sc)), e / s
    want, got = errors(ba['poses']), errors(hr['poses'])
    print(f'noise-free (5, 257): device {got}, restatements {want}')
    assert want[0] < 1e-3 and want[1] < 1e-4
    assert got[0] <= 1000 * want[0] and got[1] <= 1000 * want[1]


def test_zoom_engine_reconstruct_views(monkeypatch):
    V, Q = 4, 64
    sc = so.scene(V, Q, seed=100 * V + Q)
    imgs = [np.full((480, 640, 3), v, np.uint8) for v in range(V)]
    calls = []

    def fake(self, img_a, img_b, zoom_ins=(1.0,), converge_iters=1, max_corrs=1000, queries_a=None, force=False, **kw):
        a, b = int(img_a[0, 0, 0]), int(img_b[0, 0, 0])
        calls.append((a, b, force, max_corrs))
        assert np.array_equal(queries_a, sc['points'][a])
        return np.concatenate([sc['points'][a], sc['points'][b]], axis=1)
    monkeypatch.setattr(ZoomEngine, 'cotr_corr_multiscale', fake)
    eng = ZoomEngine.__new__(ZoomEngine)
    Ks = np.stack([so.camera_matrix(c) for c in sc['cams']])
    kw = dict(pose_kw=dict(threshold=2.0, max_iters=200, seed=3), bundle_rounds=1)
    r = eng.reconstruct_views(imgs, Ks, span=1, queries=[sc['points'][a] for a in range(V)], **kw)
    assert [c[:2] for c in calls] == [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2)] and all(c[2] and c[3] == Q for c in calls)
    free = reconstruct_views_tensors(_blocks(sc, V, span=1), sc['cams'], V, **kw)
    hr, hf = host(r), host(free)
    assert set(hr) == set(hf) and tuple(hr['c2w'].shape) == (V, 4, 4) and hr['located'].all()
    for k in hf:
        assert np.array_equal(hr[k], hf[k], equal_nan=True), k
