"""What the rules of DESIGN.md 3h-19 stand on, without a GPU: the numpy restatement tests/global_pose_oracle.py against
independent dense algebra (the graph step against a least-squares solve of the stacked edge equations, the reduced matrix against
the Schur complement of the dense normal matrix, the inverse iteration against numpy.linalg.eigh), the order noise the GPU tests'
bounds are made of, noise-free input, the fixtures of the prototype with the conditions they must meet, degenerate and edge
input, every argument error of the ABI and of the wrappers, and the host logic of the drivers."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import ZoomEngine, global_pose, structure
from tests import global_pose_oracle as go
from tests import structure_oracle as so


# ---- the pieces against independent algebra -------------------------------------------------------------------------------
def test_log_exp_round_trip():
    rng = np.random.default_rng(0)
    for scale in (1e-12, 1e-9, 1e-6, 1e-3, 0.1, 1.0, 3.0):
        for _ in range(20):
            w = rng.normal(size=3)
            w = w / np.linalg.norm(w) * scale * rng.uniform(0.5, 1.0)
            assert np.abs(go.log_so3(go.exp_so3(w)) - w).max() <= 1e-15 + 4e-16 * scale / max(np.sin(min(scale, np.pi - scale)), 1e-3)
    # a half turn: the magnitude is pi and the axis is the turn's, up to its sign
    for axis in (np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]), np.array([1.0, 2.0, -2.0]) / 3):
        r = go.log_so3(2 * np.outer(axis, axis) - np.eye(3))
        assert abs(go.norm3(r) - np.pi) < 1e-15 and abs(abs(r @ axis) - np.pi) < 1e-14
    assert np.array_equal(go.log_so3(np.eye(3)), np.zeros(3))
    R = so.rotation([0.3, -0.2, 0.5])
    assert np.abs(go.exp_so3(go.log_so3(R)) - R).max() < 1e-15


def test_graph_step_against_dense_least_squares():
    g = go.random_graph(32, 255)
    live, wt = go.dead_edges(g['R_rel'], g['edges'].astype(np.int64), 32, g['weights'], g['found'])
    rng = np.random.default_rng(1)
    er, ew = rng.normal(size=(255, 3)) * 0.01, wt * rng.uniform(0.1, 1.0, 255)
    free = list(range(1, 32))
    for order in ('asc', 'desc'):
        S, b, diag0 = go.laplacian_step(32, g['edges'].astype(np.int64), live, ew, er, free, order)
        x, _ = go.chol_solve(S, b, lambda col, p: p > go.PIVOT_TOL * diag0[col])
        # the stacked equations sqrt(w_e) (r_e + x_i - x_j) = 0 over the live edges, the root's x = 0
        rows, rhs = [], []
        for e in np.flatnonzero(live):
            i, j = g['edges'][e]
            for c in range(3):
                row = np.zeros(93)
                if i > 0:
                    row[3 * (i - 1) + c] = np.sqrt(ew[e])
                if j > 0:
                    row[3 * (j - 1) + c] = -np.sqrt(ew[e])
                rows.append(row), rhs.append(-np.sqrt(ew[e]) * er[e, c])
        want = np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)[0]
        assert np.abs(x - want).max() <= 1e-12 * np.abs(want).max()


def _dense_normal(P, used, V, N, root):
    """the normal matrix of sum |P_vp (X_p - C_v)|^2 over (C_0 .. C_V-1, X_0 .. X_N-1)"""
    H = np.zeros((3 * V + 3 * N, 3 * V + 3 * N))
    for v in range(V):
        for p in np.flatnonzero(used[v]):
            Pm = go.sym_full(P[v, p])
            c, x = slice(3 * v, 3 * v + 3), slice(3 * V + 3 * p, 3 * V + 3 * p + 3)
            H[c, c] += Pm
            H[x, x] += Pm
            H[c, x] -= Pm
            H[x, c] -= Pm
    return H


def test_reduced_matrix_against_the_dense_schur_complement():
    fx = go.position_fixture(5, 257)
    trace = []
    go.solve_positions(fx['points'], fx['cams'], fx['R'], visible=fx['visible'], rounds=1, trace=trace)
    used, S = trace[0]['used'], trace[0]['S']
    V, N = used.shape
    d, _ = go.rays(fx['points'], fx['cams'], fx['R'])
    H = _dense_normal(go.proj(d), used, V, N, 0)
    keep = [i for i in range(3 * V + 3 * N) if i >= 3 and (i < 3 * V or used[:, (i - 3 * V) // 3].any())]   # C_root = 0; unsolved points drop
    H = H[np.ix_(keep, keep)]
    m = 3 * (V - 1)
    want = H[:m, :m] - H[:m, m:] @ np.linalg.solve(H[m:, m:], H[m:, :m])
    assert np.abs(S - want).max() <= 1e-12 * np.abs(want).max() and np.array_equal(S, S.T)


def test_inverse_iteration_against_eigh():
    for shape in go.SHAPES:
        fx = go.position_fixture(*shape)
        trace = []
        go.solve_positions(fx['points'], fx['cams'], fx['R'], visible=fx['visible'], rounds=1, trace=trace)
        S, mu = trace[0]['S'], trace[0]['mu']
        lam, vec = np.linalg.eigh(S)
        for run, key in ((0, 'v0'), (1, 'v1')):
            # what one run can reach: the geometric rate of the iteration against the next eigenvalue, times 10; below it only
            # what rounding leaves of an eigenvector in either method, 10 eps |S| / gap
            gap = min(lam[run + 1] - lam[run], lam[run] - lam[run - 1] if run else np.inf)
            bound = 10 * ((lam[run] + mu) / (lam[run + 1] + mu)) ** 16 + 10 * np.finfo(np.float64).eps * lam[-1] / gap
            u, v = vec[:, run], trace[0][key]
            sine = float(np.linalg.norm(v - (v @ u) * u))
            got = trace[0]['lam0' if run == 0 else 'lam1']
            print(f'{shape} run {run}: sine {sine:.2e}, eigenvalue {got:.6e} against {lam[run]:.6e}, bound {bound:.2e}')
            assert sine <= bound and abs(got - lam[run]) <= bound * lam[run + 1]


# ---- the order noise ------------------------------------------------------------------------------------------------------
def _rotation_noise(a, b):
    assert np.array_equal(a['info'], b['info']) and np.array_equal(a['view_info'], b['view_info']) and np.array_equal(a['edge'][:, 2:], b['edge'][:, 2:])
    return max(go.rotation_differences(a, b).values())


def _position_noise(a, b, trace):
    assert np.array_equal(a['info'], b['info']) and np.array_equal(a['used'], b['used'])
    if not a['info'][0]:
        return 0.0
    scale = float(np.diag(trace[-1]['S']).max())
    d = [abs(a['stats'][0] - b['stats'][0]) / scale, abs(a['stats'][1] - b['stats'][1]) / scale]
    if all(go.determined(t) for t in trace):
        d += [go.rel(a['C'], b['C']), go.rel(a['X'], b['X']), go.rel(a['poses'], b['poses']), go.rel(a['stats'][2:3], b['stats'][2:3])]
    return max(d)


def test_order_noise():
    """the figures the constants of tests/global_pose_oracle.py were set from: the largest difference between the two orders
    over the fixtures the GPU tests use.  The GPU tests hold the device to 1000 times the constants."""
    noise = dict(ar_step=0.0, ar_run=0.0, sp_round=0.0, sp_run=0.0)
    for n, E in go.AR_SHAPES:
        g = go.random_graph(n, E)
        for iters, key in ((1, 'ar_step'), (12, 'ar_run')):
            kw = dict(weights=g['weights'], found=g['found'], iters=iters)
            a, b = go.average_rotations(g['R_rel'], g['edges'], n, **kw), go.average_rotations(g['R_rel'], g['edges'], n, order='desc', **kw)
            assert not (np.abs(a['edge'][:, 0] / (3 * go.DEG) - 1) < 0.1).any()       # no residual within 10 % of edge_thresh
            noise[key] = max(noise[key], _rotation_noise(a, b))
    g = go.graph_fixture(32, 65)
    noise['ar_run'] = max(noise['ar_run'], _rotation_noise(go.average_rotations(g['R_rel'], g['edges'], 32),
                                                           go.average_rotations(g['R_rel'], g['edges'], 32, order='desc')))
    for V in go.SP_VS + [32]:
        for N in (go.SP_NS if V < 32 else [65, 257]):
            fx = go.step_fixture(V, N)
            for _, vis in (fx['visibles'] if V < 32 else fx['visibles'][:1]):
                trace = []
                kw = dict(visible=vis, rounds=1, min_obs=fx['min_obs'] if V < 32 else 8)
                a = go.solve_positions(fx['points'], fx['cams'], fx['R'], trace=trace, **kw)
                noise['sp_round'] = max(noise['sp_round'], _position_noise(a, go.solve_positions(fx['points'], fx['cams'], fx['R'], order='desc', **kw), trace))
    for shape in [(3, 64), (5, 257), (8, 300)]:
        fx = go.position_fixture(*shape)
        trace = []
        a = go.solve_positions(fx['points'], fx['cams'], fx['R'], visible=fx['visible'], trace=trace)
        noise['sp_run'] = max(noise['sp_run'], _position_noise(a, go.solve_positions(fx['points'], fx['cams'], fx['R'], visible=fx['visible'], order='desc'), trace))
    print('order noise:', {k: f'{v:.2e}' for k, v in noise.items()})
    assert 0 < noise['ar_step'] <= go.AR_STEP_NOISE and 0 < noise['ar_run'] <= go.AR_RUN_NOISE
    assert 0 < noise['sp_round'] <= go.SP_ROUND_NOISE and 0 < noise['sp_run'] <= go.SP_RUN_NOISE
    assert go.AR_STEP_NOISE <= 2 * noise['ar_step'] and go.AR_RUN_NOISE <= 2 * noise['ar_run']           # the constants are the measurement,
    assert go.SP_ROUND_NOISE <= 2 * noise['sp_round'] and go.SP_RUN_NOISE <= 2 * noise['sp_run']          # not a margin on top of it


# ---- noise-free input -----------------------------------------------------------------------------------------------------
def test_noise_free_input_returns_the_truth():
    g = go.graph_fixture(32, 65, plant=False, noise_deg=0.0)
    r = go.average_rotations(g['R_rel'], g['edges'], 32)
    want = np.stack([Rv @ g['truth'][0].T for Rv in g['truth']])
    assert go.rel(r['R'], want) <= go.AR_RUN_BOUND and r['edge'][:, 0].max() <= go.AR_RUN_BOUND and r['info'][3] == len(g['edges'])
    # the dyadic scene: every pixel is a float32, so the input is noise-free as the device reads it
    sc = so.dyadic_scene()
    out = go.solve_positions(sc['points'], sc['cams'], go.true_rotations(sc))
    err, s = go.centre_error(out['C'], sc['poses'])
    print(f'dyadic scene: lambda0 {out["stats"][0]:.2e}, lambda1 {out["stats"][1]:.2e}, centre error {err:.2e} at scale {s:.3f}')
    assert out['info'][0] == 1 and s > 0 and err <= go.SP_RUN_BOUND and abs(out['stats'][0]) <= go.SP_RUN_BOUND * out['stats'][1]
    assert np.abs(out['X'] / s - sc['X']).max() <= go.SP_RUN_BOUND * np.abs(sc['X']).max() * 10


# ---- the fixtures of the prototype ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', go.SHAPES)
def test_prototype_fixtures(shape):
    V, N = shape
    g = go.graph_fixture(V, N)
    r = go.average_rotations(g['R_rel'], g['edges'], V)
    res = r['edge'][:, 0]
    assert not (np.abs(res / (3 * go.DEG) - 1) < 0.1).any()                          # no residual within 10 % of edge_thresh
    assert np.array_equal(r['edge'][:, 3] == 0, g['planted'])                        # every planted edge flagged and no clean one
    tree, avg = go.rotation_error_deg(r['tree'], g['truth']), go.rotation_error_deg(r['R'], g['truth'])
    crossed = bool(g['planted'][r['parent'][r['parent'] >= 0]].any())                 # the tree itself took a planted edge
    assert crossed == (tree > 5.0)                                                   # (a planted edge is ~20 degrees per axis)
    print(f'{shape}: planted {int(g["planted"].sum())}, tree {tree:.2f} degrees off, averaged {avg:.2f}')
    assert avg < 2.0 and (not crossed or avg < tree)
    if V == 32:
        assert crossed
    fx = go.position_fixture(V, N)
    trace = []
    out = go.solve_positions(fx['points'], fx['cams'], fx['R'], visible=fx['visible'], trace=trace)
    assert min(t['margin'] for t in trace) >= 0.1                                    # no angle within 10 % of its threshold
    assert trace[-1]['lam1'] >= 10 * trace[-1]['lam0'] > 0
    assert np.array_equal(trace[1]['used'], trace[2]['used']) and out['info'][7] == 3
    hidden = fx['hidden'] & fx['visible']
    if hidden.sum() >= 10:                                                           # most of the undetected outliers leave the set
        assert out['used'][hidden].mean() <= 0.3, out['used'][hidden].mean()
    err, s = go.centre_error(out['C'], fx['sc']['poses'])
    assert s > 0 and err / s < 0.03, (err, s)                                        # of a baseline of 0.6
    # with the averaged rotations in place of the true ones
    fa = go.position_fixture(V, N, R=r['R'])
    oa = go.solve_positions(fa['points'], fa['cams'], fa['R'], visible=fa['visible'])
    erra, sa = go.centre_error(oa['C'], fx['sc']['poses'])
    print(f'{shape}: centre error {err / s:.4f} with the true rotations, {erra / sa:.4f} with the averaged ones')
    assert oa['info'][0] == 1 and erra / sa < 0.15


# ---- degenerate and edge input --------------------------------------------------------------------------------------------
def test_rotation_edge_cases():
    g = go.random_graph(5, 20)
    r = go.average_rotations(g['R_rel'], g['edges'], 5, weights=g['weights'], found=g['found'])
    assert not r['edge'][g['dead'], 2].any() and r['info'][2] == 13 and np.isnan(r['edge'][g['dead'], 0]).all()
    tree = go.average_rotations(g['R_rel'], g['edges'], 5, weights=g['weights'], found=g['found'], iters=0)
    assert np.array_equal(tree['R'], tree['tree']) and tree['info'][4] == 0 and np.array_equal(tree['tree'], r['tree'])
    one = go.average_rotations(g['R_rel'][:1], g['edges'][:1], 2)
    assert list(one['info'][:6]) == [1, 2, 1, 1, 12, 0] and go.rel(one['R'][1], g['R_rel'][0]) < 1e-15 and one['edge'][0, 0] < 1e-15
    # a view joined by no live edge, and a graph with none at all
    part = go.average_rotations(g['R_rel'][:3], g['edges'][:3], 5)
    assert list(part['view_info'][:, 0]) == [1, 1, 1, 1, 0] and list(part['view_info'][:, 1]) == [0, 1, 2, 3, -1] and np.isnan(part['R'][4]).all()
    none = go.average_rotations(g['R_rel'][:3], g['edges'][:3], 5, found=np.zeros(3))
    assert list(none['info']) == [0, 1, 0, 0, 0, 1, 0, 0]
    # a refused pivot: the rotations and the weights are those of the last step taken
    s = go.singular_graph()
    stop = go.average_rotations(s['R_rel'], s['edges'], 3, weights=s['weights'])
    assert list(stop['info']) == [0, 3, 3, 1, 2, 2, 0, 0]
    two = go.average_rotations(s['R_rel'], s['edges'], 3, weights=s['weights'], iters=2)
    assert two['info'][5] == 0 and np.array_equal(two['R'], stop['R']) and np.array_equal(two['edge'], stop['edge'])
    assert (stop['edge'][:2, 1] < s['weights'][:2]).all()
    # duplicates and reversed pairs each count
    both = go.average_rotations(np.stack([g['R_rel'][0], g['R_rel'][0].T, g['R_rel'][0]]), np.array([(0, 1), (1, 0), (0, 1)]), 2)
    assert list(both['view_info'][1]) == [1, 1, 3, 3] and both['edge'][:, 0].max() < 1e-15


def test_position_edge_cases():
    fx = go.position_fixture(5, 257)
    args = (fx['points'], fx['cams'], fx['R'])
    zero = go.solve_positions(*args, found=0)
    assert all(not zero[k].any() for k in zero)
    vis = fx['visible'].copy()
    vis[3, 5:] = False                                                               # starved below min_obs
    out = go.solve_positions(*args, visible=vis)
    assert out['info'][0] == 1 and out['info'][2] == 4 and out['info'][3] == 1 and np.isnan(out['C'][3]).all() and not out['used'][3].any()
    # tracks that leave views 3 and 4 untied to the root: ok is 1, lambda1 is as small as lambda0
    vis = fx['visible'].copy()
    vis[:3, 128:], vis[3:, :128] = False, False
    full = go.solve_positions(*args, visible=fx['visible'], rounds=1)
    out = go.solve_positions(*args, visible=vis, rounds=1)
    assert out['info'][0] == 1 and abs(out['stats'][1]) < 1e-6 * full['stats'][1]
    # two views: the baseline direction
    sc = so.scene(2, 64, seed=264)
    two = go.solve_positions(sc['points'], sc['cams'], go.true_rotations(sc))
    c_true = -(go.true_rotations(sc)[1].T @ sc['poses'][1].reshape(3, 4)[:, 3])
    assert two['info'][0] == 1 and abs(np.linalg.norm(two['C'][1]) - 1) < 1e-12 and two['C'][1] @ c_true / np.linalg.norm(c_true) > 0.999
    # NaN and infinite entries
    pts, R = fx['points'].copy(), fx['R'].copy()
    pts[2, 3, 0], pts[2, 4, 1], pts[0, 5] = np.nan, np.inf, -np.inf
    R[4, 1, 1] = np.inf
    out = go.solve_positions(pts, fx['cams'], R, visible=fx['visible'])
    assert out['info'][0] == 1 and not out['used'][2, [3, 4]].any() and not out['used'][0, 5] and not out['used'][4].any() and np.isnan(out['C'][4]).all()
    assert np.isfinite(out['C'][:4]).all() and out['info'][3] == 0
    bad = R.copy()
    bad[0, 0, 0] = np.nan                                                            # the root itself is not valid: as found = 0
    assert not go.solve_positions(pts, fx['cams'], bad)['info'].any()


# ---- argument errors ------------------------------------------------------------------------------------------------------
def test_abi_argument_errors():
    lib = _lib.load_library()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)

    def rot(n=3, E=3, root=0, iters=12, s0=0.5, s1=0.01, thr=0.05, R_rel=p, out=p):
        return lib.cotr_average_rotations(R_rel, p, None, None, n, E, root, iters, s0, s1, thr, out, p, p, p, p, None)
    for kw, msg in ((dict(n=1), 'n must be in [2, 32]'), (dict(n=33), 'n must be'), (dict(E=0), 'E must be in [1, n (n - 1)]'), (dict(E=7), 'E must be'),
                    (dict(root=3), 'root'), (dict(root=-1), 'root'), (dict(iters=-1), 'iters'), (dict(iters=65), 'iters'), (dict(s1=0.0), 'sigma_end'),
                    (dict(s0=0.001), 'sigma0'), (dict(s0=float('inf')), 'finite'), (dict(s0=float('nan')), 'sigma'), (dict(thr=0.0), 'edge_thresh'),
                    (dict(thr=float('inf')), 'edge_thresh'), (dict(R_rel=None), 'must not be NULL'), (dict(out=None), 'must not be NULL'),
                    (dict(out=odd), 'aligned')):
        assert rot(**kw) == -1 and msg in lib.cotr_raster_last_error().decode(), kw
    count = ctypes.c_size_t()
    assert lib.cotr_solve_positions_work_doubles(2, 1, ctypes.byref(count)) == 0 and count.value == 32 * 24 + 64 + 144 + 96 + 6 + 1 + 3 * 16
    assert lib.cotr_solve_positions_work_doubles(32, 2049, ctypes.byref(count)) == 0 and count.value == 1072 + 2049 * 6 + 9 + 528 * 2 * 16
    for V, n in ((1, 5), (33, 5), (3, 0), (3, (1 << 20) + 1)):
        assert lib.cotr_solve_positions_work_doubles(V, n, ctypes.byref(count)) == -1
    assert lib.cotr_solve_positions_work_doubles(3, 5, None) == -1

    def pos(V=3, n=5, root=0, thr=4.0, rounds=3, min_obs=8, power=16, points=p, work=p):
        return lib.cotr_solve_positions(points, None, p, p, None, V, n, None, root, thr, rounds, min_obs, power, p, p, p, p, p, p, work, None)
    for kw, msg in ((dict(V=1), 'V must be in [2, 32]'), (dict(V=33), 'V must be'), (dict(n=0), 'n must be in [1, 2^20]'), (dict(n=(1 << 20) + 1), 'n must be'),
                    (dict(root=3), 'root'), (dict(thr=0.0), 'threshold'), (dict(thr=float('nan')), 'threshold'), (dict(rounds=0), 'rounds'),
                    (dict(rounds=9), 'rounds'), (dict(min_obs=0), 'min_obs'), (dict(power=0), 'power_iters'), (dict(power=65), 'power_iters'),
                    (dict(points=None), 'must not be NULL'), (dict(work=None), 'must not be NULL'), (dict(points=ctypes.c_void_p(p.value + 8)), '16-byte'),
                    (dict(work=odd), 'aligned')):
        assert pos(**kw) == -1 and msg in lib.cotr_raster_last_error().decode(), kw


def test_wrapper_argument_errors():
    R_rel, edges = np.stack([np.eye(3)] * 3), np.array([(0, 1), (1, 2), (0, 2)])
    ar = global_pose.average_rotations
    for args, kw, msg in (((R_rel[:, :2], edges, 3), {}, r'R_rel must be'), ((R_rel, edges[:2], 3), {}, 'edges must be'), ((R_rel, torch.from_numpy(edges.astype(np.float64)), 3), {}, 'edges must be'),
                          ((R_rel, edges, 3), dict(weights=np.ones(2)), 'weights must be'), ((R_rel, edges, 3), dict(found=np.ones(2)), 'found must be'),
                          ((R_rel, edges, 3), dict(found=[1, 1]), 'found must be'),
                          ((R_rel, edges, 1), {}, 'n must be'), ((R_rel, edges, 33), {}, 'n must be'), ((R_rel[:1].repeat(7, 0), edges[:1].repeat(7, 0), 3), {}, 'edges'),
                          ((R_rel, edges, 3), dict(root=3), 'root'), ((R_rel, edges, 3), dict(iters=65), 'iters'), ((R_rel, edges, 3), dict(iters=1.5), 'iters'),
                          ((R_rel, edges, 3), dict(sigma_end=0), 'sigma_end'), ((R_rel, edges, 3), dict(sigma0=1e-3), 'sigma0'),
                          ((R_rel, edges, 3), dict(edge_thresh=np.inf), 'edge_thresh')):
        with pytest.raises(ValueError, match=msg):
            ar(*args, **kw)
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        ar(torch.from_numpy(R_rel), edges, 3)
    pts, cams, R = np.zeros((3, 9, 2)), np.tile([500.0, 500, 320, 240, 0], (3, 1)), np.stack([np.eye(3)] * 3)
    sp = global_pose.solve_positions
    for args, kw, msg in (((pts[:, :, :1], cams, R), {}, 'points must be'), ((pts[:1], cams[:1], R[:1]), {}, 'between 2 and 32 views'), ((pts, cams[:2], R), {}, 'cameras must be'),
                          ((pts, cams, R[:2]), {}, 'R must be'), ((pts, cams, R), dict(visible=np.ones((3, 8))), 'visible must be'),
                          ((pts, cams, R), dict(located=np.ones(2)), 'located must be'), ((pts, cams, R), dict(located=[1, 1]), 'located must be'), ((pts, cams, R), dict(root=3), 'root'), ((pts, cams, R), dict(threshold=0), 'threshold'),
                          ((pts, cams, R), dict(rounds=0), 'rounds'), ((pts, cams, R), dict(rounds=9), 'rounds'), ((pts, cams, R), dict(min_obs=0), 'min_obs'),
                          ((pts, cams, R), dict(power_iters=0), 'power_iters'), ((pts, cams, R), dict(power_iters=65), 'power_iters'),
                          ((np.zeros((2, (1 << 20) + 1, 2)), cams[:2], R[:2]), {}, '2\\^20')):
        with pytest.raises(ValueError, match=msg):
            sp(*args, **kw)
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        sp(torch.from_numpy(pts), cams, R)
    good = (0, [1], np.zeros((2, 9, 2)))
    rv = structure.reconstruct_views_tensors
    for blocks, kw, msg in (([], {}, 'at least one block'), ([(0, [1])], {}, 'a block must be'), ([5], {}, 'a block must be'), ([(0, 1, np.zeros((2, 9, 2)))], {}, 'a block must be'), ([(0, [1], np.zeros((3, 9, 2)))], {}, 'points of a block'), ([(0, [], np.zeros((1, 9, 2)))], {}, 'points of a block'),
                            ([(0, [1], np.zeros((2, 4, 2)))], {}, 'at least 5'), ([(0, [0], np.zeros((2, 9, 2)))], {}, 'distinct other views'),
                            ([(0, [3], np.zeros((2, 9, 2)))], {}, 'distinct other views'), ([(3, [1], np.zeros((2, 9, 2)))], {}, 'distinct other views'),
                            ([good], dict(bundle_rounds=-1), 'bundle_rounds'), ([good], dict(root=3), 'root'), ([good] * 7, {}, 'view pairs')):
        with pytest.raises(ValueError, match=msg):
            rv(blocks, cams, 3, **kw)
    with pytest.raises(ValueError, match='V must be'):
        rv([good], cams, 33)
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        rv([(0, [1], torch.zeros((2, 9, 2)))], cams, 3)


# ---- the drivers' host logic ----------------------------------------------------------------------------------------------
def test_zoom_engine_reconstruct_views_host_logic(monkeypatch):
    calls, got = [], {}

    def fake(blocks, Ks, V, **kw):
        got.update(blocks=blocks, Ks=Ks, V=V, kw=kw)
        return 'result'
    monkeypatch.setattr(structure, 'reconstruct_views_tensors', fake)

    class Spy(ZoomEngine):
        def __init__(self):
            pass

        def cotr_corr_multiscale(self, img_a, img_b, zoom_ins=(1.0,), converge_iters=1, max_corrs=1000, queries_a=None, force=False, **kw):
            calls.append((int(img_a[0, 0, 0]), int(img_b[0, 0, 0]), force, max_corrs, len(zoom_ins), converge_iters))
            return np.concatenate([queries_a, queries_a + 10 * img_b[0, 0, 0]], axis=1)
    imgs = [np.full((48, 64, 3), v, np.uint8) for v in range(5)]
    K = np.array([[50.0, 0, 32], [0, 50, 24], [0, 0, 1]])
    assert Spy().reconstruct_views(imgs, K, span=1, grid=4, bundle_rounds=3, root=2) == 'result'
    assert [c[:2] for c in calls] == [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2), (3, 4), (4, 3)] and all(c[2:] == (True, 16, 4, 1) for c in calls)
    assert got['V'] == 5 and got['Ks'] is K and got['kw'] == dict(bundle_rounds=3, root=2) and [(a, n) for a, n, _ in got['blocks']] == [
        (0, [1]), (1, [0, 2]), (2, [1, 3]), (3, [2, 4]), (4, [3])]
    pts = got['blocks'][1][2]
    assert pts.shape == (3, 16, 2) and np.array_equal(pts[0, 0], [8.0, 6.0]) and np.array_equal(pts[0, 5], [24.0, 18.0]) and np.array_equal(pts[2], pts[0] + 20)
    del calls[:]
    q = np.arange(12.0).reshape(6, 2)
    Spy().reconstruct_views(imgs, K, span=2, anchors=[0, 4], queries=q, zoom_ins=(1.0, 0.5), converge_iters=2)
    assert [c[:2] for c in calls] == [(0, 1), (0, 2), (4, 2), (4, 3)] and all(c[2:] == (True, 6, 2, 2) for c in calls)
    assert [(a, n) for a, n, _ in got['blocks']] == [(0, [1, 2]), (4, [2, 3])] and np.array_equal(got['blocks'][1][2][0], q)
    for kw, msg in ((dict(span=0), 'span'), (dict(anchors=[5]), 'anchors'), (dict(anchors=[]), 'anchors'), (dict(anchors=[0, 1], queries=[q]), 'one set per anchor')):
        with pytest.raises(ValueError, match=msg):
            Spy().reconstruct_views(imgs, K, **kw)
    with pytest.raises(ValueError, match='between 2 and 32 images'):
        Spy().reconstruct_views(imgs[:1], K)


def test_reconstruct_views_tensors_host_logic(monkeypatch):
    """the device calls replaced: what each is handed"""
    from cotr_amd.inference import bundle, essential
    log = []
    P0 = torch.eye(3, 4, dtype=torch.float64).repeat(3, 1, 1)
    dev = torch.device('cpu')
    monkeypatch.setattr(structure._args, 'device', lambda d: dev)
    monkeypatch.setattr(torch.cuda, 'device', lambda d: __import__('contextlib').nullcontext())

    def fake_pose(p1, p2, K1, K2, device=None, **kw):
        log.append(('pose', float(K1[0, 0]), float(K2[0, 0]), kw))
        mask = torch.arange(p1.shape[0]) % 2 == 0
        return dict(R=torch.eye(3, dtype=torch.float64) * len(log), mask=mask, info=torch.tensor([1, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32))

    def fake_rot(R_rel, e, n, **kw):
        log.append(('rot', R_rel, e, n, kw))
        return dict(R='R', located='located', info='rot_info')

    def fake_pos(points, cams, R, **kw):
        log.append(('pos', points, cams, R, kw))
        return dict(poses=P0, used='used', info='pos_info')

    def fake_tri(points, cams, poses, **kw):
        log.append(('tri', poses, kw))
        return dict(X='X', used=torch.ones((3, 12), dtype=torch.bool), mask=torch.ones(12, dtype=torch.bool), info='tri_info')

    def fake_ba(points, cams, poses, X, **kw):
        log.append(('ba', poses, X, kw))
        return dict(poses=torch.eye(3, 4, dtype=torch.float64).repeat(3, 1, 1), X='Xb')
    monkeypatch.setattr(essential, 'relative_pose_tensors', fake_pose)
    monkeypatch.setattr(global_pose, 'average_rotations', fake_rot)
    monkeypatch.setattr(global_pose, 'solve_positions', fake_pos)
    monkeypatch.setattr(structure, 'triangulate_views', fake_tri)
    monkeypatch.setattr(bundle, 'bundle_adjust_tensors', fake_ba)
    monkeypatch.setattr(structure._args, 'no_cpu_tensors', lambda *a: None)
    cams = np.array([[500.0, 500, 320, 240, 0], [510.0, 510, 320, 240, 0], [520.0, 520, 320, 240, 0]])
    b0, b1 = np.arange(36.0).reshape(3, 6, 2), 100 + np.arange(24.0).reshape(2, 6, 2)
    r = structure.reconstruct_views_tensors([(0, [1, 2], b0), (2, [1], b1)], cams, 3, root=0, pose_kw=dict(seed=5), rotation_kw=dict(iters=3),
                                            position_kw=dict(rounds=2), bundle_rounds=2, threshold=3.0, min_angle=2.0)
    kinds = [entry[0] for entry in log]
    assert kinds == ['pose', 'pose', 'pose', 'rot', 'pos', 'tri', 'ba']
    assert [entry[1:3] for entry in log[:3]] == [(500.0, 510.0), (500.0, 520.0), (520.0, 510.0)] and all(entry[3] == dict(refine_rounds=4, seed=5) for entry in log[:3])
    _, R_rel, e, n, kw = log[3]
    assert n == 3 and e.tolist() == [[0, 1], [0, 2], [2, 1]] and [float(m[0, 0]) for m in R_rel] == [1.0, 2.0, 3.0]
    assert kw['weights'].tolist() == [3.0, 3.0, 3.0] and kw['found'].tolist() == [1, 1, 1] and kw['root'] == 0 and kw['iters'] == 3
    _, points, _, R, kw = log[4]
    assert R == 'R' and kw['located'] == 'located' and kw['found'] == 'rot_info' and kw['rounds'] == 2 and tuple(points.shape) == (3, 12, 2)
    assert np.array_equal(points[0, :6].numpy(), b0[0]) and np.array_equal(points[1, :6].numpy(), b0[1]) and np.array_equal(points[2, 6:].numpy(), b1[0])
    assert torch.isnan(points[0, 6:]).all() and np.array_equal(points[1, 6:].numpy(), b1[1])
    even = [True, False, True, False, True, False]
    assert kw['visible'].tolist() == [even + [False] * 6, even + even, even + even]
    assert log[5][1] is P0 and log[5][2]['visible'] == 'used' and log[5][2]['found'] == 'pos_info' and log[5][2]['threshold'] == 3.0 and log[5][2]['min_angle'] == 2.0
    assert log[6][1] is P0 and log[6][2] == 'X' and log[6][3]['fixed_views'] == (0,) and log[6][3]['rounds'] == 2 and log[6][3]['found'] == 'tri_info'
    assert log[6][3]['threshold'] == 3.0 and 'min_angle' not in log[6][3]
    assert r['X'] == 'Xb' and r['located'] == 'located' and np.array_equal(r['c2w'].numpy(), np.tile(np.eye(4), (3, 1, 1))) and len(r['pairs']) == 3
    del log[:]
    r = structure.reconstruct_views_tensors([(0, [1, 2], b0)], cams, 3, bundle_rounds=0)
    assert [entry[0] for entry in log] == ['pose', 'pose', 'rot', 'pos', 'tri'] and 'bundle' not in r and r['X'] == 'X'
