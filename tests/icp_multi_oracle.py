"""numpy float64 restatement of the joint point-to-plane ICP of N depth maps (cotr_amd/csrc/icp_multi.hip),
on top of tests/icp_oracle.py as it is: the maps and the gates of an edge are ``icp_oracle``'s (written in the device's order,
so maps and associations can be compared exactly); the relative pose of an edge, the world-frame Jacobian, the per-band sums,
the edge gate, the assembly of the joint system and the step are restated here.  The step goes another numerical route
(``np.linalg.cholesky`` and two ``np.linalg.solve`` where the device factorises the packed triangle by columns), and the sums
are added sequentially where the device adds per thread, wavefront and band.

numpy only.  Test infrastructure."""
import functools

import numpy as np

from tests import icp_oracle as io
from tests import pnp_oracle as po

BANDS = 8
ROW = 32
MIN_PAIRS = 6
PIVOT_TOL = 1e-9
MAX_DIST = 0.25


# ---- one evaluation -------------------------------------------------------------------------------------------------------
def relative(ca, cb):
    """R_ab = R_a^T R_b, t_ab = R_a^T (t_b - t_a), in the device's order"""
    Ra, ta, Rb, tb = ca[:3, :3], ca[:3, 3], cb[:3, :3], cb[:3, 3]
    R = np.array([[(Ra[0, i] * Rb[0, j] + Ra[1, i] * Rb[1, j]) + Ra[2, i] * Rb[2, j] for j in range(3)] for i in range(3)])
    d = tb - ta
    t = np.array([(Ra[0, i] * d[0] + Ra[1, i] * d[1]) + Ra[2, i] * d[2] for i in range(3)])
    return R, t


def band_rows(hs, s):
    return s * hs // BANDS, (s + 1) * hs // BANDS


def live_edges(edges, n, found=None):
    """an edge is dead when an index is out of range, a == b, a view was not found, or an earlier edge names the same pair"""
    seen, out = set(), []
    for a, b in np.asarray(edges).reshape(-1, 2):
        a, b = int(a), int(b)
        ok = 0 <= a < n and 0 <= b < n and a != b and (found is None or (found[a] != 0 and found[b] != 0))
        ok = ok and (a, b) not in seen
        if ok:
            seen.add((a, b))
        out.append(ok)
    return np.array(out, bool)


def jacobian(ca, centre, Y, na):
    """rows over the twist (w, dt) of the source view b; those of the target view a are the negative"""
    Ra, ta = ca[:3, :3], ca[:3, 3]
    N = io._rot(Ra, na)
    Yc = (io._rot(Ra, Y) + ta) - np.asarray(centre, np.float64)
    return np.stack([Yc[:, 1] * N[:, 2] - Yc[:, 2] * N[:, 1], Yc[:, 2] * N[:, 0] - Yc[:, 0] * N[:, 2], Yc[:, 0] * N[:, 1] - Yc[:, 1] * N[:, 0],
                     N[:, 0], N[:, 1], N[:, 2]], axis=1)


def evaluate_edge(maps, Ks, poses, a, b, centre, max_dist=MAX_DIST, normal_cos=0.5, stride=1, reverse=False):
    """-> dict(bands [8, 32], abs [8, 29], assoc [n_src], near [n_src], usable [n_src])"""
    R, t = relative(poses[a], poses[b])
    e = io.evaluate(maps[a], Ks[a], maps[b], R, t, max_dist, normal_cos, stride)
    X, _, _ = io.source(maps[b], stride)
    with np.errstate(all='ignore'):
        Y = io._rot(R, X) + t
        J = jacobian(poses[a], centre, Y, e['J'][:, 3:6])
        r = e['r']
        T = np.stack([J[:, i] * J[:, j] for i in range(6) for j in range(i, 6)] + [J[:, i] * r for i in range(6)] + [r * r, np.ones(len(r))], axis=1)
    T[~e['pairs']] = 0.0
    H, W = maps[b].shape[:2]
    hs, ws = -(-H // stride), -(-W // stride)
    bands, absb = np.zeros((BANDS, ROW)), np.zeros((BANDS, 29))
    for s in range(BANDS):
        r0, r1 = band_rows(hs, s)
        part = T[r0 * ws:r1 * ws]
        if len(part):
            bands[s, :29] = np.cumsum(part[::-1] if reverse else part, axis=0)[-1]
            absb[s] = np.abs(part).sum(axis=0)
        bands[s, 29] = e['usable'][r0 * ws:r1 * ws].sum()
    return dict(bands=bands, abs=absb, assoc=e['assoc'], near=e['near'], usable=e['usable'])


def evaluate(maps, Ks, poses, edges, centre, found=None, max_dist=MAX_DIST, normal_cos=0.5, stride=1, reverse=False):
    """every edge at ``poses`` -> dict(edge_out [E, 8, 32], abs [E, 8, 29], assoc [E, n_src], near [E, n_src], live [E])"""
    n = len(maps)
    H, W = maps[0].shape[:2]
    n_src = -(-H // stride) * -(-W // stride)
    edges = np.asarray(edges).reshape(-1, 2)
    live = live_edges(edges, n, found)
    out = dict(edge_out=np.zeros((len(edges), BANDS, ROW)), abs=np.zeros((len(edges), BANDS, 29)), assoc=np.full((len(edges), n_src), -1, np.int32),
               near=np.zeros((len(edges), n_src), bool), live=live)
    for i, (a, b) in enumerate(edges):
        if live[i]:
            e = evaluate_edge(maps, Ks, poses, int(a), int(b), centre, max_dist, normal_cos, stride, reverse)
            out['edge_out'][i], out['abs'][i], out['assoc'][i], out['near'][i] = e['bands'], e['abs'], e['assoc'], e['near']
    return out


# ---- one step -------------------------------------------------------------------------------------------------------------
def edge_totals(edge_out, reverse=False):
    """the bands of every edge in band order -> [E, 32]"""
    return np.cumsum(edge_out[:, ::-1] if reverse else edge_out, axis=1)[:, -1]


def system(tot, edges, kept, n, free):
    """-> (H [6F, 6F], g [6F], slots): block (v, v) the sum of A over the kept edges touching v, the other view ascending and
    (v, w) before (w, v); block (a, b) minus A of (lo, hi) and (hi, lo); the gradient -g at the target, +g at the source"""
    tab = {(int(a), int(b)): i for i, (a, b) in enumerate(edges) if kept[i]}
    slots = {v: s for s, v in enumerate(np.flatnonzero(free))}
    F = len(slots)
    H, g = np.zeros((6 * F, 6 * F)), np.zeros(6 * F)
    A = lambda e: io.normal_matrix(tot[e])   # noqa: E731
    for v, p in slots.items():
        blk, gv = np.zeros((6, 6)), np.zeros(6)
        for w in range(n):
            if (v, w) in tab:
                blk, gv = blk + A(tab[(v, w)]), gv - tot[tab[(v, w)], 21:27]
            if (w, v) in tab:
                blk, gv = blk + A(tab[(w, v)]), gv + tot[tab[(w, v)], 21:27]
        H[6 * p:6 * p + 6, 6 * p:6 * p + 6], g[6 * p:6 * p + 6] = blk, gv
    for v, p in slots.items():
        for w, q in slots.items():
            if w < v:
                x = np.zeros((6, 6))
                if (w, v) in tab:
                    x = x + A(tab[(w, v)])
                if (v, w) in tab:
                    x = x + A(tab[(v, w)])
                H[6 * p:6 * p + 6, 6 * q:6 * q + 6] = -x
                H[6 * q:6 * q + 6, 6 * p:6 * p + 6] = -x.T
    return H, g, slots


def pivot_ratio(H):
    """the smallest Cholesky pivot over its original diagonal value; 0 when the factorisation fails"""
    try:
        L = np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return 0.0, None
    with np.errstate(all='ignore'):
        ratio = float(np.min(np.diag(L) ** 2 / np.diag(H)))
    return (ratio if np.isfinite(ratio) else 0.0), L


def column_pivots(H):
    """Cholesky by columns as the device runs it -> the smallest pivot over its original diagonal value, up to and with the
    first pivot that is not positive (where np.linalg.cholesky only raises)"""
    A = np.array(H, np.float64)
    d0 = np.diag(A).copy()
    worst = np.inf
    for k in range(len(A)):
        worst = min(worst, A[k, k] / d0[k])
        if not A[k, k] > 0:
            break
        A[k:, k] = A[k:, k] / np.sqrt(A[k, k])
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k])
    return float(worst)


def solve(edge_out, edges, n, fixed=(0,), found=None, pivot_tol=PIVOT_TOL, last=False, reverse=False):
    """-> dict(reason, x {view: [6]} or None, kept [E], free [n], view_info [n, 4], pairs, err, ratio, F, H, g)"""
    edges = np.asarray(edges).reshape(-1, 2)
    tot = edge_totals(edge_out, reverse)
    kept = tot[:, 28] >= MIN_PAIRS
    vinfo = np.zeros((n, 4), np.int32)
    for i, (a, b) in enumerate(edges):
        if kept[i]:
            for v in (int(a), int(b)):
                vinfo[v, 1] += int(tot[i, 28])
                vinfo[v, 2] += 1
    free = np.array([v not in fixed and (found is None or found[v] != 0) and vinfo[v, 2] >= 1 for v in range(n)])
    vinfo[:, 0] = free
    order = np.flatnonzero(kept)[::-1] if reverse else np.flatnonzero(kept)
    pairs, err = int(tot[kept, 28].sum()), 0.0
    for i in order:
        err = err + tot[i, 27]
    out = dict(reason=0, x=None, kept=kept, free=free, view_info=vinfo, pairs=pairs, err=float(err), ratio=0.0, F=int(free.sum()), H=None, g=None)
    if out['F'] == 0 or pairs < MIN_PAIRS:
        out['reason'] = 1
        return out
    if last:
        return out
    H, g, slots = system(tot, edges, kept, n, free)
    out['H'], out['g'] = H, g
    if not (np.isfinite(H).all() and np.isfinite(g).all() and np.isfinite(err)):
        out['reason'] = 3
        return out
    ratio, L = pivot_ratio(H)
    if L is None or not ratio > pivot_tol:
        out['reason'], out['raw_ratio'] = 2, ratio
        return out
    x = np.linalg.solve(L.T, np.linalg.solve(L, g))
    out['ratio'], out['x'] = ratio, {v: x[6 * p:6 * p + 6] for v, p in slots.items()}
    return out


def twist(c2w, d, centre):
    """R <- exp([w]x) R, t <- exp([w]x) (t - c) + c + dt"""
    c = np.asarray(centre, np.float64)
    E = po.rotate(d[:3], np.eye(3))
    out = np.array(c2w, np.float64)
    out[:3, :3] = po.rotate(d[:3], c2w[:3, :3])
    out[:3, 3] = E @ (c2w[:3, 3] - c) + c + d[3:]
    return out


def apply(poses, x, centre):
    return [twist(p, -x[v], centre) if v in x else np.array(p, np.float64) for v, p in enumerate(poses)]


def multiview(maps, Ks, c2w0, edges, fixed=(0,), centre=None, found=None, max_dist=MAX_DIST, normal_cos=0.5, pivot_tol=PIVOT_TOL, iters=10,
              stride=1, reverse=False):
    """the chain -> dict(c2w [n, 4, 4], info [8], view_info [n, 4], stats [2], edge_out, hist [iters + 1, 4], assoc, near, poses: the
    poses of every evaluation run, evals, solves)"""
    n = len(maps)
    poses = [np.array(p, np.float64) for p in c2w0]
    centre = default_centre(poses) if centre is None else centre
    edges = np.asarray(edges).reshape(-1, 2)
    hist = np.zeros((iters + 1, 4))
    steps, trail, evals, solves = 0, [], [], []
    for k in range(iters + 1):
        ev = evaluate(maps, Ks, poses, edges, centre, found, max_dist, normal_cos, stride, reverse)
        so = solve(ev['edge_out'], edges, n, fixed, found, pivot_tol, k == iters, reverse)
        trail.append(poses), evals.append(ev), solves.append(so)
        hist[k] = so['err'], so['pairs'], so['ratio'], 0.0
        if so['reason'] != 0 or k == iters:
            break
        poses = apply(poses, so['x'], centre)
        steps += 1
    info = np.array([so['reason'] == 0, steps, so['pairs'], so['reason'], int(ev['live'].sum()), int(so['kept'].sum()), so['F'], 0], np.int32)
    stats = np.array([so['err'], np.sqrt(so['err'] / so['pairs']) if so['pairs'] else 0.0])
    return dict(c2w=np.stack(poses), info=info, view_info=so['view_info'], stats=stats, edge_out=ev['edge_out'], hist=hist, assoc=ev['assoc'],
                near=ev['near'], poses=trail, evals=evals, solves=solves)


def default_centre(poses):
    return np.mean([np.asarray(p)[:3, 3] for p in poses], axis=0)


def all_pairs(n):
    return np.array([(a, b) for a in range(n) for b in range(n) if a != b], np.int32)


def star(n):
    return np.array([(0, b) for b in range(1, n)], np.int32)


def ring(n):
    return np.array([(v, (v + 1) % n) for v in range(n)], np.int32)


def all_edge_rmse(maps, Ks, poses, max_dist=MAX_DIST, stride=1):
    """the rmse over every ordered pair at ``poses``: what the star, the ring and the joint result are compared by"""
    n = len(maps)
    ev = evaluate(maps, Ks, poses, all_pairs(n), default_centre(poses), max_dist=max_dist, stride=stride)
    tot = edge_totals(ev['edge_out'])
    return float(np.sqrt(tot[:, 27].sum() / tot[:, 28].sum()))


# ---- scenes ---------------------------------------------------------------------------------------------------------------
VIEW_1 = ((2.0, -4.5, 1.2), (0.5, 0.05, 0.2))
VIEW_3 = ((4.0, -9.0, 2.5), (1.2, 0.2, 0.5))
SIZES = ((3, 3), (5, 5), (7, 9), (8, 8), (9, 8), (10, 7), (16, 16), (17, 241), (32, 64), (96, 128))


def true_poses():
    (_, _, ca), (_, _, cb) = po.capture_pair(96, 128)
    return [ca, po.pose_matrix(*VIEW_1), cb, po.pose_matrix(*VIEW_3)]


def start_poses(true):
    """views 1 .. of ``true`` turned by up to a degree about each axis and shifted by up to 0.03, from RandomState(3)"""
    rs = np.random.RandomState(3)
    out = [np.array(true[0], np.float64)]
    for c in true[1:]:
        d = po.pose_matrix(rs.uniform(-1, 1, 3), (0, 0, 0))
        d[:3, 3] = rs.uniform(-0.03, 0.03, 3)
        out.append(d @ c)
    return out


@functools.lru_cache(maxsize=None)
def scene(H, W, edge=io.SWEEP_EDGE, n=4):
    """n views of the three-plane corner at H x W: the four poses of the issue, repeated with small deterministic offsets
    beyond four -> dict(depths [n, H, W], Ks [n, 3, 3], true, start: lists of c2w, maps [n, H, W, 6], centre, edge); read only"""
    (_, Ka, _), (_, Kb, _) = po.capture_pair(96, 128)
    base = true_poses()
    true = []
    for v in range(n):
        rep = v // 4
        off = po.pose_matrix((0.3 * rep, -0.2 * rep, 0.1 * rep), (0.01 * rep, -0.008 * rep, 0.006 * rep))
        true.append(off @ base[v % 4])
    Ks = np.stack([io.scaled_camera(Ka if v % 2 == 0 else Kb, H, W) for v in range(n)])
    depths = np.stack([io.render(H, W, Ks[v], true[v], io.PLANES) for v in range(n)])
    start = start_poses(true)
    maps = np.stack([io.maps(depths[v], Ks[v], edge) for v in range(n)])
    return dict(depths=depths, Ks=Ks, true=true, start=start, maps=maps, centre=default_centre(start), edge=edge)


def pose_distance(a, b):
    """the largest over the views of icp_oracle.pose_distance"""
    return max(io.pose_distance(p[:3, :3], p[:3, 3], q[:3, :3], q[:3, 3]) for p, q in zip(a, b))


# The dependence of one joint step on the order of its sums, measured on the CPU from the scene's start over every size of
# SIZES that solves, all 12 edges (tests/test_icp_multi_cpu.py measures it again): the poses after one step from the sums taken
# forwards against backwards differ by at most ORDER_NOISE in an entry of R and in t relative to its norm.  The device, which
# sums in yet another order and factorises by columns, is allowed 1000 times that.
ORDER_NOISE = 6e-15   # measured 5.0e-15 (5 x 5, the worst conditioned); <= 2.6e-15 from 7 x 9 up
STEP_BOUND = 1000 * ORDER_NOISE
# 32 views at 16 x 16: all 992 pairs stay below ORDER_NOISE (2.8e-15); the ring, a chain of 31 free views hung on one fixed view
# (smallest pivot ratio 1.4e-3), measures 1.04e-12 and has its own bound
ORDER_NOISE_RING32 = 1.2e-12
STEP_BOUND_RING32 = 1000 * ORDER_NOISE_RING32


def order_noise(sc, edges=None):
    n = len(sc['maps'])
    edges = all_pairs(n) if edges is None else edges
    out = []
    for rev in (False, True):
        ev = evaluate(sc['maps'], sc['Ks'], sc['start'], edges, sc['centre'], reverse=rev)
        so = solve(ev['edge_out'], edges, n, reverse=rev)
        assert so['reason'] == 0
        out.append(apply(sc['start'], so['x'], sc['centre']))
    return pose_distance(out[0], out[1])
