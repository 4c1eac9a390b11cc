"""numpy restatement of the guided-matching rules of DESIGN.md 3h (cotr_amd/csrc/guided.hip): nearest keypoint and the
mutual check, the RANSAC sampler, the 7-point solver, the symmetric epipolar error and count, OpenCV's iteration update and
the sequential selection.  numpy only (the GPU machine may not have scipy).  Test infrastructure."""
import math

import numpy as np

from tests import ransac_oracle as ro
from tests.ransac_oracle import DBL_EPSILON, DBL_MIN, M64, MAX_DRAWS, RANK_TOL, f32, splitmix64, update  # noqa: F401

MODEL = 7
SLOTS = 3


# ---- nearest keypoint and the mutual check ------------------------------------------------------------------------------
def distances(q, k):
    """scipy.spatial.distance_matrix(q, k) as it computes it: sqrt(dx*dx + dy*dy), dx = k.x - q.x, in float64"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    dx = k[None, :, 0] - q[:, None, 0]
    dy = k[None, :, 1] - q[:, None, 1]
    return np.sqrt(dx * dx + dy * dy)


def nearest(q, k, rows=512):
    """argmin_j d(q_i, k_j), first index on ties, NaN smallest (np.argmin), in row blocks to bound memory"""
    q = np.asarray(q, np.float64)
    out = np.empty(len(q), np.int64)
    for r in range(0, len(q), rows):
        out[r:r + rows] = np.argmin(distances(q[r:r + rows], k), axis=1)
    return out


def mutual(idx_ab, idx_ba):
    """the vectorised mutual rule: mutual[i] = idx_ba[idx_ab[i]] == i"""
    idx_ab, idx_ba = np.asarray(idx_ab), np.asarray(idx_ba)
    return idx_ba[idx_ab] == np.arange(len(idx_ab))


def demo_double_loop(idx_ab, idx_ba):
    """demo_guided_matching.py:52-63 transcribed: the matches the double loop keeps, in its order"""
    matched_a_b = np.stack([np.arange(len(idx_ab)), idx_ab]).T
    matched_b_a = np.stack([np.arange(len(idx_ba)), idx_ba]).T
    final_matches = []
    for m_ab in matched_a_b:
        for m_ba in matched_b_a:
            if (m_ab == m_ba[::-1]).all():
                final_matches.append(m_ab)
                break
    return np.array(final_matches, dtype=np.int64).reshape(-1, 2)


# ---- sampler --------------------------------------------------------------------------------------------------------------
def samples(n, max_iters, seed):
    """[max_iters, 7] int64: the first 7 distinct indices of the 64 draws of every iteration, -1 past them"""
    return ro.samples(n, max_iters, seed, MODEL)


# ---- 7-point solver -------------------------------------------------------------------------------------------------------
def _det3(m):
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])


def cubic_roots(c3, c2, c1, c0):
    """real roots of c3 l^3 + c2 l^2 + c1 l + c0, ascending (the same case split and formulas as the device)"""
    r = []
    if c3 == 0.0:
        if c2 == 0.0:
            if c1 != 0.0:
                r = [-c0 / c1]
        else:
            disc = c1 * c1 - 4.0 * c2 * c0
            if disc == 0.0:
                r = [-c1 / (2.0 * c2)]
            elif disc > 0.0:
                q = -0.5 * (c1 + math.copysign(math.sqrt(disc), c1))
                r = [q / c2, c0 / q]
    else:
        with np.errstate(all='ignore'):
            a, b, c = np.float64(c2) / c3, np.float64(c1) / c3, np.float64(c0) / c3
            Q = (a * a - 3.0 * b) / 9.0
            R = (2.0 * a * a * a - 9.0 * a * b + 27.0 * c) / 54.0
            Q3 = Q * Q * Q
            if R * R < Q3:
                th = np.arccos(R / np.sqrt(Q3))
                m = -2.0 * np.sqrt(Q)
                r = [m * np.cos(th / 3.0) - a / 3.0, m * np.cos((th + 2.0 * np.pi) / 3.0) - a / 3.0,
                     m * np.cos((th - 2.0 * np.pi) / 3.0) - a / 3.0]
            else:
                A = -np.copysign(np.cbrt(abs(R) + np.sqrt(R * R - Q3)), R)
                B = 0.0 if A == 0.0 else Q / A
                r = [(A + B) - a / 3.0]
    return sorted(float(x) for x in r)


def _normalise(x, y):
    cx, cy = x.sum() / MODEL, y.sum() / MODEL
    m = np.sqrt((x - cx) ** 2 + (y - cy) ** 2).sum() / MODEL
    return cx, cy, m


def seven_point(p1, p2):
    """p1, p2 [7,2] (already rounded to float32) -> the list of candidate F's [9] (p2^T F p1 = 0), by the rule of DESIGN.md
    3h; the null space from np.linalg.svd of the Hartley-normalised 7x9 system.  [] for a degenerate sample."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    c1x, c1y, m1 = _normalise(p1[:, 0], p1[:, 1])
    c2x, c2y, m2 = _normalise(p2[:, 0], p2[:, 1])
    if not (0.0 < m1 < np.inf and 0.0 < m2 < np.inf):
        return []
    s1, s2 = np.sqrt(2.0) / m1, np.sqrt(2.0) / m2
    u1, v1 = (p1[:, 0] - c1x) * s1, (p1[:, 1] - c1y) * s1
    u2, v2 = (p2[:, 0] - c2x) * s2, (p2[:, 1] - c2y) * s2
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones(MODEL)], axis=1)
    _, sv, vt = np.linalg.svd(A)
    if not sv[MODEL - 1] > RANK_TOL * sv[0]:
        return []
    f1, f2 = vt[7], vt[8]
    pen = lambda l: l * f1 + (1.0 - l) * f2   # noqa: E731
    D0, D1, Dm, D2 = _det3(f2), _det3(f1), _det3(pen(-1.0)), _det3(pen(2.0))
    c0 = D0
    c2 = 0.5 * (D1 + Dm) - D0
    o = 0.5 * (D1 - Dm)
    c3 = (D2 - D0 - 4.0 * c2 - 2.0 * o) / 6.0
    c1 = o - c3
    T1 = np.array([[s1, 0, -s1 * c1x], [0, s1, -s1 * c1y], [0, 0, 1.0]])
    T2 = np.array([[s2, 0, -s2 * c2x], [0, s2, -s2 * c2y], [0, 0, 1.0]])
    out = []
    for l in cubic_roots(c3, c2, c1, c0):
        with np.errstate(all='ignore'):
            F = (T2.T @ pen(l).reshape(3, 3) @ T1).reshape(9)
            F = F / np.sqrt((F * F).sum())
            if abs(F[8]) > DBL_EPSILON:
                F = np.concatenate([F[:8] / F[8], [1.0]])
            elif F[np.argmax(np.abs(F))] < 0:
                F = -F
        out.append(F)
    return out


def candidates(pts1, pts2, smp):
    """slot table [3 * iters, 9] (NaN where a slot has no candidate) for the samples ``smp`` [iters, 7]"""
    p1, p2 = f32(pts1), f32(pts2)
    H = np.full((3 * len(smp), 9), np.nan)
    for it, s in enumerate(smp):
        if (s < 0).any():
            continue
        for k, F in enumerate(seven_point(p1[s], p2[s])):
            H[3 * it + k] = F
    return H


# ---- error, count ---------------------------------------------------------------------------------------------------------
def errors(F, pts1, pts2):
    """float32 [H, n] symmetric epipolar errors of the candidates F [H, 9], in the device's operation order"""
    F = np.asarray(F, np.float64).reshape(-1, 9)
    p1, p2 = f32(pts1), f32(pts2)
    x, y, u, v = p1[None, :, 0], p1[None, :, 1], p2[None, :, 0], p2[None, :, 1]
    f = [F[:, i:i + 1] for i in range(9)]
    with np.errstate(all='ignore'):
        a = f[0] * x + f[1] * y + f[2]
        b = f[3] * x + f[4] * y + f[5]
        c = f[6] * x + f[7] * y + f[8]
        d2 = u * a + v * b + c
        e2 = d2 * d2 / (a * a + b * b)
        at = f[0] * u + f[3] * v + f[6]
        bt = f[1] * u + f[4] * v + f[7]
        ct = f[2] * u + f[5] * v + f[8]
        d1 = x * at + y * bt + ct
        e1 = d1 * d1 / (at * at + bt * bt)
        return np.where(e1 < e2, e2, e1).astype(np.float32)


def inliers(F, pts1, pts2, threshold):
    return errors(F, pts1, pts2) <= np.float32(threshold * threshold)


def counts(H, pts1, pts2, threshold, rows=256):
    """inlier counts of the slot table H [S, 9]: -1 for an empty (all-NaN) slot, 0 for any other non-finite candidate"""
    H = np.asarray(H, np.float64)
    return ro.counts(H, ~np.isnan(H).all(axis=1), lambda F: inliers(F, pts1, pts2, threshold), rows)


# ---- selection (the iteration update is ransac_oracle's) ------------------------------------------------------------------
def select_sequential(cnt, max_iters, n, confidence):
    """the FM_RANSAC loop written out: -> (found, best, iterations run, chosen slot)"""
    return ro.select_sequential(cnt, max_iters, n, confidence, MODEL, SLOTS)


def select(cnt, max_iters, n, confidence):
    """the same rule as the device replays it: jump to the next slot that beats max(best, 6) within the iterations left"""
    return ro.select(cnt, max_iters, n, confidence, MODEL, SLOTS)


def ransac(pts1, pts2, threshold, confidence, max_iters, seed):
    """the whole rule -> dict(samples, hyp_F, hyp_count, info, F, mask)"""
    n = len(pts1)
    smp = samples(n, max_iters, seed)
    H = candidates(pts1, pts2, smp)
    cnt = counts(H, pts1, pts2, threshold)
    info = select(cnt, max_iters, n, confidence)
    F = H[info[3]] if info[0] else np.zeros(9)
    mask = inliers(F, pts1, pts2, threshold)[0] if info[0] else np.zeros(n, bool)
    return dict(samples=smp, hyp_F=H, hyp_count=cnt, info=np.array(info), F=F, mask=mask)


# ---- synthetic two-view scene -----------------------------------------------------------------------------------------
def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def two_view_scene(n, outlier_frac, seed, noise=0.5, size=(640, 480)):
    """n correspondences between two pinhole cameras looking at points at depths 4-12 (non-planar): a fraction of them
    replaced by uniform outliers, 0.5 px Gaussian noise on the rest -> (pts1 [n,2], pts2 [n,2], true inlier mask [n],
    F_true [3,3] with p2^T F p1 = 0)"""
    rng = np.random.default_rng(seed)
    W, H = size
    K = np.array([[500.0, 0, W / 2], [0, 500.0, H / 2], [0, 0, 1]])
    R = _rot(*rng.uniform(-0.1, 0.1, 3))
    t = np.array([1.0, rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1)])
    z = rng.uniform(4, 12, n)
    X = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.45, 0.45, n) * z, z], axis=1)
    x1 = X @ K.T
    x2 = (X @ R.T + t) @ K.T
    p1, p2 = x1[:, :2] / x1[:, 2:], x2[:, :2] / x2[:, 2:]
    p1 = p1 + rng.normal(0, noise, p1.shape)
    p2 = p2 + rng.normal(0, noise, p2.shape)
    out = rng.random(n) < outlier_frac
    p2[out] = rng.uniform([0, 0], [W, H], (int(out.sum()), 2))
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Kinv = np.linalg.inv(K)
    F = Kinv.T @ tx @ R @ Kinv
    return p1, p2, ~out, F / F[2, 2]


# ---- the edge cases the tests use -----------------------------------------------------------------------------------------
# (n, outlier share, threshold, confidence, max_iters, seed = scene seed): the wavefront, chunk (2048 points) and
# solve-workgroup (64 iterations) edges, n and max_iters paired as homography_oracle.EDGES pairs them, from the 15 points the
# estimator starts at.  Seeds chosen on the CPU so that the restatement finds a model wherever max_iters >= 63
# (tests/test_guided_cpu.py checks it).
EDGES = [(15, 0.0, 3.0, 0.99, 1, 0), (15, 0.0, 3.0, 0.99, 63, 0), (63, 0.3, 3.0, 0.99, 64, 0), (65, 0.3, 3.0, 0.99, 65, 0),
         (2047, 0.4, 3.0, 0.99, 63, 0), (2049, 0.4, 3.0, 0.99, 65, 0), (5000, 0.3, 3.0, 0.99, 1, 0),
         (5000, 0.3, 3.0, 0.99, 63, 0)]
