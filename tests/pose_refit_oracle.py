"""numpy restatement of the relative-pose refit of DESIGN.md 3h-5 (cotr_refine_pose in cotr_amd/csrc/essential.hip):
undamped Gauss-Newton on the Sampson error over (R, unit t), the inliers re-counted between rounds.  Every rule of the device
in its operation order; the sums are taken point by point (forwards, or backwards to measure what their order decides).  The
Jacobian comes a second time by another route, central differences of the residual along the five directions
(``jacobian_numeric``), which tests/test_pose_refit_cpu.py holds against the analytic rule.  Camera normalisation, threshold,
Sampson error, in-front rule and the scenes are those of tests/essential_oracle.py.  numpy only.  Test infrastructure."""
import functools

import numpy as np

from tests import essential_oracle as eo
from tests import ransac_oracle as ro
from tests.pnp_oracle import rotate  # noqa: F401  (exp([w]x) R by Rodrigues' formula, the rule of DESIGN.md 3h-4)

PARAMS = 5
SUMS = 22
MAX_ROUNDS = 8
MAX_REFINE = 64


def tri(i, j):
    """index of (i, j), i <= j, in the row-major upper triangle of a 5 x 5 matrix"""
    return i * 5 - i * (i - 1) // 2 + (j - i)


# ---- state ----------------------------------------------------------------------------------------------------------------
def cross_mat(v, M):
    """[v]x M, each entry a difference of two products"""
    M = np.asarray(M, np.float64).reshape(3, 3)
    return np.stack([v[1] * M[2] - v[2] * M[1], v[2] * M[0] - v[0] * M[2], v[0] * M[1] - v[1] * M[0]])


def basis(t):
    """-> (b1, b2, k): k the first index of smallest |t_k|, b1 = e_k x t normalised, b2 = t x b1"""
    k = int(np.argmin(np.abs(t)))
    c = [np.array([0.0, -t[2], t[1]]), np.array([t[2], 0.0, -t[0]]), np.array([-t[1], t[0], 0.0])][k]
    b1 = c / np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    b2 = np.array([t[1] * b1[2] - t[2] * b1[1], t[2] * b1[0] - t[0] * b1[2], t[0] * b1[1] - t[1] * b1[0]])
    return b1, b2, k


def derive(R, t):
    """-> (E = [t]x R, dE [5, 3, 3] = [t]x [e_j]x R for j = 0..2 then [b1]x R, [b2]x R, b1, b2)"""
    b1, b2, _ = basis(t)
    dE = [cross_mat(t, cross_mat(e, R)) for e in np.eye(3)] + [cross_mat(b1, R), cross_mat(b2, R)]
    return cross_mat(t, R), np.stack(dE), b1, b2


def unit(t):
    t = np.asarray(t, np.float64).reshape(3)
    return t / np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])


def step(R, t, d, b1, b2):
    """R <- exp([w]x) R, t <- (t + u b1 + v b2) / |...|"""
    return rotate(d[:3], R), unit((t + d[3] * b1) + d[4] * b2)


def unit_signed(E):
    """unit Frobenius norm (the squares added in order), the first entry of largest magnitude positive"""
    e = np.asarray(E, np.float64).reshape(9)
    ss = 0.0
    for v in e:
        ss += v * v
    e = e / np.sqrt(ss)
    return -e if e[np.argmax(np.abs(e))] < 0 else e


# ---- residual, Jacobian, sums ---------------------------------------------------------------------------------------------
def _ab(E, x1, y1, x2, y2):
    e = np.asarray(E, np.float64).reshape(9)
    a0 = e[0] * x1 + e[1] * y1 + e[2]
    a1 = e[3] * x1 + e[4] * y1 + e[5]
    a2 = e[6] * x1 + e[7] * y1 + e[8]
    b0 = e[0] * x2 + e[3] * y2 + e[6]
    b1 = e[1] * x2 + e[4] * y2 + e[7]
    return a0, a1, a2, b0, b1


def residual(E, xn1, xn2):
    """-> (r = d / sqrt(g) [m], skipped [m]: g = 0 or r not finite)"""
    x1, y1, x2, y2 = xn1[:, 0], xn1[:, 1], xn2[:, 0], xn2[:, 1]
    with np.errstate(all='ignore'):
        a0, a1, a2, b0, b1 = _ab(E, x1, y1, x2, y2)
        d = x2 * a0 + y2 * a1 + a2
        g = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1
        r = d / np.sqrt(g)
    return r, ~(g > 0.0) | ~np.isfinite(r)


def jacobian(E, dE, xn1, xn2):
    """the analytic rule -> (r [m], J [m, 5], skipped [m]): for each direction dd = x2h^T dE x1h, da = dE x1h,
    db = dE^T x2h, dg = 2 (a0 da0 + a1 da1 + b0 db0 + b1 db1), J = dd / s - d dg / (2 s g) with s = sqrt(g)"""
    x1, y1, x2, y2 = xn1[:, 0], xn1[:, 1], xn2[:, 0], xn2[:, 1]
    with np.errstate(all='ignore'):
        a0, a1, a2, b0, b1 = _ab(E, x1, y1, x2, y2)
        d = x2 * a0 + y2 * a1 + a2
        g = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1
        s = np.sqrt(g)
        r = d / s
        J = []
        for q in dE:
            da0, da1, da2, db0, db1 = _ab(q, x1, y1, x2, y2)
            dd = x2 * da0 + y2 * da1 + da2
            dg = 2.0 * (a0 * da0 + a1 * da1 + b0 * db0 + b1 * db1)
            J.append(dd / s - d * dg / (2.0 * s * g))
    return r, np.stack(J, axis=1), ~(g > 0.0) | ~np.isfinite(r)


def jacobian_numeric(R, t, xn1, xn2, h=1e-6):
    """the other route: central differences of the residual along the five parameters of ``step``"""
    _, _, b1, b2 = derive(R, t)
    J = []
    for k in range(PARAMS):
        d = np.zeros(PARAMS)
        d[k] = h
        Rp, tp = step(R, t, d, b1, b2)
        Rm, tm = step(R, t, -d, b1, b2)
        J.append((residual(cross_mat(tp, Rp), xn1, xn2)[0] - residual(cross_mat(tm, Rm), xn1, xn2)[0]) / (2.0 * h))
    return np.stack(J, axis=1)


def sums(R, t, xn1, xn2, reverse=False):
    """the 22 sums of the device at (R, t) over the points given, each added in order (reverse: in reversed order): 15 of
    J^T J, 5 of J^T r, the squared error, the points skipped (which add nothing else)"""
    if not len(xn1):
        return np.zeros(SUMS)
    E, dE, _, _ = derive(R, t)
    r, J, skip = jacobian(E, dE, xn1, xn2)
    with np.errstate(all='ignore'):
        terms = [J[:, i] * J[:, j] for i in range(PARAMS) for j in range(i, PARAMS)] + [J[:, i] * r for i in range(PARAMS)] + [r * r]
    T = np.stack(terms, axis=1)
    T[skip] = 0.0
    T = np.concatenate([T, skip[:, None].astype(np.float64)], axis=1)
    if reverse:
        T = T[::-1]
    return np.cumsum(T, axis=0)[-1]


# ---- a round, the re-count, the whole rule --------------------------------------------------------------------------------
def fit(R, t, xn1, xn2, iters, reverse=False):
    """up to ``iters`` Gauss-Newton steps from (R, t) on the points given: a step is kept only if the summed squared error
    falls; the first one not kept, a singular system or fewer than 5 points end it
    -> dict(R, t, kept, skipped, margin: the relative size of the last decision's error difference (inf: none taken),
    errs: the error at every pose accepted)"""
    kept, trial, margin, errs, skipped = 0, None, np.inf, [], 0
    for j in range(iters + 1):
        s = sums(R, t, xn1, xn2, reverse)
        err = s[20]
        if trial is not None:
            Rp, tp, ep = trial
            margin = abs(err - ep) / ep if ep > 0 else np.inf
            if err < ep:
                kept += 1
            else:
                return dict(R=Rp, t=tp, kept=kept, skipped=skipped, margin=margin, errs=errs)
        skipped = int(s[21])
        errs.append(err)
        if j == iters or len(xn1) < 5:
            break
        A = np.zeros((PARAMS, PARAMS))
        for a in range(PARAMS):
            for b in range(a, PARAMS):
                A[a, b] = A[b, a] = s[tri(a, b)]
        d = ro.solve_full_pivot(A, -s[15:20])
        if d is None:
            break
        trial = (R, t, err)
        _, _, b1, b2 = derive(R, t)
        R, t = step(R, t, d, b1, b2)
    return dict(R=R, t=t, kept=kept, skipped=skipped, margin=margin, errs=errs)


def recount(R, t, xn1, xn2, thr, dist=50.0):
    """the mask of a later round: Sampson inliers of E = [t]x R under the scaled float32 threshold, in front under (R, t)
    -> (mask, margin: how close, relative, an error comes to the threshold or a Sampson inlier's depth to 0 or to dist)"""
    E = cross_mat(t, R).reshape(1, 9)
    err = eo.errors(E, xn1, xn2)[0]
    thr2 = np.float32(thr * thr)
    near = err <= thr2
    z1, z2, det = eo.depths(R, t, xn1, xn2)
    front = eo.in_front(R, t, xn1, xn2, dist)
    with np.errstate(all='ignore'):
        m_err = np.abs(err.astype(np.float64) - float(thr2)) / float(thr2)
        z = np.concatenate([z1[near], z2[near]])
        z = z[np.isfinite(z)]
        m_z = np.minimum(np.abs(z), np.abs(z - dist) / dist)
    margin = min(float(m_err[np.isfinite(m_err)].min()) if np.isfinite(m_err).any() else np.inf, float(m_z.min()) if len(m_z) else np.inf)
    return near & front, margin


def refine(R0, t0, pts1, pts2, K1, K2=None, mask=None, threshold=1.0, dist=50.0, rounds=4, iters=10, found=1, reverse=False):
    """the whole rule of cotr_refine_pose -> dict(R [3,3], t [3], E [9], mask [n], info [8], rounds: per round dict(mask,
    R0, t0 (the pose the round started from), kept, margin, errs, recount_margin))"""
    K2 = K1 if K2 is None else K2
    n = len(pts1)
    R0, t0 = np.asarray(R0, np.float64).reshape(3, 3), np.asarray(t0, np.float64).reshape(3)
    nrm = np.sqrt((t0[0] * t0[0] + t0[1] * t0[1]) + t0[2] * t0[2]) if np.isfinite(t0).all() else np.nan
    if not found or not np.isfinite(R0).all() or not (nrm > 0.0 and nrm < np.inf):
        return dict(R=np.zeros((3, 3)), t=np.zeros(3), E=np.zeros(9), mask=np.zeros(n, bool), info=np.zeros(8, np.int64), rounds=[])
    xn1, xn2 = eo.normalise(pts1, K1), eo.normalise(pts2, K2)
    thr = eo.scaled_threshold(threshold, K1, K2)
    R, t = R0.copy(), t0 / nrm
    m = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    log, total = [], 0
    for r in range(rounds):
        rm = np.inf
        if r > 0:
            m, rm = recount(R, t, xn1, xn2, thr, dist)
        f = fit(R, t, xn1[m], xn2[m], iters, reverse)
        log.append(dict(mask=m.copy(), R0=R, t0=t, kept=f['kept'], margin=f['margin'], errs=f['errs'], recount_margin=rm))
        R, t, total = f['R'], f['t'], total + f['kept']
    info = np.array([1, int(m.sum()), rounds, total, log[-1]['kept'], f['skipped'], 0, 0])
    return dict(R=R, t=t, E=unit_signed(cross_mat(t, R)), mask=m, info=info, rounds=log)


# ---- starting poses and the scenes the tests use --------------------------------------------------------------------------
def perturbed(R, t, rot_deg, dir_deg, seed):
    """the pose turned by rot_deg about a random axis, its direction by dir_deg about a random axis perpendicular to it"""
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    R0 = rotate(ax * np.radians(rot_deg), R)
    p = np.cross(t, rng.normal(size=3))
    p /= np.linalg.norm(p)
    return R0, rotate(p * np.radians(dir_deg), np.eye(3)) @ t


# what the device tests start from: the scene's pose turned by 0.05 / 0.15 degrees (the size of a RANSAC model's error at
# 1 px: 0.05 degrees move a point by 0.7 px at a focal length of 800) and the Sampson inliers of that pose in front of it
START_ROT_DEG, START_DIR_DEG = 0.05, 0.15


@functools.lru_cache(maxsize=None)
def start(scene):
    """-> dict(p1, p2, K1, K2, R, t (the scene's), good, R0, t0, mask0, thr): read only"""
    n, outl, noise, thr, conf, iters, seed = scene
    p1, p2, K1, K2, R, t, good = eo.two_view_scene(n, outl, seed, noise)
    R0, t0 = perturbed(R, t, START_ROT_DEG, START_DIR_DEG, seed + 1000)
    mask0, _ = recount(R0, unit(t0), eo.normalise(p1, K1), eo.normalise(p2, K2), eo.scaled_threshold(thr, K1, K2))
    return dict(p1=p1, p2=p2, K1=K1, K2=K2, R=R, t=t, good=good, R0=R0, t0=t0, mask0=mask0, thr=thr)


# (n, outlier share, noise px, threshold px, -, -, scene seed), the tuple form of essential_oracle.  n: the fewest points (5,
# 6), the wavefront (63, 64, 65), the 256-thread block (255, 256, 257), the 2048-point chunk (2047, 2048, 2049) and three chunks
# (4097).  Seeds chosen on the CPU (tests/test_pose_refit_cpu.py checks it) so that, for the restatement alone, from ``start``
# with rounds = 8 and refine_iters = 10: every re-counted mask keeps a relative margin above 1e-6 from the threshold and from 0
# and the distance threshold.
SIZES = [(5, 0.0, 0.0, 1.0, 0, 0, 0), (6, 0.0, 0.5, 1.0, 0, 0, 1), (63, 0.3, 1.0, 1.0, 0, 0, 2), (64, 0.3, 1.0, 1.0, 0, 0, 3),
         (65, 0.3, 0.5, 1.0, 0, 0, 4), (255, 0.4, 1.0, 1.0, 0, 0, 5), (256, 0.0, 1.0, 1.0, 0, 0, 6), (257, 0.2, 0.5, 1.0, 0, 0, 7),
         (2047, 0.4, 1.0, 1.0, 0, 0, 8), (2048, 0.4, 0.5, 1.0, 0, 0, 9), (2049, 0.4, 1.0, 1.0, 0, 0, 10), (4097, 0.3, 1.0, 1.0, 0, 0, 11)]

# The scenes of essential_oracle on which the restatement alone, started from the restatement's own RANSAC pose and pose mask
# with rounds = 4 and refine_iters = 10, ends with both pose errors below the unrefined ones (checked on the CPU by
# tests/test_pose_refit_cpu.py; none has noise at n < 1000).
QUALITY = [eo.SCENES[2], eo.SCENES[3], eo.SCENES[4], eo.EDGES[5], eo.EDGES[6], eo.EDGES[7], eo.EDGES[9]]


@functools.lru_cache(maxsize=None)
def reference(scene, rounds=8, iters=10):
    """the restatement from ``start`` -> the dict of ``refine``; read only"""
    s = start(scene)
    return refine(s['R0'], s['t0'], s['p1'], s['p2'], s['K1'], s['K2'], s['mask0'], s['thr'], 50.0, rounds, iters)


def order_noise(scene, rounds=8, iters=10):
    """the largest difference in an entry of R or t between the restatement with its sums forwards and backwards"""
    s = start(scene)
    a = reference(scene, rounds, iters)
    b = refine(s['R0'], s['t0'], s['p1'], s['p2'], s['K1'], s['K2'], s['mask0'], s['thr'], 50.0, rounds, iters, reverse=True)
    return max(np.abs(a['R'] - b['R']).max(), np.abs(a['t'] - b['t']).max())


def sums_order_noise(scene):
    """the largest relative difference of one of the 21 float sums at ``start``, forwards against backwards, relative to the
    largest magnitude among the sums of its group (J^T J, J^T r, the error)"""
    s = start(scene)
    xn1, xn2 = eo.normalise(s['p1'], s['K1'])[s['mask0']], eo.normalise(s['p2'], s['K2'])[s['mask0']]
    a, b = sums(s['R0'], unit(s['t0']), xn1, xn2), sums(s['R0'], unit(s['t0']), xn1, xn2, reverse=True)
    return sums_distance(a, b)


def sums_distance(a, b):
    """the 22 sums compared: each float sum relative to the largest magnitude in its group; inf when the skipped counts differ"""
    if a[21] != b[21]:
        return np.inf
    worst = 0.0
    for lo, hi in ((0, 15), (15, 20), (20, 21)):
        scale = max(np.abs(a[lo:hi]).max(), np.abs(b[lo:hi]).max())
        if scale > 0:
            worst = max(worst, float(np.abs(a[lo:hi] - b[lo:hi]).max() / scale))
    return worst


# Measured on the CPU over SIZES (tests/test_pose_refit_cpu.py measures both again and holds them):
# ORDER_NOISE: the refit with its sums forwards against backwards, in an entry of R or t, rounds = 8, refine_iters = 10 - near
# the minimum the order decides whether a last marginal step is kept.  SUMS_ORDER_NOISE: one accumulation forwards against
# backwards.  The device sums in a third order and is allowed 1000 times each (the margin of DESIGN.md 3h-2 and 3h-4).
ORDER_NOISE = 5.1e-9
SUMS_ORDER_NOISE = 2.5e-15
REFIT_BOUND = 1000 * ORDER_NOISE
SUMS_BOUND = 1000 * SUMS_ORDER_NOISE
