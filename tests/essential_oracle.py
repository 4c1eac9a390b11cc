"""numpy restatement of the essential-matrix rules of DESIGN.md 3h-3 (cotr_amd/csrc/essential.hip): the camera
normalisation, the sampler (the F path's draws, model size 5), the five-point solver, the Sampson error and count, the
sequential selection over 10 slots per iteration, and the pose of an essential matrix (decomposition by cyclic Jacobi, the
four candidates, the least-squares depths, the cheirality count).  The candidates are reached by another numerical route
than the device's: the null space by np.linalg.svd, the reduced system by np.linalg.solve, the roots by np.linalg.eig of the
action matrix; then the same three polish steps.  numpy only.  Test infrastructure."""
import functools

import numpy as np

from tests import ransac_oracle as ro
from tests.ransac_oracle import JACOBI_SWEEPS, RANK_TOL, f32, jacobi, solve_full_pivot  # noqa: F401

MODEL = 5
SLOTS = 10
POLISH = 3
MAX_ITERS = 6553
# exponents (x, y, z) of the 20 columns: the ten cubic monomials, then x2 xy y2 xz yz z2 x y z 1
MON = [(3, 0, 0), (2, 1, 0), (1, 2, 0), (0, 3, 0), (2, 0, 1), (1, 1, 1), (0, 2, 1), (1, 0, 2), (0, 1, 2), (0, 0, 3),
       (2, 0, 0), (1, 1, 0), (0, 2, 0), (1, 0, 1), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_MX, _MY, _MZ = (np.array([m[i] for m in MON]) for i in range(3))


# ---- cameras and the sampler ----------------------------------------------------------------------------------------------
def normalise(pts, K):
    """pixels rounded to float32 -> normalised coordinates: y = (v - cy) / fy, then x = (u - cx - s y) / fx"""
    p, K = f32(pts), np.asarray(K, np.float64).reshape(3, 3)
    y = (p[:, 1] - K[1, 2]) / K[1, 1]
    x = (p[:, 0] - K[0, 2] - K[0, 1] * y) / K[0, 0]
    return np.stack([x, y], axis=1)


def scaled_threshold(threshold, K1, K2):
    K1, K2 = np.asarray(K1, np.float64).reshape(3, 3), np.asarray(K2, np.float64).reshape(3, 3)
    return threshold / ((K1[0, 0] + K1[1, 1] + K2[0, 0] + K2[1, 1]) / 4.0)


def samples(n, max_iters, seed):
    """[max_iters, 5] int64: the first 5 distinct indices of the F path's 64 draws of every iteration, -1 past them"""
    return ro.samples(n, max_iters, seed, MODEL)


# ---- five-point solver ----------------------------------------------------------------------------------------------------
def _lin_mul(P, l):
    """the polynomial P [4,4,4] (exponents of x, y, z) times l[0] x + l[1] y + l[2] z + l[3]"""
    out = l[3] * P
    out[1:] += l[0] * P[:-1]
    out[:, 1:] += l[1] * P[:, :-1]
    out[:, :, 1:] += l[2] * P[:, :, :-1]
    return out


def constraints(N):
    """N [4,9], E = x N0 + y N1 + z N2 + N3 -> the 10 x 20 coefficients of the nine entries of 2 E E^T E - tr(E E^T) E and of
    det E in the monomials MON"""
    L = N.T.reshape(3, 3, 4)                                    # L[r, c]: the linear polynomial of E[r, c]
    one = np.zeros((4, 4, 4))
    one[0, 0, 0] = 1.0
    Ep = [[_lin_mul(one, L[r, c]) for c in range(3)] for r in range(3)]
    EEt = [[sum(_lin_mul(Ep[r][k], L[c, k]) for k in range(3)) for c in range(3)] for r in range(3)]
    tr = EEt[0][0] + EEt[1][1] + EEt[2][2]
    eqs = [2.0 * sum(_lin_mul(EEt[r][k], L[k, c]) for k in range(3)) - _lin_mul(tr, L[r, c]) for r in range(3) for c in range(3)]
    minor = lambda a, b: _lin_mul(Ep[1][a], L[2, b]) - _lin_mul(Ep[1][b], L[2, a])   # noqa: E731
    eqs.append(_lin_mul(minor(1, 2), L[0, 0]) - _lin_mul(minor(0, 2), L[0, 1]) + _lin_mul(minor(0, 1), L[0, 2]))
    return np.array([e[_MX, _MY, _MZ] for e in eqs])


def action(B, var='x'):
    """the matrix of multiplication by x (or z) on the basis x2 xy y2 xz yz z2 x y z 1, from the reduced system [I | B]"""
    A = np.zeros((10, 10))
    if var == 'x':      # x * basis = x3 x2y xy2 x2z xyz xz2 | x2 xy xz x
        rows, units = (0, 1, 2, 4, 5, 7), ((6, 0), (7, 1), (8, 3), (9, 6))
    else:               # z * basis = x2z xyz y2z xz2 yz2 z3 | xz yz z2 z
        rows, units = (4, 5, 6, 7, 8, 9), ((6, 3), (7, 4), (8, 5), (9, 8))
    for i, r in enumerate(rows):
        A[i] = -B[r]
    for i, j in units:
        A[i, j] = 1.0
    return A


def _monomials(p):
    x, y, z = p
    m3 = np.array([x * x * x, x * x * y, x * y * y, y * y * y, x * x * z, x * y * z, y * y * z, x * z * z, y * z * z, z * z * z])
    d3 = np.array([[3 * x * x, 2 * x * y, y * y, 0, 2 * x * z, y * z, 0, z * z, 0, 0],
                   [0, x * x, 2 * x * y, 3 * y * y, 0, x * z, 2 * y * z, 0, z * z, 0],
                   [0, 0, 0, 0, x * x, x * y, y * y, 2 * x * z, 2 * y * z, 3 * z * z]])
    low = np.array([x * x, x * y, y * y, x * z, y * z, z * z, x, y, z, 1.0])
    dl = np.array([[2 * x, y, 0, z, 0, 0, 1, 0, 0, 0], [0, x, 2 * y, 0, z, 0, 0, 1, 0, 0], [0, 0, 0, x, y, 2 * z, 0, 0, 1, 0]], np.float64)
    return m3, d3, low, dl


def polish(B, p, steps=POLISH):
    """Gauss-Newton steps on the ten constraints m3_i(p) + sum_j B[i, j] low_j(p) = 0; a step whose 3 x 3 normal equations
    are singular by the full-pivot rule is skipped"""
    p = np.array(p, np.float64)
    for _ in range(steps):
        with np.errstate(all='ignore'):
            m3, d3, low, dl = _monomials(p)
            r = m3 + B @ low
            J = d3.T + B @ dl.T
            d = solve_full_pivot(J.T @ J, J.T @ r)
        if d is not None:
            p = p - d
    return p


def unit_signed(E):
    """unit Frobenius norm, the first entry of largest magnitude positive"""
    with np.errstate(all='ignore'):
        E = E / np.sqrt((E * E).sum())
    return -E if E[np.argmax(np.abs(E))] < 0 else E


def five_point(x1, x2, var='x', steps=POLISH):
    """x1, x2 [5,2] normalised points -> the list of candidates E [9] (x2h^T E x1h = 0) in ascending order of the root;
    [] for a degenerate sample"""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    Q = np.stack([x2[:, 0] * x1[:, 0], x2[:, 0] * x1[:, 1], x2[:, 0], x2[:, 1] * x1[:, 0], x2[:, 1] * x1[:, 1], x2[:, 1],
                  x1[:, 0], x1[:, 1], np.ones(MODEL)], axis=1)
    if not np.isfinite(Q).all():
        return []
    _, sv, vt = np.linalg.svd(Q)
    if not sv[MODEL - 1] > RANK_TOL * sv[0]:
        return []
    N = vt[MODEL:]
    M = constraints(N)
    M = M / np.linalg.norm(M, axis=1, keepdims=True)
    sv = np.linalg.svd(M[:, :10], compute_uv=False)
    if not sv[-1] > RANK_TOL * sv[0]:
        return []
    B = np.linalg.solve(M[:, :10], M[:, 10:])
    w, V = np.linalg.eig(action(B, var))
    out = []
    for i in np.argsort(w.real, kind='stable'):
        if w[i].imag != 0:
            continue
        v = V[:, i].real
        with np.errstate(all='ignore'):
            p = polish(B, (v[6] / v[9], v[7] / v[9], v[8] / v[9]), steps)
        out.append(unit_signed(p[0] * N[0] + p[1] * N[1] + p[2] * N[2] + N[3]))
    return out


def candidates(xn1, xn2, smp, var='x'):
    """-> (slot table [10 * iters, 9], number of candidates per iteration [iters]); a slot without a candidate holds NaN"""
    E = np.full((SLOTS * len(smp), 9), np.nan)
    nc = np.zeros(len(smp), np.int64)
    for it, s in enumerate(smp):
        if (s < 0).any():
            continue
        c = five_point(xn1[s], xn2[s], var)
        nc[it] = len(c)
        for k, e in enumerate(c):
            E[SLOTS * it + k] = e
    return E, nc


def set_distance(a, b):
    """two lists of candidates compared as sets, up to sign: the largest entry difference under a greedy matching (inf when
    their sizes differ)"""
    if len(a) != len(b):
        return np.inf
    used, worst = set(), 0.0
    for e in a:
        best, bj = np.inf, -1
        for j, f in enumerate(b):
            if j not in used:
                d = min(np.abs(e - f).max(), np.abs(e + f).max())
                if d < best:
                    best, bj = d, j
        used.add(bj)
        worst = max(worst, best)
    return worst


def residuals(E, x1, x2):
    """of a candidate at unit norm: (the largest |x2h^T E x1h| over the sample, ||2 E E^T E - tr(E E^T) E||)"""
    E = np.asarray(E, np.float64).reshape(3, 3)
    E = E / np.linalg.norm(E)
    h1, h2 = np.c_[x1, np.ones(len(x1))], np.c_[x2, np.ones(len(x2))]
    epi = np.abs(((h2 @ E) * h1).sum(axis=1)).max()
    return epi, np.linalg.norm(2.0 * E @ E.T @ E - np.trace(E @ E.T) * E)


# ---- error, count ---------------------------------------------------------------------------------------------------------
def errors(E, xn1, xn2):
    """float32 [K, n] Sampson errors of the candidates E [K, 9] on normalised points, in the device's operation order"""
    E = np.asarray(E, np.float64).reshape(-1, 9)
    x1, y1, x2, y2 = xn1[None, :, 0], xn1[None, :, 1], xn2[None, :, 0], xn2[None, :, 1]
    e = [E[:, i:i + 1] for i in range(9)]
    with np.errstate(all='ignore'):
        a0 = e[0] * x1 + e[1] * y1 + e[2]
        a1 = e[3] * x1 + e[4] * y1 + e[5]
        a2 = e[6] * x1 + e[7] * y1 + e[8]
        b0 = e[0] * x2 + e[3] * y2 + e[6]
        b1 = e[1] * x2 + e[4] * y2 + e[7]
        d = x2 * a0 + y2 * a1 + a2
        return (d * d / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1)).astype(np.float32)


def inliers(E, xn1, xn2, thr):
    """thr: the threshold in normalised units (scaled_threshold)"""
    return errors(E, xn1, xn2) <= np.float32(thr * thr)


def counts(E, has, xn1, xn2, thr, rows=256):
    """-1 for a slot without a candidate, 0 for a non-finite candidate"""
    return ro.counts(E, has, lambda Ec: inliers(Ec, xn1, xn2, thr), rows)


def slots_used(nc):
    """bool [10 * iters]: slot 10 it + k holds a candidate"""
    return (np.arange(SLOTS)[None, :] < np.asarray(nc)[:, None]).reshape(-1)


# ---- selection ------------------------------------------------------------------------------------------------------------
def select_sequential(cnt, max_iters, n, confidence):
    """the RANSAC loop written out: -> (found, best, iterations run, chosen slot)"""
    return ro.select_sequential(cnt, max_iters, n, confidence, MODEL, SLOTS)


def select(cnt, max_iters, n, confidence):
    """the same rule as the device replays it"""
    return ro.select(cnt, max_iters, n, confidence, MODEL, SLOTS)


def ransac(pts1, pts2, K1, K2=None, threshold=1.0, confidence=0.999, max_iters=1000, seed=0, var='x'):
    """the whole rule -> dict(samples, hyp_E, hyp_count, info [8], E [9], mask)"""
    K2 = K1 if K2 is None else K2
    n = len(pts1)
    xn1, xn2 = normalise(pts1, K1), normalise(pts2, K2)
    thr = scaled_threshold(threshold, K1, K2)
    smp = samples(n, max_iters, seed)
    Ec, nc = candidates(xn1, xn2, smp, var)
    cnt = counts(Ec, slots_used(nc), xn1, xn2, thr)
    found, best, runs, slot = select(cnt, max_iters, n, confidence)
    E = Ec[slot] if found else np.zeros(9)
    mask = inliers(E, xn1, xn2, thr)[0] if found else np.zeros(n, bool)
    return dict(samples=smp, hyp_E=Ec, hyp_count=cnt, ncand=nc, info=np.array([found, best, runs, slot, 0, 0, 0, 0]), E=E, mask=mask)


# ---- the pose of an essential matrix --------------------------------------------------------------------------------------
def decompose(E):
    """-> (U, V, R1, R2, t) or None: V from Jacobi on E^T E with the column of the smallest eigenvalue last and the other two
    in their order; U = E v / sigma for the two leading columns, their cross product for the third; V's last column signed so
    that det V > 0; R1 = U W V^T, R2 = U W^T V^T with W = [0 1 0; -1 0 0; 0 0 1]; t = U[:, 2]"""
    E = np.asarray(E, np.float64).reshape(3, 3)
    if not np.isfinite(E).all():
        return None
    A = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            A[i, j] = E[0, i] * E[0, j] + E[1, i] * E[1, j] + E[2, i] * E[2, j]
    lam, Vj = jacobi(A)
    m = int(np.argmin(lam))
    V = Vj[:, [c for c in range(3) if c != m] + [m]]
    U = np.zeros((3, 3))
    for c in range(2):
        u = E[:, 0] * V[0, c] + E[:, 1] * V[1, c] + E[:, 2] * V[2, c]
        sg = np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
        if not sg > 0.0:
            return None
        U[:, c] = u / sg
    U[0, 2] = U[1, 0] * U[2, 1] - U[2, 0] * U[1, 1]
    U[1, 2] = U[2, 0] * U[0, 1] - U[0, 0] * U[2, 1]
    U[2, 2] = U[0, 0] * U[1, 1] - U[1, 0] * U[0, 1]
    if np.linalg.det(V) < 0:
        V[:, 2] = -V[:, 2]
    R1, R2 = np.zeros((3, 3)), np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            R1[i, j] = -U[i, 1] * V[j, 0] + U[i, 0] * V[j, 1] + U[i, 2] * V[j, 2]
            R2[i, j] = U[i, 1] * V[j, 0] - U[i, 0] * V[j, 1] + U[i, 2] * V[j, 2]
    return U, V, R1, R2, U[:, 2].copy()


def depths(R, t, xn1, xn2):
    """the least-squares depths (z1, z2) of z2 x2h = z1 a + t with a = R x1h, in the device's operation order, and the
    determinant of the 2 x 2 normal system"""
    x1, y1, x2, y2 = xn1[:, 0], xn1[:, 1], xn2[:, 0], xn2[:, 1]
    with np.errstate(all='ignore'):
        a0 = R[0, 0] * x1 + R[0, 1] * y1 + R[0, 2]
        a1 = R[1, 0] * x1 + R[1, 1] * y1 + R[1, 2]
        a2 = R[2, 0] * x1 + R[2, 1] * y1 + R[2, 2]
        aa = a0 * a0 + a1 * a1 + a2 * a2
        ab = a0 * x2 + a1 * y2 + a2
        bb = x2 * x2 + y2 * y2 + 1.0
        at = a0 * t[0] + a1 * t[1] + a2 * t[2]
        bt = x2 * t[0] + y2 * t[1] + t[2]
        det = aa * bb - ab * ab
        return (ab * bt - at * bb) / det, (aa * bt - ab * at) / det, det


def in_front(R, t, xn1, xn2, dist=50.0):
    z1, z2, det = depths(R, t, xn1, xn2)
    with np.errstate(all='ignore'):
        return (det != 0.0) & (z1 > 0.0) & (z1 < dist) & (z2 > 0.0) & (z2 < dist)


def pose_candidates(E):
    """cv2's order: (R1, t), (R2, t), (R1, -t), (R2, -t); None when E cannot be decomposed"""
    d = decompose(E)
    if d is None:
        return None
    _, _, R1, R2, t = d
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def recover_pose(E, pts1, pts2, K1, K2=None, mask=None, dist=50.0):
    """-> dict(info [8] = (count, chosen, counts[4], 0, 0), R [3,3], t [3], mask [n], margin): margin is how close, relative, a
    depth of a masked point comes to 0 or to dist under any candidate"""
    K2 = K1 if K2 is None else K2
    n = len(pts1)
    xn1, xn2 = normalise(pts1, K1), normalise(pts2, K2)
    m = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1).astype(bool)
    cands = pose_candidates(E)
    if cands is None:
        return dict(info=np.array([0, -1, 0, 0, 0, 0, 0, 0]), R=np.zeros((3, 3)), t=np.zeros(3), mask=np.zeros(n, bool), margin=np.inf)
    fronts = [in_front(R, t, xn1, xn2, dist) & m for R, t in cands]
    cnt = [int(f.sum()) for f in fronts]
    chosen = int(np.argmax(cnt))                                 # the first of the largest
    z = np.concatenate([np.stack(depths(R, t, xn1[m], xn2[m])[:2]).ravel() for R, t in cands[:2]])
    z = np.abs(z[np.isfinite(z)])
    margin = float(np.minimum(z, np.abs(z - dist) / dist).min()) if len(z) else np.inf
    R, t = cands[chosen]
    return dict(info=np.array([cnt[chosen], chosen] + cnt + [0, 0]), R=R, t=t, mask=fronts[chosen], margin=margin)


def relative_pose(pts1, pts2, K1, K2=None, dist=50.0, **kw):
    r = ransac(pts1, pts2, K1, K2, **kw)
    if not r['info'][0]:
        return None
    return recover_pose(r['E'], pts1, pts2, K1, K2, r['mask'], dist)


# ---- measures and scenes --------------------------------------------------------------------------------------------------
def rotation_error_deg(R, R_true):
    return float(np.degrees(np.arccos(np.clip((np.trace(np.asarray(R).reshape(3, 3).T @ R_true) - 1.0) / 2.0, -1.0, 1.0))))


def direction_error_deg(t, t_true):
    t, t_true = np.asarray(t, np.float64).ravel(), np.asarray(t_true, np.float64).ravel()
    return float(np.degrees(np.arccos(np.clip(t @ t_true / (np.linalg.norm(t) * np.linalg.norm(t_true)), -1.0, 1.0))))


def essential_of(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ R


def two_view_scene(n, outlier_frac, seed, noise=1.0, size=(640, 480)):
    """n correspondences of random 3-D points in front of both cameras (depth 4-8 in the first): a rotation of 0.1-0.5 rad
    about a random axis, a unit baseline, two different camera matrices with skew, Gaussian pixel noise, a share replaced by
    uniform outliers, float32 points -> (pts1, pts2, K1, K2, R, t, true inlier mask); x2 ~ R x1 + t"""
    rng = np.random.default_rng(seed)
    W, H = size
    K1 = np.array([[rng.uniform(700, 900), rng.uniform(-2, 2), W / 2 + rng.uniform(-20, 20)], [0, rng.uniform(700, 900), H / 2 + rng.uniform(-20, 20)], [0, 0, 1.0]])
    K2 = np.array([[rng.uniform(500, 700), rng.uniform(-2, 2), W / 2 + rng.uniform(-20, 20)], [0, rng.uniform(500, 700), H / 2 + rng.uniform(-20, 20)], [0, 0, 1.0]])
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = rng.uniform(0.1, 0.5)
    S = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(th) * S + (1 - np.cos(th)) * S @ S
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    X = np.concatenate([rng.uniform(-2, 2, (n, 2)), rng.uniform(4, 8, (n, 1))], axis=1)
    Y = X @ R.T + t
    assert (Y[:, 2] > 1.0).all()
    p1, p2 = X @ K1.T, Y @ K2.T
    p1, p2 = p1[:, :2] / p1[:, 2:], p2[:, :2] / p2[:, 2:]
    p1 = p1 + rng.normal(0, 1, p1.shape) * noise
    p2 = p2 + rng.normal(0, 1, p2.shape) * noise
    out = rng.random(n) < outlier_frac
    p2[out] = rng.uniform([0, 0], [W, H], (int(out.sum()), 2))
    return f32(p1), f32(p2), K1, K2, R, t, ~out


# ---- the scenes the tests use ---------------------------------------------------------------------------------------------
# (n, outlier share, noise px, threshold px, confidence, max_iters, seed = scene seed).  Seeds chosen on the CPU
# (tests/test_essential_cpu.py checks it) so that, for the restatement alone: the x-route and the z-route of the action matrix
# give the same number of candidates on every iteration, within 1e-7 as sets; a model is found; no depth of a masked point
# comes within 1e-9 relative of 0 or of the distance threshold.
SCENES = [(64, 0.3, 1.0, 1.0, 0.999, 200, 0), (200, 0.4, 1.0, 1.0, 0.999, 200, 1), (300, 0.0, 0.0, 1.0, 0.999, 200, 2),
          (1000, 0.2, 0.0, 0.5, 0.99, 100, 3), (2048, 0.4, 1.0, 1.5, 0.999, 200, 4)]
# the wavefront and chunk edges in n; in max_iters the solve workgroup of 32 (31, 32, 33), the 64 of the sibling estimators
# (63, 64, 65), the select kernel's stride (1024 threads against 10 * max_iters slots: crossed at 103) and 500 (with a small
# n: the restatement's time goes with the iterations and with slots x points)
EDGES = [(5, 0.0, 0.0, 1.0, 0.999, 1, 0), (6, 0.0, 0.5, 1.0, 0.999, 31, 1), (63, 0.3, 1.0, 1.0, 0.999, 32, 2),
         (64, 0.3, 1.0, 1.0, 0.999, 33, 3), (65, 0.3, 0.5, 1.0, 0.999, 500, 4), (2047, 0.4, 1.0, 1.0, 0.999, 64, 5),
         (2048, 0.4, 0.5, 1.0, 0.999, 65, 6), (2049, 0.4, 1.0, 1.0, 0.999, 103, 7), (5000, 0.3, 1.0, 1.0, 0.999, 1, 8),
         (5000, 0.5, 1.0, 1.0, 0.999, 63, 9)]


@functools.lru_cache(maxsize=None)
def reference(scene):
    """the scene and the whole restatement on it, computed once for every test that asks -> dict(p1, p2, K1, K2, R, t, good,
    ransac, pose); read only"""
    n, outl, noise, thr, conf, iters, seed = scene
    p1, p2, K1, K2, R, t, good = two_view_scene(n, outl, seed, noise)
    r = ransac(p1, p2, K1, K2, thr, conf, iters, seed)
    pose = recover_pose(r['E'], p1, p2, K1, K2, r['mask']) if r['info'][0] else None
    return dict(p1=p1, p2=p2, K1=K1, K2=K2, R=R, t=t, good=good, ransac=r, pose=pose)
