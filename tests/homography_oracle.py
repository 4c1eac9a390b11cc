"""numpy restatement of the homography rules of DESIGN.md 3h-2 (cotr_amd/csrc/homography.hip): the sampler (the F path's
draws, model size 4), the degenerate-sample check, the normalised 4-point solver, the transfer error and count, the
sequential selection, and the refit on the inliers (DLT by cyclic Jacobi, Gauss-Newton steps kept while the error falls).
numpy only.  Test infrastructure."""
import numpy as np

from tests import ransac_oracle as ro
from tests.ransac_oracle import DBL_EPSILON, JACOBI_SWEEPS, f32, solve_full_pivot  # noqa: F401

MODEL = 4
SLOTS = 1
FLT_EPSILON = float(np.finfo(np.float32).eps)
H22_TOL = 1e-12
TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))


# ---- sampler --------------------------------------------------------------------------------------------------------------
def samples(n, max_iters, seed):
    """[max_iters, 4] int64: the first 4 distinct indices of the F path's 64 draws of every iteration, -1 past them"""
    return ro.samples(n, max_iters, seed, MODEL)


# ---- degenerate samples ---------------------------------------------------------------------------------------------------
def _det(p, i, j, k):
    return p[i, 0] * (p[j, 1] - p[k, 1]) - p[i, 1] * (p[j, 0] - p[k, 0]) + (p[j, 0] * p[k, 1] - p[j, 1] * p[k, 0])


def sample_ok(p1, p2):
    """cv2's checkSubset on 4 pairs: no three points on a line in either set, and the orientation of the four triples is
    kept by all of them or by none"""
    negative = 0
    for i, j, k in TRIPLES:
        for p in (p1, p2):
            d1, d2 = p[j] - p[i], p[k] - p[i]
            if abs(d1[1] * d2[0] - d1[0] * d2[1]) <= FLT_EPSILON * (abs(d1[0]) + abs(d1[1]) + abs(d2[0]) + abs(d2[1])):
                return False
        if _det(p1, i, j, k) * _det(p2, i, j, k) < 0:
            negative += 1
    return negative in (0, 4)


# ---- 4-point solver -------------------------------------------------------------------------------------------------------
def solve_numpy(A, b):
    try:
        return np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        return None


def hartley(p):
    """-> (cx, cy, s) with s = sqrt 2 / mean distance to the centroid, or None"""
    k = len(p)
    cx, cy = p[:, 0].sum() / k, p[:, 1].sum() / k
    m = np.sqrt((p[:, 0] - cx) ** 2 + (p[:, 1] - cy) ** 2).sum() / k
    if not 0.0 < m < np.inf:
        return None
    return cx, cy, np.sqrt(2.0) / m


def _T(cx, cy, s):
    return np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1.0]])


def _Tinv(cx, cy, s):
    return np.array([[1.0 / s, 0, cx], [0, 1.0 / s, cy], [0, 0, 1.0]])


def scale(H):
    """unit Frobenius norm, then H[2,2] = 1 unless |H[2,2]| <= DBL_EPSILON (then the F rule's sign)"""
    with np.errstate(all='ignore'):
        H = H / np.sqrt((H * H).sum())
        if abs(H[8]) > DBL_EPSILON:
            H = np.concatenate([H[:8] / H[8], [1.0]])
        elif H[np.argmax(np.abs(H))] < 0:
            H = -H
    return H


def four_point(p1, p2, solver=solve_full_pivot):
    """p1, p2 [4,2] (already rounded to float32) -> H [9] or None"""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    if not sample_ok(p1, p2):
        return None
    n1, n2 = hartley(p1), hartley(p2)
    if n1 is None or n2 is None:
        return None
    x, y = (p1[:, 0] - n1[0]) * n1[2], (p1[:, 1] - n1[1]) * n1[2]
    u, v = (p2[:, 0] - n2[0]) * n2[2], (p2[:, 1] - n2[1]) * n2[2]
    A, b = np.zeros((8, 8)), np.zeros(8)
    for k in range(4):
        A[k] = [x[k], y[k], 1, 0, 0, 0, -(x[k] * u[k]), -(y[k] * u[k])]
        A[k + 4] = [0, 0, 0, x[k], y[k], 1, -(x[k] * v[k]), -(y[k] * v[k])]
        b[k], b[k + 4] = u[k], v[k]
    h = solver(A, b)
    if h is None:
        return None
    Hn = np.append(h, 1.0).reshape(3, 3)
    return scale((_Tinv(*n2) @ Hn @ _T(*n1)).reshape(9))


def candidates(pts1, pts2, smp, solver=solve_full_pivot):
    """-> (slot table [iters, 9], has_model bool [iters]): a slot without a model holds NaN; a slot with one may hold a
    non-finite candidate all the same, so the flag is kept apart, as the device keeps it (count -1 against count 0)"""
    p1, p2 = f32(pts1), f32(pts2)
    H = np.full((len(smp), 9), np.nan)
    has = np.zeros(len(smp), bool)
    for it, s in enumerate(smp):
        if (s < 0).any():
            continue
        h = four_point(p1[s], p2[s], solver)
        if h is not None:
            H[it], has[it] = h, True
    return H, has


# ---- error, count ---------------------------------------------------------------------------------------------------------
def errors(H, pts1, pts2):
    """float32 [K, n] transfer errors of the candidates H [K, 9], in the device's operation order"""
    H = np.asarray(H, np.float64).reshape(-1, 9)
    p1, p2 = f32(pts1), f32(pts2)
    x, y, u, v = p1[None, :, 0], p1[None, :, 1], p2[None, :, 0], p2[None, :, 1]
    h = [H[:, i:i + 1] for i in range(9)]
    with np.errstate(all='ignore'):
        w = 1.0 / (h[6] * x + h[7] * y + h[8])
        dx = (h[0] * x + h[1] * y + h[2]) * w - u
        dy = (h[3] * x + h[4] * y + h[5]) * w - v
        return (dx * dx + dy * dy).astype(np.float32)


def inliers(H, pts1, pts2, threshold):
    return errors(H, pts1, pts2) <= np.float32(threshold * threshold)


def counts(H, has_model, pts1, pts2, threshold, rows=256):
    """-1 for a slot without a model, 0 for a non-finite candidate"""
    return ro.counts(H, has_model, lambda Hc: inliers(Hc, pts1, pts2, threshold), rows)


# ---- selection ------------------------------------------------------------------------------------------------------------
def select_sequential(cnt, max_iters, n, confidence):
    """the RANSAC loop written out: -> (found, best, iterations run, chosen slot)"""
    return ro.select_sequential(cnt, max_iters, n, confidence, MODEL, SLOTS)


def select(cnt, max_iters, n, confidence):
    """the same rule as the device replays it"""
    return ro.select(cnt, max_iters, n, confidence, MODEL, SLOTS)


# ---- refit ----------------------------------------------------------------------------------------------------------------
def jacobi_smallest(A, sweeps=JACOBI_SWEEPS):
    """the eigenvector of the smallest eigenvalue of the symmetric A by cyclic Jacobi, the device's rotations"""
    lam, v = ro.jacobi(A, sweeps)
    return v[:, int(np.argmin(lam))]


def eigh_smallest(A):
    return np.linalg.eigh(np.asarray(A, np.float64))[1][:, 0]


def _sum(terms):
    """left-to-right sum over the points (axis 0)"""
    acc = np.zeros(terms.shape[1:])
    for t in terms:
        acc = acc + t
    return acc


def dlt_matrix(X, Y, U, V):
    one, zero = np.ones_like(X), np.zeros_like(X)
    r1 = np.stack([X, Y, one, zero, zero, zero, -(U * X), -(U * Y), -U], axis=1)
    r2 = np.stack([zero, zero, zero, X, Y, one, -(V * X), -(V * Y), -V], axis=1)
    return _sum(r1[:, :, None] * r1[:, None, :] + r2[:, :, None] * r2[:, None, :])


def gn_sums(h, X, Y, U, V):
    """-> (J^T J [8,8], J^T r [8], squared error) at Hn = h (h[8] = 1)"""
    with np.errstate(all='ignore'):
        w = 1.0 / (h[6] * X + h[7] * Y + h[8])
        px, py = (h[0] * X + h[1] * Y + h[2]) * w, (h[3] * X + h[4] * Y + h[5]) * w
        rx, ry = px - U, py - V
        xw, yw = X * w, Y * w
        zero = np.zeros_like(X)
        j1 = np.stack([xw, yw, w, zero, zero, zero, -(xw * px), -(yw * px)], axis=1)
        j2 = np.stack([zero, zero, zero, xw, yw, w, -(xw * py), -(yw * py)], axis=1)
        JtJ = _sum(j1[:, :, None] * j1[:, None, :] + j2[:, :, None] * j2[:, None, :])
        Jtr = _sum(j1 * rx[:, None] + j2 * ry[:, None])
        err = _sum((rx * rx + ry * ry)[:, None])[0]
    return JtJ, Jtr, err


def refit(pts1, pts2, mask, refine_iters=10, H_ransac=None, eig=jacobi_smallest, solver=solve_full_pivot, order=None):
    """the refit on the inliers ``mask`` -> (H [9], steps kept, status, H of the DLT alone [9]).  order: a permutation of the
    inliers, the order every sum over them is taken in (default: ascending; reversed or shuffled to measure how far the
    result depends on the summation order)"""
    p1, p2 = f32(pts1)[mask], f32(pts2)[mask]
    if order is not None:
        p1, p2 = p1[order], p2[order]
    n1, n2 = hartley(p1), hartley(p2)
    if n1 is None or n2 is None:
        return H_ransac, 0, 2, H_ransac
    X, Y = (p1[:, 0] - n1[0]) * n1[2], (p1[:, 1] - n1[1]) * n1[2]
    U, V = (p2[:, 0] - n2[0]) * n2[2], (p2[:, 1] - n2[1]) * n2[2]
    e = eig(dlt_matrix(X, Y, U, V))
    nrm = np.sqrt((e * e).sum())
    if not (np.isfinite(e).all() and nrm > 0):
        return H_ransac, 0, 2, H_ransac
    den = lambda hn: scale((_Tinv(*n2) @ hn.reshape(3, 3) @ _T(*n1)).reshape(9))   # noqa: E731
    if not abs(e[8]) > H22_TOL * nrm:
        return den(e), 0, 1, den(e)
    h = np.append(e[:8] / e[8], 1.0)
    h_dlt = h.copy()
    kept, status = 0, 1
    if refine_iters > 0:
        status = 0
        JtJ, Jtr, err = gn_sums(h, X, Y, U, V)
        for _ in range(refine_iters):
            d = solver(JtJ, -Jtr)
            if d is None:
                break
            trial = h.copy()
            trial[:8] = trial[:8] + d
            JtJ_t, Jtr_t, err_t = gn_sums(trial, X, Y, U, V)
            if not err_t < err:
                break
            h, JtJ, Jtr, err = trial, JtJ_t, Jtr_t, err_t
            kept += 1
    return den(h), kept, status, den(h_dlt)


def ransac(pts1, pts2, threshold=3.0, confidence=0.995, max_iters=2000, seed=0, refine_iters=10):
    """the whole rule -> dict(samples, hyp_H, hyp_count, info [8], H_ransac, H, mask)"""
    n = len(pts1)
    smp = samples(n, max_iters, seed)
    Hc, has = candidates(pts1, pts2, smp)
    cnt = counts(Hc, has, pts1, pts2, threshold)
    found, best, runs, slot = select(cnt, max_iters, n, confidence)
    if not found:
        return dict(samples=smp, hyp_H=Hc, hyp_count=cnt, info=np.array([0, best, runs, slot, 0, 2, 0, 0]), H_ransac=np.zeros(9),
                    H=np.zeros(9), mask=np.zeros(n, bool))
    mask = inliers(Hc[slot], pts1, pts2, threshold)[0]
    H, kept, status, _ = refit(pts1, pts2, mask, refine_iters, Hc[slot])
    return dict(samples=smp, hyp_H=Hc, hyp_count=cnt, info=np.array([1, best, runs, slot, kept, status, 0, 0]), H_ransac=Hc[slot],
                H=H, mask=mask)


# ---- measures and scenes --------------------------------------------------------------------------------------------------
def apply(H, p):
    H = np.asarray(H, np.float64).reshape(3, 3)
    q = np.concatenate([np.asarray(p, np.float64), np.ones((len(p), 1))], axis=1) @ H.T
    return q[:, :2] / q[:, 2:]


def bbox_corners(p):
    p = np.asarray(p, np.float64)
    (x0, y0), (x1, y1) = p.min(axis=0), p.max(axis=0)
    return np.array([[x0, y0], [x1, y0], [x0, y1], [x1, y1]])


def corner_error(Ha, Hb, p):
    """the largest distance (px) between where Ha and Hb send the corners of the bounding box of the points p"""
    c = bbox_corners(p)
    return float(np.linalg.norm(apply(Ha, c) - apply(Hb, c), axis=1).max())


def order_noise(pts1, pts2, mask, refine_iters=10, shuffles=6):
    """the largest corner distance (px) between the refit summed in ascending order and summed in reversed order and in
    ``shuffles`` random orders: the oracle's own dependence on the summation order"""
    k = int(np.sum(mask))
    H = refit(pts1, pts2, mask, refine_iters)[0]
    rng = np.random.default_rng(k)
    orders = [np.arange(k)[::-1]] + [rng.permutation(k) for _ in range(shuffles)]
    return max(corner_error(H, refit(pts1, pts2, mask, refine_iters, order=o)[0], pts1) for o in orders)


def sq_error(H, pts1, pts2, mask):
    """float64 squared transfer error summed over the mask"""
    d = apply(H, f32(pts1)[mask]) - f32(pts2)[mask]
    return float((d * d).sum())


def planar_scene(n, outlier_frac, seed, noise=0.5, size=(640, 480)):
    """n correspondences of a plane: a random similarity plus perspective terms up to 3e-4, Gaussian noise on the images of
    the inliers, a fraction replaced by uniform outliers, everything rounded to float32 -> (pts1, pts2, true inlier mask,
    H_true [3,3])"""
    rng = np.random.default_rng(seed)
    W, Hh = size
    a, s = rng.uniform(-0.5, 0.5), rng.uniform(0.7, 1.4)
    Ht = np.array([[s * np.cos(a), -s * np.sin(a), rng.uniform(-60, 60)],
                   [s * np.sin(a), s * np.cos(a), rng.uniform(-60, 60)],
                   [rng.uniform(-3e-4, 3e-4), rng.uniform(-3e-4, 3e-4), 1.0]])
    p1 = rng.uniform([0, 0], [W, Hh], (n, 2))
    p2 = apply(Ht, p1) + rng.normal(0, noise, (n, 2))
    out = rng.random(n) < outlier_frac
    p2[out] = rng.uniform([0, 0], [W, Hh], (int(out.sum()), 2))
    return f32(p1), f32(p2), ~out, Ht


# ---- the scenes the tests use ---------------------------------------------------------------------------------------------
# (n, outlier share, noise px, threshold, confidence, max_iters, seed = scene seed).  Seeds chosen on the CPU so that, for the
# restatement alone: the refit's corner error against the scene's H is below H_ransac's; the two 4-point solvers agree on
# every iteration; and the refit moves by less than 1e-9 px when its sums are taken in reversed and in shuffled orders
# (order_noise).  The last one matters: a Gauss-Newton step is kept only while the summed squared error falls, and close to
# the minimum the summation order decides whether the last, marginal step is kept.  On most scenes that moves H by 1e-9 to
# 1e-6 px (40 of 60 seeds tried), far below the 3e-5 px of the float32 input rounding but above what a bound under 1e-6 px
# allows as noise; the scenes below are those where it stays under 1e-9 px.
SCENES = [(64, 0.3, 0.5, 3.0, 0.995, 500, 0), (200, 0.6, 1.0, 3.0, 0.999, 1000, 2), (300, 0.45, 2.0, 4.0, 0.995, 1000, 0),
          (1000, 0.5, 0.5, 2.0, 0.99, 500, 0), (2048, 0.4, 1.0, 3.0, 0.995, 300, 6)]
# the wavefront and chunk edges in n, the solve-workgroup edges in max_iters
EDGES = [(4, 0.0, 0.5, 3.0, 0.995, 1, 1), (5, 0.0, 0.5, 3.0, 0.995, 63, 17), (63, 0.3, 0.5, 3.0, 0.995, 64, 4),
         (64, 0.3, 1.0, 3.0, 0.995, 65, 15), (65, 0.3, 0.5, 3.0, 0.995, 1000, 1), (2047, 0.4, 0.5, 3.0, 0.995, 63, 2),
         (2048, 0.4, 0.5, 3.0, 0.995, 64, 1), (2049, 0.4, 1.0, 3.0, 0.995, 65, 1), (5000, 0.3, 0.5, 3.0, 0.995, 1, 1),
         (5000, 0.5, 1.0, 3.0, 0.995, 200, 10)]
# The largest order_noise over SCENES + EDGES, measured on the CPU: 6.24e-10 px (scene n = 64; most are near 1e-13).  The
# device differs from the restatement by its summation order and by last-bit differences of the Jacobi rotations: allowed
# 1000 times the measured noise, which has to stay below 1e-6 px.
ORDER_NOISE_PX = 6.3e-10
REFIT_BOUND_PX = 1000 * ORDER_NOISE_PX
assert REFIT_BOUND_PX < 1e-6
