"""numpy restatement of what the RANSAC estimators share (cotr_amd/csrc/ransac.h): the sampler, OpenCV's
iteration update, the sequential selection, the counting rule, the full-pivot solve and the cyclic Jacobi iteration.
guided_oracle, homography_oracle and essential_oracle bind their model size and slots per iteration to these.  numpy only.
Test infrastructure."""
import math

import numpy as np

MAX_DRAWS = 64
RANK_TOL = 1e-12
JACOBI_SWEEPS = 30
DBL_EPSILON = np.finfo(np.float64).eps
DBL_MIN = np.finfo(np.float64).tiny
M64 = (1 << 64) - 1


def f32(p):
    return np.asarray(p, np.float64).astype(np.float32).astype(np.float64)


# ---- sampler --------------------------------------------------------------------------------------------------------------
def splitmix64(x):
    """splitmix64 on uint64 arrays (wrapping arithmetic)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def samples(n, max_iters, seed, model):
    """[max_iters, model] int64: draw d of iteration it is (splitmix64(splitmix64(seed) ^ (it << 6 | d)) >> 32) % n; a
    duplicate is rejected; -1 past the indices drawn when 64 draws give fewer than ``model`` distinct ones"""
    sk = splitmix64(np.uint64(seed & M64))
    it = np.arange(max_iters, dtype=np.uint64)[:, None]
    d = np.arange(MAX_DRAWS, dtype=np.uint64)[None, :]
    z = splitmix64(sk ^ ((it << np.uint64(6)) | d))
    c = ((z >> np.uint64(32)) % np.uint64(n)).astype(np.int64)                    # [it, 64]
    earlier = np.tril(np.ones((MAX_DRAWS, MAX_DRAWS), bool), -1)                  # earlier[d, e]: e < d
    dup = ((c[:, :, None] == c[:, None, :]) & earlier[None]).any(axis=2)
    out = np.full((max_iters, model), -1, np.int64)
    for i in range(max_iters):
        first = c[i][~dup[i]][:model]
        out[i, :len(first)] = first
    return out


# ---- count ----------------------------------------------------------------------------------------------------------------
def counts(table, has_model, inliers_fn, rows=256):
    """inlier counts of the slot table [S, 9]: -1 for a slot without a model (``has_model`` false), 0 for a non-finite
    candidate; inliers_fn(candidates [K, 9]) -> bool [K, n]"""
    table = np.asarray(table, np.float64)
    out = np.zeros(len(table), np.int64)
    finite = np.isfinite(table).all(axis=1)
    for r in range(0, len(table), rows):
        out[r:r + rows] = inliers_fn(table[r:r + rows]).sum(axis=1)
    out[~finite] = 0
    out[~np.asarray(has_model, bool)] = -1
    return out


# ---- iteration update and selection ---------------------------------------------------------------------------------------
def update(p, ep, m, N):
    """OpenCV's RANSACUpdateNumIters"""
    num = math.log(max(1.0 - p, DBL_MIN))
    denom = 1.0 - math.pow(1.0 - ep, m)
    if denom < DBL_MIN:
        return 0
    lden = math.log(denom)
    return N if (lden >= 0 or -num >= N * (-lden)) else int(np.rint(num / lden))


def select_sequential(cnt, max_iters, n, confidence, model, slots):
    """the RANSAC loop written out, ``slots`` candidates per iteration: -> (found, best, iterations run, chosen slot)"""
    niters, best, chosen, it = max_iters, 0, -1, 0
    while it < niters:
        for k in range(slots):
            c = int(cnt[slots * it + k])
            if c > max(best, model - 1):
                best, chosen = c, slots * it + k
                niters = update(confidence, (n - best) / n, model, niters)
        it += 1
    return int(chosen >= 0), best, it, chosen


def select(cnt, max_iters, n, confidence, model, slots):
    """the same rule as the device replays it: jump to the next slot that beats max(best, model - 1) within the iterations
    left"""
    cnt = np.asarray(cnt)
    pos, best, niters, chosen = 0, 0, max_iters, -1
    while True:
        limit = slots * max(niters, chosen // slots + 1 if chosen >= 0 else 0)
        hit = np.flatnonzero(cnt[pos:limit] > max(best, model - 1))
        if not len(hit):
            break
        chosen = pos + int(hit[0])
        best = int(cnt[chosen])
        niters = update(confidence, (n - best) / n, model, niters)
        pos = chosen + 1
    runs = max(niters, chosen // slots + 1) if chosen >= 0 else max_iters
    return int(chosen >= 0), best, runs, chosen


# ---- small dense problems -------------------------------------------------------------------------------------------------
def solve_full_pivot(A, b):
    """A z = b by the device's full-pivot elimination; None when a pivot falls below RANK_TOL times the first one.  As on the
    device, the pivot scan passes over NaN entries (no comparison with a NaN holds) and takes the largest of the others"""
    n = len(b)
    M = np.concatenate([np.array(A, np.float64), np.array(b, np.float64)[:, None]], axis=1)
    perm = list(range(n))
    piv0 = 0.0
    for k in range(n):
        sub = np.abs(M[k:, k:n])
        sub = np.where(np.isnan(sub), -1.0, sub)
        pv = sub.max()
        if k == 0:
            piv0 = pv
        if not pv > RANK_TOL * piv0:
            return None
        pr, pc = np.unravel_index(np.argmax(sub), sub.shape)     # first maximum in row-major order, as the device's scan
        pr, pc = pr + k, pc + k
        M[[k, pr]] = M[[pr, k]]
        M[:, [k, pc]] = M[:, [pc, k]]
        perm[k], perm[pc] = perm[pc], perm[k]
        for r in range(k + 1, n):
            m = M[r, k] / M[k, k]
            M[r, k + 1:] = M[r, k + 1:] - m * M[k, k + 1:]
            M[r, k] = 0.0
    y = np.zeros(n)
    for r in range(n - 1, -1, -1):
        acc = M[r, n]
        for c in range(r + 1, n):
            acc -= M[r, c] * y[c]
        y[r] = acc / M[r, r]
    z = np.zeros(n)
    z[perm] = y
    return z


def jacobi(A, sweeps=JACOBI_SWEEPS):
    """cyclic Jacobi on the symmetric A, the device's rotations -> (diagonal, V): V's columns are the eigenvectors"""
    a = np.array(A, np.float64)
    n = len(a)
    v = np.eye(n)
    for _ in range(sweeps):
        sq = a * a
        if not np.sqrt(sq[~np.eye(n, dtype=bool)].sum()) >= DBL_EPSILON * np.sqrt(sq.sum()):
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                if a[p, q] == 0.0:
                    continue
                with np.errstate(over='ignore'):
                    theta = (a[q, q] - a[p, p]) / (2.0 * a[p, q])
                    t = np.copysign(1.0, theta) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                ap, aq = a[:, p].copy(), a[:, q].copy()
                a[:, p], a[:, q] = c * ap - s * aq, s * ap + c * aq
                ap, aq = a[p].copy(), a[q].copy()
                a[p], a[q] = c * ap - s * aq, s * ap + c * aq
                vp, vq = v[:, p].copy(), v[:, q].copy()
                v[:, p], v[:, q] = c * vp - s * vq, s * vp + c * vq
    return np.diag(a).copy(), v
