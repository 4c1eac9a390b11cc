"""numpy restatement of the 3D-3D registration (cotr_amd/csrc/rigid3d.hip): the 3-point sampler, the
collinearity rule, Horn's closed form on the centred moments, Umeyama's scale, the counts, the selection, the mask, the
two-pass refit with its re-counted masks and its skip rule, and the scenes the tests use.  The sampler, the iteration update
and the selection are ransac_oracle's.

The restatement reaches the candidates by other numerical routes than the device, which runs a cyclic Jacobi iteration on
Horn's 4 x 4 matrix: route B (``route='horn'``, the one the restatement itself uses) takes the eigenvectors of the same
matrix from LAPACK (``np.linalg.eigh``); route A (``route='svd'``) is Umeyama's form, the SVD of the 3 x 3 cross-covariance
with the determinant fix, which never forms the quaternion.

Points: the scenes store both clouds at float32 precision (as points lifted from float32 depth maps are), in float64, so a
"noise-free" scene has the error of that rounding, about 1e-7 of a coordinate, and not that of float64 alone.

numpy only.  Test infrastructure."""
import functools

import numpy as np

from tests import ransac_oracle as ro
from tests.ransac_oracle import f32

MODEL = 3
SLOTS = 1
MAX_ROUNDS = 8


def samples(n, max_iters, seed):
    return ro.samples(n, max_iters, seed, MODEL)


# ---- a candidate: rows 1 and 2 of s R, then t ---------------------------------------------------------------------------
def expand(m, with_scale):
    """[..., 9] candidates -> (s R [..., 3, 3], t [..., 3], s [...]) by the device's rule: s = |row 1| and row 3 =
    (row 1 x row 2) / s with a scale; s = 1 exactly and row 3 = row 1 x row 2 without"""
    m = np.asarray(m, np.float64)
    c0 = m[..., 1] * m[..., 5] - m[..., 2] * m[..., 4]
    c1 = m[..., 2] * m[..., 3] - m[..., 0] * m[..., 5]
    c2 = m[..., 0] * m[..., 4] - m[..., 1] * m[..., 3]
    if with_scale:
        with np.errstate(invalid='ignore', divide='ignore'):
            s = np.sqrt((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2])
            c0, c1, c2 = c0 / s, c1 / s, c2 / s
    else:
        s = np.ones(m.shape[:-1])
    sR = np.stack([m[..., 0], m[..., 1], m[..., 2], m[..., 3], m[..., 4], m[..., 5], c0, c1, c2], axis=-1)
    return sR.reshape(m.shape[:-1] + (3, 3)), m[..., 6:9], s


def pack(sR, t):
    return np.concatenate([np.asarray(sR, np.float64).reshape(9)[:6], np.asarray(t, np.float64).reshape(3)])


def sq_errors(sR, t, src, dst):
    """|s R x + t - y|^2 of the models sR [S, 3, 3], t [S, 3] on every pair, in the device's order of operations -> [S, n]"""
    sR, t = np.asarray(sR, np.float64).reshape(-1, 3, 3), np.asarray(t, np.float64).reshape(-1, 3)
    X, Y, Z = (np.asarray(src, np.float64)[None, :, c] for c in range(3))
    y = np.asarray(dst, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        d = [(((sR[:, r, 0, None] * X + sR[:, r, 1, None] * Y) + sR[:, r, 2, None] * Z) + t[:, r, None]) - y[None, :, r] for r in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def model_inliers(sR, t, src, dst, thr):
    """bool [S, n]: float32(squared distance) <= float32(thr^2); false for NaN"""
    with np.errstate(invalid='ignore', over='ignore'):
        return sq_errors(sR, t, src, dst).astype(np.float32) <= np.float32(thr * thr)


def inliers(cands, src, dst, thr, with_scale):
    sR, t, _ = expand(np.asarray(cands, np.float64).reshape(-1, 9), with_scale)
    return model_inliers(sR, t, src, dst, thr)


def counts(cands, has, src, dst, thr, with_scale):
    return ro.counts(np.asarray(cands).reshape(-1, 9), has, lambda c: inliers(c, src, dst, thr, with_scale))


def select_sequential(cnt, max_iters, n, confidence):
    return ro.select_sequential(cnt, max_iters, n, confidence, MODEL, SLOTS)


def select(cnt, max_iters, n, confidence):
    return ro.select(cnt, max_iters, n, confidence, MODEL, SLOTS)


# ---- the closed form ------------------------------------------------------------------------------------------------------
def collinear(p):
    """p [m, 3 points, 3]: |e1 x e2| <= RANK_TOL |e1| |e2| (true for NaN too)"""
    with np.errstate(invalid='ignore', over='ignore'):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        return ~(np.linalg.norm(np.cross(e1, e2), axis=1) > ro.RANK_TOL * (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)))


def horn_matrix(S):
    """S [..., 3, 3], S[j, i] = sum a'_j b'_i -> Horn's symmetric 4 x 4 matrix N"""
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = (S[..., j, i] for j in range(3) for i in range(3))
    rows = [[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx], [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
            [Szx - Sxz, Sxy + Syx, Syy - Sxx - Szz, Syz + Szy], [Sxy - Syx, Szx + Sxz, Syz + Szy, Szz - Sxx - Syy]]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


def quaternion_rotation(q):
    w, x, y, z = (q[..., i] for i in range(4))
    rows = [[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


def closed_form(S, saa, ca, cb, with_scale, route='horn'):
    """moments S [m, 3, 3], saa [m], centroids ca, cb [m, 3] -> (s R [m, 3, 3], t [m, 3], s [m], ok [m]).
    route 'horn': the eigenvector of the largest eigenvalue of N (LAPACK), degenerate when l1 is not finite and > 0 or
    l1 - l2 <= RANK_TOL l1; route 'svd': Umeyama, R = U diag(1, 1, det(U V^T)) V^T of the SVD of sum b' a'^T, no such test.
    With a scale it must be finite and > 0."""
    S, saa = np.asarray(S, np.float64), np.asarray(saa, np.float64)
    good = np.isfinite(S).all(axis=(1, 2)) & np.isfinite(saa)
    Sg = np.where(good[:, None, None], S, np.eye(3))
    with np.errstate(all='ignore'):
        if route == 'horn':
            w, V = np.linalg.eigh(horn_matrix(Sg))                                # ascending
            l1, l2 = w[:, 3], w[:, 2]
            ok = good & (l1 > 0) & (l1 < np.inf) & (l1 - l2 > ro.RANK_TOL * l1)
            q = V[:, :, 3]
            R = quaternion_rotation(q / np.linalg.norm(q, axis=1, keepdims=True))
            num = np.einsum('mij,mji->m', R, Sg)
        else:
            U, D, Vt = np.linalg.svd(np.swapaxes(Sg, 1, 2))
            sign = np.sign(np.linalg.det(U @ Vt))
            fix = np.stack([np.ones_like(sign), np.ones_like(sign), sign], axis=1)
            R = (U * fix[:, None, :]) @ Vt
            num = (D * fix).sum(axis=1)
            ok = good.copy()
        if with_scale:
            s = num / saa
            ok &= (s > 0) & (s < np.inf)
        else:
            s = np.ones(len(S))
        sR = s[:, None, None] * R
        t = cb - np.einsum('mij,mj->mi', sR, ca)
    return sR, t, s, ok


def candidates(src, dst, smp, with_scale, route='horn'):
    """the candidate of every sample [iters, 3] (-1: short draw) -> (table [iters, 9], NaN without a candidate; has bool)"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    full = (smp >= 0).all(axis=1)
    idx = np.where(full[:, None], smp, 0)
    a, b = src[idx], dst[idx]                                                     # [iters, 3, 3]
    full &= np.isfinite(a).all(axis=(1, 2)) & np.isfinite(b).all(axis=(1, 2))
    a, b = np.where(full[:, None, None], a, 0.0), np.where(full[:, None, None], b, 0.0)
    full &= ~collinear(a) & ~collinear(b)
    ca, cb = ((a[:, 0] + a[:, 1]) + a[:, 2]) / 3.0, ((b[:, 0] + b[:, 1]) + b[:, 2]) / 3.0
    da, db = a - ca[:, None], b - cb[:, None]
    S = np.einsum('mkj,mki->mji', da, db)
    sR, t, _, ok = closed_form(S, (da * da).sum(axis=(1, 2)), ca, cb, with_scale, route)
    table = np.concatenate([sR.reshape(-1, 9)[:, :6], t], axis=1)
    has = full & ok & np.isfinite(table).all(axis=1)
    table[~has] = np.nan
    return table, has


def model_distance(sRa, ta, sRb, tb):
    """the largest entry difference of s R and of t / max(1, |t|)"""
    tb = np.asarray(tb, np.float64)
    return max(np.abs(np.asarray(sRa) - np.asarray(sRb)).max(), np.abs(np.asarray(ta) - tb).max() / max(1.0, np.linalg.norm(tb)))


def candidate_distance(a, b, with_scale):
    (sRa, ta, _), (sRb, tb, _) = expand(a, with_scale), expand(b, with_scale)
    return model_distance(sRa, ta, sRb, tb)


# ---- the refit ------------------------------------------------------------------------------------------------------------
def _total(T, reverse):
    return np.cumsum(T[::-1] if reverse else T, axis=0)[-1]


def fit(src, dst, mask, with_scale, sR0=None, t0=None, reverse=False):
    """one round on the masked pairs, each sum added point by point in order (reverse: in reversed order): pass 1 the count and
    the coordinate sums -> the centroids; pass 2 the centred moments -> the closed form
    -> (s R, t, s, squared error of (sR0, t0) on the mask), or None when the round is skipped: fewer than 3 points, or
    degenerate moments"""
    a, b = np.asarray(src, np.float64)[mask], np.asarray(dst, np.float64)[mask]
    cnt = float(len(a))
    if cnt < MODEL:
        return None
    ca, cb = _total(a, reverse) / cnt, _total(b, reverse) / cnt
    da, db = a - ca, b - cb
    S = _total((da[:, :, None] * db[:, None, :]).reshape(-1, 9), reverse).reshape(3, 3)
    saa = _total((da[:, 0] * da[:, 0] + da[:, 1] * da[:, 1]) + da[:, 2] * da[:, 2], reverse)
    err = 0.0 if sR0 is None else _total(sq_errors(sR0, t0, a, b)[0], reverse)
    sR, t, s, ok = closed_form(S[None], np.array([saa]), ca[None], cb[None], with_scale)
    if not ok[0]:
        return None
    return sR[0], t[0], float(s[0]), float(err)


def refit(src, dst, mask, thr, with_scale, sR, t, s, rounds, reverse=False):
    """the rounds of the device from the chosen model and its mask -> (s R, t, s, mask of the last executed round, rounds run)"""
    run = 0
    for r in range(rounds):
        m = mask if r == 0 else model_inliers(sR, t, src, dst, thr)[0]
        got = fit(src, dst, m, with_scale, sR, t, reverse)
        if got is None:
            break
        sR, t, s, _ = got
        mask, run = m, run + 1
    return sR, t, s, mask, run


# ---- the whole estimator --------------------------------------------------------------------------------------------------
def ransac(src, dst, threshold, confidence=0.99, max_iters=100, seed=0, with_scale=False, rounds=2):
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    n = len(src)
    smp = samples(n, max_iters, seed)
    table, has = candidates(src, dst, smp, with_scale)
    cnt = counts(table, has, src, dst, threshold, with_scale)
    found, best, runs, slot = select(cnt, max_iters, n, confidence)
    out = dict(samples=smp, hyp_model=table, hyp_count=cnt, has=has)
    if not found:
        return dict(out, info=np.array([0, 0, runs, -1, 0, 0, 0, 0]), R=np.zeros((3, 3)), t=np.zeros(3), scale=0.0, mask=np.zeros(n, bool))
    mask0 = inliers(table[slot], src, dst, threshold, with_scale)[0]
    sR0, t0, s0 = expand(table[slot], with_scale)
    sR, t, s, mask, run = refit(src, dst, mask0, threshold, with_scale, sR0, t0, float(s0), rounds)
    return dict(out, info=np.array([1, best, runs, slot, run, int(mask.sum()), 0, 0]), R=sR / s, t=t, scale=s, mask=mask, mask_ransac=mask0)


# ---- errors against a scene -----------------------------------------------------------------------------------------------
def scene_errors(R, t, s, ref):
    """(largest difference of a rotation entry, |t - t_true| / |t_true|, |s - s_true| / s_true)"""
    return (float(np.abs(np.asarray(R, np.float64).reshape(3, 3) - ref['R']).max()),
            float(np.linalg.norm(np.asarray(t, np.float64).ravel() - ref['t']) / np.linalg.norm(ref['t'])), abs(float(s) - ref['s']) / ref['s'])


# ---- scenes ---------------------------------------------------------------------------------------------------------------
CENTRE = np.array([3.0, -5.0, 8.0])


def rotation(axis, angle):
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    S = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * S @ S


def rigid_scene(n, outlier_frac, seed, noise, with_scale, shift=0.0):
    """n points in a 4-unit box around (3, -5, 8) (+ shift), a rotation of 0.2-2.5 rad about a random axis, a translation in
    [-3, 3]^3, a scale in [0.5, 2] (1 without), Gaussian noise on the target, a share of the targets replaced by uniform
    points of the targets' bounding box, both clouds rounded to float32 (shift = 0 only)
    -> (src, dst float64 [n, 3], R, t, s, true inlier mask); dst = s R src + t"""
    rng = np.random.default_rng(seed)
    R = rotation(rng.normal(size=3), rng.uniform(0.2, 2.5))
    t = rng.uniform(-3, 3, 3)
    s = float(rng.uniform(0.5, 2.0)) if with_scale else 1.0
    src = CENTRE + shift + rng.uniform(-2, 2, (n, 3))
    if shift == 0.0:
        src = f32(src)
    dst = s * (src @ R.T) + t
    lo, hi = dst.min(axis=0), dst.max(axis=0)
    dst = dst + rng.normal(0, 1, dst.shape) * noise
    out = rng.random(n) < outlier_frac
    if n <= 4:
        out[:] = False
    dst[out] = rng.uniform(lo, hi, (int(out.sum()), 3))
    if shift == 0.0:
        dst = f32(dst)
    return src, dst, R, t, s, ~out


# (n, outlier share, noise, threshold, confidence, max_iters, seed = scene seed); noise and threshold in the clouds' units.
SCENES = [(64, 0.3, 0.01, 0.04, 0.99, 100, 0), (200, 0.5, 0.01, 0.04, 0.99, 200, 1), (300, 0.0, 0.0, 0.02, 0.99, 100, 2),
          (1000, 0.2, 0.0, 0.01, 0.999, 100, 3), (2048, 0.4, 0.005, 0.03, 0.99, 200, 4)]
# n: the smallest problem (3, 4), the wavefront ballot (63, 64, 65), the 256-thread mask block (255, 256, 257), the 2048-point
# count chunk (2047, 2048, 2049; 4097: three chunks); max_iters: the 64-thread solve block (63, 64, 65), the 1024-thread
# select block (1025), 1; two seeds above 2^63
EDGES = [(3, 0.0, 0.0, 0.02, 0.99, 65, 0), (4, 0.0, 0.005, 0.04, 0.99, 64, 1), (63, 0.3, 0.01, 0.04, 0.99, 63, 2), (64, 0.3, 0.01, 0.04, 0.99, 65, 3),
         (65, 0.3, 0.005, 0.04, 0.99, 64, 4), (255, 0.4, 0.01, 0.04, 0.99, 63, 5), (256, 0.0, 0.01, 0.04, 0.99, 1, (1 << 63) + 6),
         (257, 0.2, 0.005, 0.04, 0.99, 65, 7), (2047, 0.4, 0.01, 0.04, 0.99, 64, 8), (2048, 0.4, 0.005, 0.04, 0.99, 65, 9),
         (2049, 0.4, 0.01, 0.04, 0.99, 63, (1 << 63) + 10), (4097, 0.3, 0.01, 0.04, 0.99, 1025, 11)]
CASES = [(scene, ws) for scene in SCENES + EDGES for ws in (False, True)]


def case_id(case):
    scene, ws = case
    return f'n{scene[0]}-it{scene[5]}-{"similarity" if ws else "rigid"}'


@functools.lru_cache(maxsize=None)
def reference(scene, with_scale):
    """the scene and the whole restatement on it (two refit rounds), computed once for every test that asks -> dict(src,
    dst, R, t, s, good, ransac); read only"""
    n, outl, noise, thr, conf, iters, seed = scene
    src, dst, R, t, s, good = rigid_scene(n, outl, seed % (1 << 32), noise, with_scale)
    return dict(src=src, dst=dst, R=R, t=t, s=s, good=good, ransac=ransac(src, dst, thr, conf, iters, seed, with_scale, 2))


# The refit's dependence on the order of its sums, measured on the CPU over SCENES and EDGES in both scale settings
# (tests/test_rigid3d_cpu.py measures it again): one round of the restatement on the RANSAC mask with its sums taken forwards
# against backwards differs by at most 1.04e-14 in an entry of s R and of t / max(1, |t|).  The device, which sums in yet another
# order and takes its eigenvector from a Jacobi iteration, is allowed 1000 times that (the margin of DESIGN.md 3h-2 / 3h-4).
ORDER_NOISE = 1.1e-14
REFIT_BOUND = 1000 * ORDER_NOISE


def order_noise(scene, with_scale):
    r = reference(scene, with_scale)
    o = r['ransac']
    a = fit(r['src'], r['dst'], o['mask_ransac'], with_scale)
    b = fit(r['src'], r['dst'], o['mask_ransac'], with_scale, reverse=True)
    return model_distance(a[0], a[1], b[0], b[1])
