"""numpy float64 restatement of the dense point-to-plane ICP (cotr_amd/csrc/icp.hip): the vertex and normal
maps, one evaluation (the 29 sums, the association, and the source pixels that sit near a decision), one step, the loop, and
the scenes the tests use.  The products and sums of the maps and of the gates are written in the device's order, so maps and
associations can be compared exactly; the step goes another numerical route (``np.linalg.eigh`` where the device runs a
cyclic Jacobi iteration), and the sums are added sequentially where the device adds per thread, wavefront and chunk.

numpy only.  Test infrastructure."""
import functools

import numpy as np

from tests import pnp_oracle as po

MIN_PAIRS = 6
NEAR = 1e-9


# ---- the maps -------------------------------------------------------------------------------------------------------------
def maps(depth, K, edge=0.05):
    """depth [H, W] float32 -> [H, W, 6]: the vertex of every pixel centre (the rule of pnp_oracle.lift without c2w), then the
    unit normal from the central differences of the four neighbours' vertices, turned towards the camera; NaN where invalid"""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    fx, s, cx, fy, cy = po.cam(K)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    z = depth.astype(np.float64)
    ok = (z > 0) & (z < np.inf)
    yn = (ys - cy) / fy
    xn = (xs - cx - s * yn) / fx
    with np.errstate(all='ignore'):
        V = np.stack([xn * z, yn * z, z], axis=-1)
    V[~ok] = np.nan
    N = np.full((H, W, 3), np.nan)
    c = V[1:-1, 1:-1]
    l, r, u, d = V[1:-1, :-2], V[1:-1, 2:], V[:-2, 1:-1], V[2:, 1:-1]
    with np.errstate(all='ignore'):
        good = ok[1:-1, 1:-1] & ok[1:-1, :-2] & ok[1:-1, 2:] & ok[:-2, 1:-1] & ok[2:, 1:-1]
        lim = edge * c[..., 2]
        for nb in (l, r, u, d):
            good &= np.abs(nb[..., 2] - c[..., 2]) <= lim
        a, b = r - l, d - u
        n0 = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
        n1 = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
        n2 = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
        norm = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
        good &= norm > 0
        n = np.stack([n0 / norm, n1 / norm, n2 / norm], axis=-1)
        away = (n[..., 0] * c[..., 0] + n[..., 1] * c[..., 1]) + n[..., 2] * c[..., 2] > 0
        n[away] = -n[away]
    n[~good] = np.nan
    N[1:-1, 1:-1] = n
    return np.concatenate([V, N], axis=-1)


def source(maps_b, stride=1, src_mask=None):
    """-> (X [n_src, 3], n [n_src, 3], usable [n_src]): the source pixels in row-major order"""
    m = maps_b[::stride, ::stride].reshape(-1, 6)
    usable = ~np.isnan(m[:, 3])
    if src_mask is not None:
        usable &= np.asarray(src_mask)[::stride, ::stride].reshape(-1) != 0
    return m[:, :3], m[:, 3:], usable


# ---- one evaluation -------------------------------------------------------------------------------------------------------
def _rot(R, X):
    return np.stack([(R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1]) + R[i, 2] * X[:, 2] for i in range(3)], axis=1)


def evaluate(maps_a, K_a, maps_b, R, t, max_dist=0.25, normal_cos=0.5, stride=1, src_mask=None, reverse=False):
    """the gates in the device's order -> dict(sums [29], abs [29] (the sums of the absolute terms), assoc [n_src] (the pixel of
    A, or -1), near [n_src] (a projection within NEAR of a rounding tie, or a gate value within NEAR relative of its
    threshold, at the gate the pixel reached), usable [n_src], terms [n_src, 29])"""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    Ha, Wa = maps_a.shape[:2]
    A = maps_a.reshape(-1, 6)
    fx, s, cx, fy, cy = po.cam(K_a)
    X, nb, usable = source(maps_b, stride, src_mask)
    n = len(X)
    near = np.zeros(n, bool)
    with np.errstate(all='ignore'):
        P = _rot(R, X)
        Y = P + t
        g = usable & (Y[:, 2] > 0)
        near |= usable & (np.abs(Y[:, 2]) <= NEAR * np.linalg.norm(Y, axis=1))
        xn, yn = Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2]
        u, v = (fx * xn + s * yn) + cx, fy * yn + cy
        near |= g & ((np.abs(u - np.floor(u) - 0.5) <= NEAR) | (np.abs(v - np.floor(v) - 0.5) <= NEAR))
        ru, rv = np.rint(u), np.rint(v)
        g = g & (ru >= 0) & (ru < Wa) & (rv >= 0) & (rv < Ha)
        q = np.where(g, rv * Wa + ru, 0).astype(np.int64)
        Va, na = A[q, :3], A[q, 3:]
        g = g & ~np.isnan(na[:, 0])
        d = Y - Va
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        md2 = max_dist * max_dist
        near |= g & (np.abs(d2 - md2) <= NEAR * md2)
        g = g & (d2 <= md2)
        Rn = _rot(R, nb)
        dot = (Rn[:, 0] * na[:, 0] + Rn[:, 1] * na[:, 1]) + Rn[:, 2] * na[:, 2]
        near |= g & (np.abs(dot - normal_cos) <= NEAR)
        g = g & (dot >= normal_cos)
        r = (na[:, 0] * d[:, 0] + na[:, 1] * d[:, 1]) + na[:, 2] * d[:, 2]
        J = np.stack([P[:, 1] * na[:, 2] - P[:, 2] * na[:, 1], P[:, 2] * na[:, 0] - P[:, 0] * na[:, 2],
                      P[:, 0] * na[:, 1] - P[:, 1] * na[:, 0], na[:, 0], na[:, 1], na[:, 2]], axis=1)
        terms = [J[:, i] * J[:, j] for i in range(6) for j in range(i, 6)] + [J[:, i] * r for i in range(6)] + [r * r, np.ones(n)]
        T = np.stack(terms, axis=1)
    T[~g] = 0.0
    order = T[::-1] if reverse else T
    sums = np.cumsum(order, axis=0)[-1] if n else np.zeros(29)
    return dict(sums=sums, abs=np.abs(T).sum(axis=0), assoc=np.where(g, q, -1).astype(np.int32), near=near, usable=usable, terms=T,
                J=J, r=r, pairs=g)


# ---- one step -------------------------------------------------------------------------------------------------------------
def normal_matrix(sums):
    A = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = sums[k]
            k += 1
    return A


def step(sums, cond_tol=1e-6):
    """-> (stop reason, d [6] or None, l_min, l_max): 1 fewer than 6 pairs, 3 a sum that is not finite, 2 l_min <= cond_tol l_max"""
    if sums[28] < MIN_PAIRS:
        return 1, None, 0.0, 0.0
    if not np.isfinite(sums[:28]).all():
        return 3, None, 0.0, 0.0
    l, V = np.linalg.eigh(normal_matrix(sums))
    lmin, lmax = float(l.min()), float(l.max())
    if not lmin > cond_tol * lmax:
        return 2, None, lmin, lmax
    return 0, -(V @ ((V.T @ sums[21:27]) / l)), lmin, lmax


def apply(R, t, d):
    return po.rotate(d[:3], R), t + d[3:]


def icp(maps_a, K_a, maps_b, R0, t0, iters=10, max_dist=0.25, normal_cos=0.5, cond_tol=1e-6, stride=1, src_mask=None, reverse=False):
    """the chain -> dict(R, t, info [8], stats [2], hist [iters + 1, 32], assoc, poses: the pose of every evaluation run)"""
    R, t = np.array(R0, np.float64).reshape(3, 3), np.array(t0, np.float64).reshape(3)
    hist = np.zeros((iters + 1, 32))
    steps, reason, poses = 0, 0, []
    for k in range(iters + 1):
        e = evaluate(maps_a, K_a, maps_b, R, t, max_dist, normal_cos, stride, src_mask, reverse)
        poses.append((R, t))
        hist[k, :29] = e['sums']
        last = k == iters
        reason, d, lmin, lmax = step(e['sums'], cond_tol)
        if reason in (1, 3):
            break
        if last:   # the last evaluation solves for no step: nothing is known about the conditioning
            reason = 0
            break
        hist[k, 29:31] = lmin, lmax
        if reason == 2:
            break
        R, t = apply(R, t, d)
        steps += 1
    pairs, err = int(e['sums'][28]), float(e['sums'][27])
    n_a = int((~np.isnan(maps_a[..., 3])).sum())
    info = np.array([reason == 0, steps, pairs, reason, int(e['usable'].sum()), n_a, 0, 0], np.int32)
    return dict(R=R, t=t, info=info, stats=np.array([err, np.sqrt(err / pairs) if pairs else 0.0]), hist=hist, assoc=e['assoc'], poses=poses,
                near=e['near'])


# ---- scenes ---------------------------------------------------------------------------------------------------------------
PLANES = (((0.05, -0.03, 1.0), 6.0), ((1.0, 0.0, 0.1), 2.2), ((0.0, 1.0, 0.08), 1.6))
START_TURN = (1.0, -1.5, 0.8)
START_SHIFT = (0.03, -0.02, 0.04)


def render(H, W, K, c2w, planes):
    """the depth of the nearest positive ray-plane intersection through every pixel centre, in float64, as float32; 0 where
    there is none"""
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T @ c2w[:3, :3].T
    best = np.full((H, W), np.inf)
    for normal, offset in planes:
        n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
        with np.errstate(all='ignore'):
            z = (offset - n @ c2w[:3, 3]) / (rays @ n)
        best = np.where((z > 0) & (z < best), z, best)
    return np.where(np.isfinite(best), best, 0.0).astype(np.float32)


def scaled_camera(K, H, W, H0=96, W0=128):
    """the camera of a H0 x W0 map for a H x W map of the same view: its first row times W / W0, its second times H / H0"""
    K = np.array(K, np.float64)
    K[0] = K[0] * W / W0
    K[1] = K[1] * H / H0
    return K


@functools.lru_cache(maxsize=None)
def scene(Ha, Wa, Hb, Wb, planes=3, edge=0.05):
    """the two cameras of pnp_oracle.capture_pair() looking at the first ``planes`` of PLANES, A at Ha x Wa and B at Hb x Wb ->
    dict(depth_a, K_a, c2w_a, depth_b, K_b, c2w_b, R, t: the true x_a = R x_b + t, R0, t0: the start, maps_a, maps_b, edge); read
    only"""
    (_, Ka, ca), (_, Kb, cb) = po.capture_pair(96, 128)
    Ka, Kb = scaled_camera(Ka, Ha, Wa), scaled_camera(Kb, Hb, Wb)
    da, db = render(Ha, Wa, Ka, ca, PLANES[:planes]), render(Hb, Wb, Kb, cb, PLANES[:planes])
    rel = np.linalg.inv(ca) @ cb
    R, t = rel[:3, :3], rel[:3, 3]
    R0, t0 = po.pose_matrix(START_TURN, (0, 0, 0))[:3, :3] @ R, t + np.asarray(START_SHIFT)
    return dict(depth_a=da, K_a=Ka, c2w_a=ca, depth_b=db, K_b=Kb, c2w_b=cb, R=R, t=t, R0=R0, t0=t0, maps_a=maps(da, Ka, edge), maps_b=maps(db, Kb, edge),
                edge=edge)


def corner_scene(H=96, W=128):
    return scene(H, W, H, W, 3)


def pose_distance(Ra, ta, Rb, tb):
    """the largest difference of an entry of R, and of t relative to its norm"""
    Ra, Rb = np.asarray(Ra, np.float64).reshape(3, 3), np.asarray(Rb, np.float64).reshape(3, 3)
    ta, tb = np.asarray(ta, np.float64).reshape(3), np.asarray(tb, np.float64).reshape(3)
    return max(np.abs(Ra - Rb).max(), np.abs(ta - tb).max() / np.linalg.norm(tb))


def errors(R, t, sc):
    """(rotation error: the largest difference of an entry, translation error relative to the norm of the true one)"""
    return po.rotation_error(R, sc['R']), po.translation_error(t, sc['t'])


# B's sizes against A at 96 x 128: the wavefront edges (8x8 = 64, 7x9 = 63, 5x13 = 65), the chunk edges (23x89 = 2047, 32x64 =
# 2048, 3x683 = 2049, 17x241 = 4097), one interior row (3x683), maps too small to hold 6 pairs (3x3, 5x5: 1 and 9 interior
# pixels)
SIZES_B = ((3, 3), (5, 5), (7, 9), (8, 8), (5, 13), (16, 16), (23, 89), (32, 64), (3, 683), (17, 241), (80, 100), (96, 128))
SIZES_B_SMALL_A = ((16, 16), (32, 64), (96, 128))   # against A at 24 x 32


# The dependence of one step on the order of its sums, measured on the CPU from the scene's start over every case below that
# solves (tests/test_icp_cpu.py measures it again): the step from the sums taken forwards against backwards differs by at most
# 1.38e-14 in an entry of R and in t relative to its norm (3.4e-15 at 96 x 128; the worst are the coarse maps, whose normal
# matrix is the worst conditioned).  The device, which sums in yet another order and solves by Jacobi rotations, is allowed
# 1000 times that (the margin of DESIGN.md 3h-2 / 3h-4 for the same effect).
ORDER_NOISE = 1.6e-14
STEP_BOUND = 1000 * ORDER_NOISE
SWEEP_EDGE = 0.5   # the size sweep: coarse maps step more than 5 % in depth from pixel to pixel on the side walls


def solving_cases():
    """(Ha, Wa, Hb, Wb) of the size sweep whose first evaluation can be solved"""
    out = []
    for (Ha, Wa), sizes in (((96, 128), SIZES_B), ((24, 32), SIZES_B_SMALL_A)):
        for (Hb, Wb) in sizes:
            sc = scene(Ha, Wa, Hb, Wb, 3, SWEEP_EDGE)
            e = evaluate(sc['maps_a'], sc['K_a'], sc['maps_b'], sc['R0'], sc['t0'])
            if step(e['sums'])[0] == 0:
                out.append((Ha, Wa, Hb, Wb))
    return out


def order_noise(sc, **kw):
    out = []
    for rev in (False, True):
        e = evaluate(sc['maps_a'], sc['K_a'], sc['maps_b'], sc['R0'], sc['t0'], reverse=rev, **kw)
        reason, d, _, _ = step(e['sums'])
        assert reason == 0
        out.append(apply(sc['R0'], sc['t0'], d))
    (Ra, ta), (Rb, tb) = out
    return pose_distance(Ra, ta, Rb, tb)
