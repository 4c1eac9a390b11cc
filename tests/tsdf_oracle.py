"""numpy float64 restatement of the TSDF volume (cotr_amd/csrc/tsdf.hip): the integration of posed depth
maps and the raycast of the volume, with the products and sums in the device's order, so volumes, depth maps and normals can be
compared bit for bit.  Both flag the elements that sit within NEAR of a decision: a projection at a rounding tie, Y_z at 0,
sdf at -trunc (voxels); a grid coordinate at an integer, a sample value at 0 (pixels, over the samples their walk reaches).
The raycast takes every sample 0 .. S of every ray as the rule states it: it skips nothing.

numpy only.  Test infrastructure."""
import functools

import numpy as np

from tests import icp_oracle as io
from tests import pnp_oracle as po

NEAR = 1e-9


def fresh(dims):
    """dims (Nx, Ny, Nz) -> (tsdf = 1, weight = 0), float32 [Nz, Ny, Nx]"""
    Nx, Ny, Nz = dims
    return np.ones((Nz, Ny, Nx), np.float32), np.zeros((Nz, Ny, Nx), np.float32)


# ---- integration ----------------------------------------------------------------------------------------------------------
def integrate(tsdf, weight, origin, voxel, trunc, depths, Ks, c2ws, found=None, weights=None, max_weight=64.0):
    """-> dict(tsdf, weight: new arrays, info int32 [n, 4], near bool [Nz, Ny, Nx])"""
    T, Wt = np.array(tsdf, np.float32), np.array(weight, np.float32)
    Nz, Ny, Nx = T.shape
    o = np.asarray(origin, np.float64)
    kk, jj, ii = np.meshgrid(np.arange(Nz, dtype=np.float64), np.arange(Ny, dtype=np.float64), np.arange(Nx, dtype=np.float64), indexing='ij')
    P = [o[0] + voxel * ii, o[1] + voxel * jj, o[2] + voxel * kk]
    n = len(depths)
    info = np.zeros((n, 4), np.int32)
    near = np.zeros(T.shape, bool)
    for c in range(n):
        if found is not None and found[c] == 0:
            continue
        depth = np.asarray(depths[c], np.float32)
        H, W = depth.shape
        m = np.asarray(c2ws[c], np.float64).reshape(4, 4)
        fx, s, cx, fy, cy = po.cam(Ks[c])
        w = 1.0 if weights is None else float(weights[c])
        with np.errstate(all='ignore'):
            D = [P[a] - m[a, 3] for a in range(3)]
            Y = [(m[0, a] * D[0] + m[1, a] * D[1]) + m[2, a] * D[2] for a in range(3)]
            g = Y[2] > 0
            near |= np.abs(Y[2]) <= NEAR * np.sqrt(Y[0] * Y[0] + Y[1] * Y[1] + Y[2] * Y[2])
            xn, yn = Y[0] / Y[2], Y[1] / Y[2]
            u, v = (fx * xn + s * yn) + cx, fy * yn + cy
            near |= g & ((np.abs(u - np.floor(u) - 0.5) <= NEAR) | (np.abs(v - np.floor(v) - 0.5) <= NEAR))
            ru, rv = np.rint(u), np.rint(v)
            g = g & (ru >= 0) & (ru < W) & (rv >= 0) & (rv < H)
            z = depth[np.where(g, rv, 0).astype(np.int64), np.where(g, ru, 0).astype(np.int64)].astype(np.float64)
            valid = g & (z > 0) & (z < np.inf)
            sdf = z - Y[2]
            near |= valid & (np.abs(sdf + trunc) <= NEAR * trunc)
            upd = valid & ~(sdf < -trunc)
            d = np.minimum(1.0, sdf / trunc)
            Td, Wd = T.astype(np.float64), Wt.astype(np.float64)
            Tn = ((Td * Wd + d * w) / (Wd + w)).astype(np.float32)
            Wn = np.minimum(Wd + w, max_weight).astype(np.float32)
        T, Wt = np.where(upd, Tn, T), np.where(upd, Wn, Wt)
        info[c] = 1, int(upd.sum()), int(valid.sum()), 0
    return dict(tsdf=T, weight=Wt, info=info, near=near)


def integrate_voxel(t, w, i, j, k, origin, voxel, trunc, depth, K, c2w, obs_weight=1.0, max_weight=64.0):
    """one voxel, one capture, scalar by scalar as the rule reads -> (tsdf, weight) float32"""
    t, w = np.float32(t), np.float32(w)
    m = np.asarray(c2w, np.float64).reshape(4, 4)
    fx, s, cx, fy, cy = (float(x) for x in po.cam(K))
    P = [float(origin[0]) + voxel * float(i), float(origin[1]) + voxel * float(j), float(origin[2]) + voxel * float(k)]
    D = [P[a] - float(m[a, 3]) for a in range(3)]
    Y = [(float(m[0, a]) * D[0] + float(m[1, a]) * D[1]) + float(m[2, a]) * D[2] for a in range(3)]
    if not Y[2] > 0:
        return t, w
    xn, yn = Y[0] / Y[2], Y[1] / Y[2]
    u, v = float(np.rint((fx * xn + s * yn) + cx)), float(np.rint(fy * yn + cy))
    H, W = depth.shape
    if not (0 <= u < W and 0 <= v < H):
        return t, w
    z = float(depth[int(v), int(u)])
    if not (z > 0 and z < np.inf):
        return t, w
    sdf = z - Y[2]
    if sdf < -trunc:
        return t, w
    d = min(1.0, sdf / trunc)
    return np.float32((float(t) * float(w) + d * obs_weight) / (float(w) + obs_weight)), np.float32(min(float(w) + obs_weight, max_weight))


# ---- the raycast ----------------------------------------------------------------------------------------------------------
def sample(tsdf, weight, origin, voxel, p):
    """p [..., 3] -> (valid, f (0 where invalid), a grid coordinate within NEAR of an integer at a point in or on the box: a point
    clearly outside on another axis is invalid whichever way that coordinate falls)"""
    Nz, Ny, Nx = tsdf.shape
    N = np.array([Nx, Ny, Nz], np.float64)
    with np.errstate(all='ignore'):
        g = (p - np.asarray(origin, np.float64)) / voxel
        i0 = np.floor(g)
        inb = ((i0 >= 0) & (i0 <= N - 2)).all(-1)
        r = np.rint(g)
        at_int = ((np.abs(g - r) <= NEAR) & (r >= 0) & (r <= N - 1)).any(-1) & ((g >= -NEAR) & (g <= N - 1 + NEAR)).all(-1)
        b = np.where(inb[..., None], i0, 0).astype(np.int64)
        fr = g - i0
    x, y, z = b[..., 0], b[..., 1], b[..., 2]
    corner = lambda a, dx, dy, dz: a[z + dz, y + dy, x + dx]   # noqa: E731
    seen = np.ones(inb.shape, bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                seen &= corner(weight, dx, dy, dz) > 0
    a = {(dx, dy, dz): corner(tsdf, dx, dy, dz).astype(np.float64) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
    with np.errstate(all='ignore'):
        c = {(dy, dz): a[0, dy, dz] + fr[..., 0] * (a[1, dy, dz] - a[0, dy, dz]) for dy in (0, 1) for dz in (0, 1)}
        e = {dz: c[0, dz] + fr[..., 1] * (c[1, dz] - c[0, dz]) for dz in (0, 1)}
        f = e[0] + fr[..., 2] * (e[1] - e[0])
    valid = inb & seen
    return valid, np.where(valid, f, 0.0), at_int


def steps(near, far, step):
    return int(np.ceil((far - near) / step))


def directions(K, c2w, shape):
    """-> (the world directions [H, W, 3], the z of the camera-frame directions [H, W])"""
    H, W = shape
    m = np.asarray(c2w, np.float64).reshape(4, 4)
    fx, s, cx, fy, cy = po.cam(K)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    yn = (ys - cy) / fy
    xn = (xs - cx - s * yn) / fx
    norm = np.sqrt((xn * xn + yn * yn) + 1.0)
    dc = [xn / norm, yn / norm, 1.0 / norm]
    return np.stack([(m[a, 0] * dc[0] + m[a, 1] * dc[1]) + m[a, 2] * dc[2] for a in range(3)], -1), dc[2]


def raycast(tsdf, weight, origin, voxel, K, c2w, shape, near, far, step, normals=False, found=None):
    """-> dict(depth float32 [H, W], normals float64 [H, W, 3] (with ``normals``), info int32 [4], near bool [H, W], samples: the
    samples taken by rays still walking)"""
    H, W = shape
    if found is not None and found[0] == 0:
        return dict(depth=np.zeros((H, W), np.float32), normals=np.zeros((H, W, 3)) if normals else None, info=np.zeros(4, np.int32),
                    near=np.zeros((H, W), bool), samples=0)
    m = np.asarray(c2w, np.float64).reshape(4, 4)
    t = m[:3, 3]
    dw, dcz = directions(K, c2w, shape)
    state = np.zeros((H, W), np.int8)
    prev_ok, prev_f, s_hit, flag = np.zeros((H, W), bool), np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W), bool)
    taken = 0
    for k in range(steps(near, far, step) + 1):
        s = near + float(k) * step
        valid, f, at_int = sample(tsdf, weight, origin, voxel, t + s * dw)
        alive = state == 0
        taken += int(alive.sum())
        flag |= alive & (at_int | (valid & (np.abs(f) <= NEAR)))
        both = alive & valid & prev_ok
        hit, back = both & (prev_f > 0) & (f <= 0), both & (prev_f < 0) & (f > 0)
        with np.errstate(all='ignore'):
            s_hit = np.where(hit, (near + float(k - 1) * step) + step * (prev_f / (prev_f - f)), s_hit)
        state[hit], state[back] = 1, 2
        prev_ok, prev_f = valid, f
        if not (state == 0).any():
            break
    hit = state == 1
    out = dict(depth=np.where(hit, s_hit * dcz, 0.0).astype(np.float32), normals=None, near=flag, samples=taken,
               info=np.array([1, int(hit.sum()), int((state == 2).sum()), 0], np.int32))
    if normals:
        p = t + s_hit[..., None] * dw
        G, ok = [], hit.copy()
        for a in range(3):
            e = np.zeros(3)
            e[a] = voxel
            (vp, fp, ip), (vm, fm, im) = sample(tsdf, weight, origin, voxel, p + e), sample(tsdf, weight, origin, voxel, p - e)
            ok &= vp & vm
            out['near'] = out['near'] | (hit & (ip | im))
            G.append(fp - fm)
        with np.errstate(all='ignore'):
            L = np.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
            ok &= L > 0
            nrm = np.stack([((m[0, a] * G[0] + m[1, a] * G[1]) + m[2, a] * G[2]) / L for a in range(3)], -1)
        nrm[~ok] = np.nan
        out['normals'] = nrm
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------------
ORIGIN_64, VOXEL_64 = (-3.2, -3.2, 1.0), 0.1   # the 64^3 volume around the three-plane corner of icp_oracle


def small_origin(dims, voxel=VOXEL_64):
    """a small volume around the point (0, 0, 6) of the corner's far wall, off the round numbers"""
    Nx, Ny, Nz = dims
    return (0.013 - voxel * (Nx - 1) / 2, 0.007 - voxel * (Ny - 1) / 2, 6.021 - voxel * (Nz - 1) / 2)


def crossings():
    """a volume observed everywhere whose value, along z, falls through 0 at z = 1.55, rises through it at 2.35 and falls again at
    3.15, and a 5 x 5 camera looking along z from the world's origin -> dict(tsdf, weight, origin, voxel, dims, K, c2w, shape)"""
    dims, voxel, origin = (6, 6, 40), 0.1, (-0.25, -0.25, 0.0)
    z = origin[2] + voxel * np.arange(dims[2])
    tsdf = np.broadcast_to(np.where(z < 1.95, 1.55 - z, np.where(z < 2.75, z - 2.35, 3.15 - z))[:, None, None], (40, 6, 6)).astype(np.float32)
    K = np.array([[200.0, 0.0, 2.0], [0.0, 200.0, 2.0], [0.0, 0.0, 1.0]])
    return dict(tsdf=np.ascontiguousarray(tsdf), weight=np.ones_like(tsdf), origin=origin, voxel=voxel, dims=dims, K=K, c2w=np.eye(4), shape=(5, 5))


@functools.lru_cache(maxsize=None)
def captures(H, W, n=2):
    """n captures of the corner scene at H x W: the two cameras of the scene in turn -> (depths float32 [n, H, W], Ks [n, 3, 3],
    c2ws [n, 4, 4]); read only"""
    sc = io.scene(H, W, H, W, 3)
    pick = [('depth_a', 'K_a', 'c2w_a'), ('depth_b', 'K_b', 'c2w_b')]
    rows = [pick[c % 2] for c in range(n)]
    return (np.stack([sc[d] for d, _, _ in rows]), np.stack([sc[k] for _, k, _ in rows]), np.stack([sc[m] for _, _, m in rows]))


@functools.lru_cache(maxsize=None)
def fused(H=48, W=64, dims=(64, 64, 64), origin=ORIGIN_64, voxel=VOXEL_64, trunc=None):
    """the corner's two captures fused into a fresh volume by the restatement -> dict(tsdf, weight, info, near, origin, voxel,
    trunc, dims); read only"""
    trunc = 3 * voxel if trunc is None else trunc
    depths, Ks, c2ws = captures(H, W)
    r = integrate(*fresh(dims), origin, voxel, trunc, depths, Ks, c2ws)
    r.update(origin=origin, voxel=voxel, trunc=trunc, dims=dims)
    return r


def share(flags):
    return float(np.asarray(flags).mean())
