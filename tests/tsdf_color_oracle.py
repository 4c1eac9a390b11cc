"""numpy float64 restatement of the colour volume (cotr_amd/csrc/tsdf.hip): the integration of posed images,
the colour at world points and the colour of a depth map, with the products and sums in the device's order, so colour volumes
and bytes can be compared bit for bit.  Each flags the elements that sit within NEAR of a decision: what
``tsdf_oracle.integrate`` flags (a projection at a rounding tie, Y_z at 0, sdf at -trunc) and sdf at +trunc (voxels); a grid
coordinate that misses 0 or N - 1 by at most NEAR, and a channel value at a .5 tie (points and pixels).  A coordinate that is
0 or N - 1 exactly is not flagged: that is the rule's own case (the faces belong to the box), every operation up to it is one
correctly rounded IEEE operation on both sides, and the tests put points there on purpose.

Also the textured images of ``tsdf_oracle.captures``: a smooth function of the world point, evaluated at every pixel's lifted
depth, so that the cameras agree on the colour of the surface.

numpy only.  Test infrastructure."""
import functools

import numpy as np

from tests import pnp_oracle as po
from tests import tsdf_oracle as to

NEAR = to.NEAR


def fresh(dims):
    """dims (Nx, Ny, Nz) -> color = 0, float32 [Nz, Ny, Nx, 4]"""
    Nx, Ny, Nz = dims
    return np.zeros((Nz, Ny, Nx, 4), np.float32)


# ---- integration ----------------------------------------------------------------------------------------------------------
def project(shape, origin, voxel, trunc, depth, K, c2w):
    """every voxel of a [Nz, Ny, Nx] volume into one capture, as ``tsdf_oracle.integrate`` states it -> (valid, sdf, the pixel's
    row and column (0 where not valid), its flags with sdf at +trunc added)"""
    Nz, Ny, Nx = shape
    o = np.asarray(origin, np.float64)
    kk, jj, ii = np.meshgrid(np.arange(Nz, dtype=np.float64), np.arange(Ny, dtype=np.float64), np.arange(Nx, dtype=np.float64), indexing='ij')
    P = [o[0] + voxel * ii, o[1] + voxel * jj, o[2] + voxel * kk]
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    m = np.asarray(c2w, np.float64).reshape(4, 4)
    fx, s, cx, fy, cy = po.cam(K)
    with np.errstate(all='ignore'):
        D = [P[a] - m[a, 3] for a in range(3)]
        Y = [(m[0, a] * D[0] + m[1, a] * D[1]) + m[2, a] * D[2] for a in range(3)]
        g = Y[2] > 0
        near = np.abs(Y[2]) <= NEAR * np.sqrt(Y[0] * Y[0] + Y[1] * Y[1] + Y[2] * Y[2])
        xn, yn = Y[0] / Y[2], Y[1] / Y[2]
        u, v = (fx * xn + s * yn) + cx, fy * yn + cy
        near |= g & ((np.abs(u - np.floor(u) - 0.5) <= NEAR) | (np.abs(v - np.floor(v) - 0.5) <= NEAR))
        ru, rv = np.rint(u), np.rint(v)
        g = g & (ru >= 0) & (ru < W) & (rv >= 0) & (rv < H)
        iy, ix = np.where(g, rv, 0).astype(np.int64), np.where(g, ru, 0).astype(np.int64)
        z = depth[iy, ix].astype(np.float64)
        valid = g & (z > 0) & (z < np.inf)
        sdf = z - Y[2]
        near |= valid & ((np.abs(sdf + trunc) <= NEAR * trunc) | (np.abs(sdf - trunc) <= NEAR * trunc))
    return valid, sdf, np.where(valid, iy, 0), np.where(valid, ix, 0), near


def integrate(color, origin, voxel, trunc, depths, images, Ks, c2ws, found=None, weights=None, max_weight=64.0):
    """-> dict(color: a new array, info int32 [n, 4], near bool [Nz, Ny, Nx], band: the voxels a capture coloured)"""
    C = np.array(color, np.float32)
    n = len(depths)
    info = np.zeros((n, 4), np.int32)
    near, band = np.zeros(C.shape[:3], bool), np.zeros(C.shape[:3], bool)
    for c in range(n):
        if found is not None and found[c] == 0:
            continue
        w = 1.0 if weights is None else float(weights[c])
        valid, sdf, iy, ix, flag = project(C.shape[:3], origin, voxel, trunc, depths[c], Ks[c], c2ws[c])
        near |= flag
        col = valid & ~(sdf < -trunc) & ~(sdf > trunc)
        p = np.asarray(images[c], np.uint8)[iy, ix].astype(np.float64)
        Wd = C[..., 3].astype(np.float64)
        total = Wd + w
        new = np.empty(C.shape, np.float32)
        for ch in range(3):
            new[..., ch] = ((C[..., ch].astype(np.float64) * Wd + p[..., ch] * w) / total).astype(np.float32)
        new[..., 3] = np.minimum(total, max_weight).astype(np.float32)
        C = np.where(col[..., None], new, C)
        band |= col
        info[c] = 1, int(col.sum()), int(valid.sum()), 0
    return dict(color=C, info=info, near=near, band=band)


def integrate_voxel(c4, i, j, k, origin, voxel, trunc, depth, image, K, c2w, obs_weight=1.0, max_weight=64.0):
    """one voxel, one capture, scalar by scalar as the rule reads -> (r, g, b, colour weight) float32 [4]"""
    c4 = np.array(c4, np.float32)
    m = np.asarray(c2w, np.float64).reshape(4, 4)
    fx, s, cx, fy, cy = (float(x) for x in po.cam(K))
    P = [float(origin[0]) + voxel * float(i), float(origin[1]) + voxel * float(j), float(origin[2]) + voxel * float(k)]
    D = [P[a] - float(m[a, 3]) for a in range(3)]
    Y = [(float(m[0, a]) * D[0] + float(m[1, a]) * D[1]) + float(m[2, a]) * D[2] for a in range(3)]
    if not Y[2] > 0:
        return c4
    xn, yn = Y[0] / Y[2], Y[1] / Y[2]
    u, v = float(np.rint((fx * xn + s * yn) + cx)), float(np.rint(fy * yn + cy))
    H, W = depth.shape
    if not (0 <= u < W and 0 <= v < H):
        return c4
    z = float(depth[int(v), int(u)])
    if not (z > 0 and z < np.inf):
        return c4
    sdf = z - Y[2]
    if sdf < -trunc or sdf > trunc:
        return c4
    Wc = float(c4[3])
    out = [np.float32((float(c4[ch]) * Wc + float(image[int(v), int(u), ch]) * obs_weight) / (Wc + obs_weight)) for ch in range(3)]
    return np.array(out + [np.float32(min(Wc + obs_weight, max_weight))], np.float32)


# ---- the colour at points and of a depth map ----------------------------------------------------------------------------------
def sample(color, origin, voxel, p):
    """p [..., 3] in the world frame -> (rgb uint8 [..., 3], valid bool [...], near bool [...])"""
    p = np.asarray(p, np.float64)
    Nz, Ny, Nx, _ = color.shape
    N = np.array([Nx, Ny, Nz], np.float64)
    with np.errstate(all='ignore'):
        q = (p - np.asarray(origin, np.float64)) / voxel
        inb = ((q >= 0) & (q <= N - 1)).all(-1)
        off = np.minimum(np.abs(q), np.abs(q - (N - 1)))
        near = ((off > 0) & (off <= NEAR)).any(-1) & ((q >= -NEAR) & (q <= N - 1 + NEAR)).all(-1)
        b = np.minimum(np.floor(q), N - 2)
        b = np.where(inb[..., None], b, 0.0)
        r = q - b
    x, y, z = (b[..., a].astype(np.int64) for a in range(3))
    S, C = np.zeros(inb.shape), [np.zeros(inb.shape) for _ in range(3)]
    with np.errstate(all='ignore'):
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    wx, wy, wz = (r[..., a] if d else 1.0 - r[..., a] for a, d in enumerate((dx, dy, dz)))
                    beta = (wx * wy) * wz
                    c = color[z + dz, y + dy, x + dx].astype(np.float64)
                    counts = inb & (c[..., 3] > 0)
                    S = S + np.where(counts, beta, 0.0)
                    C = [C[ch] + np.where(counts, beta * c[..., ch], 0.0) for ch in range(3)]
        valid = inb & (S > 0)
        val = np.stack([np.where(valid, C[ch] / S, 0.0) for ch in range(3)], -1)
        near |= valid & (np.abs(val - np.floor(val) - 0.5) <= NEAR).any(-1)
        rgb = np.clip(np.rint(val), 0.0, 255.0).astype(np.uint8)
    return rgb, valid, near


def sample_point(color, origin, voxel, p):
    """one point, scalar by scalar as the rule reads -> ((r, g, b), valid)"""
    Nz, Ny, Nx, _ = color.shape
    N = (Nx, Ny, Nz)
    q = [(float(p[a]) - float(origin[a])) / voxel for a in range(3)]
    if not all(0.0 <= q[a] <= N[a] - 1 for a in range(3)):   # NaN fails
        return (0, 0, 0), False
    b = [int(min(np.floor(q[a]), N[a] - 2)) for a in range(3)]
    r = [q[a] - b[a] for a in range(3)]
    S, C = 0.0, [0.0, 0.0, 0.0]
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                beta = ((r[0] if dx else 1.0 - r[0]) * (r[1] if dy else 1.0 - r[1])) * (r[2] if dz else 1.0 - r[2])
                c = color[b[2] + dz, b[1] + dy, b[0] + dx]
                if c[3] > 0:
                    S += beta
                    for ch in range(3):
                        C[ch] += beta * float(c[ch])
    if not S > 0:
        return (0, 0, 0), False
    return tuple(int(min(max(np.rint(C[ch] / S), 0.0), 255.0)) for ch in range(3)), True


def lift(depth, K, c2w):
    """the world point of every pixel of a depth map by the device's rule -> (p [H, W, 3], NaN where the depth is not finite and
    > 0, has bool [H, W])"""
    z = np.asarray(depth, np.float32).astype(np.float64)
    H, W = z.shape
    m = np.asarray(c2w, np.float64).reshape(4, 4)
    fx, s, cx, fy, cy = po.cam(K)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    with np.errstate(all='ignore'):
        has = (z > 0) & (z < np.inf)
        yn = (ys - cy) / fy
        xn = (xs - cx - s * yn) / fx
        Yx, Yy = xn * z, yn * z
        p = np.stack([((m[a, 0] * Yx + m[a, 1] * Yy) + m[a, 2] * z) + m[a, 3] for a in range(3)], -1)
    return np.where(has[..., None], p, np.nan), has


def color_map(color, origin, voxel, depth, K, c2w, found=None):
    """-> dict(rgb uint8 [H, W, 3], info int32 [4], near bool [H, W])"""
    H, W = np.shape(depth)
    if found is not None and found[0] == 0:
        return dict(rgb=np.zeros((H, W, 3), np.uint8), info=np.zeros(4, np.int32), near=np.zeros((H, W), bool))
    p, has = lift(depth, K, c2w)
    rgb, valid, near = sample(color, origin, voxel, p)
    return dict(rgb=rgb, info=np.array([1, int(valid.sum()), int(has.sum()), 0], np.int32), near=near & has)


# ---- scenes ---------------------------------------------------------------------------------------------------------------
# the largest change of each channel of ``texture`` per unit length: its amplitude times the length of its wave vector
GRADIENT = np.array([90.0 * np.hypot(1.3, 0.4), 80.0 * np.hypot(1.1, 0.3), 100.0 * np.hypot(0.7, 0.9)])


def texture(P):
    """a smooth colour on the 0 .. 255 scale at the world points P [..., 3]: a sine in each channel -> float64 [..., 3]"""
    P = np.asarray(P, np.float64)
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    return np.stack([128.0 + 90.0 * np.sin(1.3 * x + 0.4 * z), 120.0 + 80.0 * np.sin(1.1 * y - 0.3 * x + 1.0), 130.0 + 100.0 * np.sin(0.7 * z + 0.9 * y - 2.0)], -1)


@functools.lru_cache(maxsize=None)
def images(H, W, n=2):
    """the images of ``tsdf_oracle.captures(H, W, n)``: the texture at every pixel's lifted depth, rounded -> uint8 [n, H, W, 3],
    (0, 0, 0) where the depth is 0; read only"""
    depths, Ks, c2ws = to.captures(H, W, n)
    out = np.zeros((n, H, W, 3), np.uint8)
    for c in range(n):
        p, has = lift(depths[c], Ks[c], c2ws[c])
        out[c][has] = np.rint(texture(p[has])).astype(np.uint8)
    return out


# The weights of the two captures wherever a fused colour is sampled: with equal weights the mean of two bytes sits at a .5 tie
# for every odd sum, and a blend of such voxels within 1e-9 of one - a seventh of all mesh vertices would be flagged.  (4 a + 3 b) / 7
# is never k + 1 / 2: 8 a + 6 b is even and 14 k + 7 is odd.
FUSED_WEIGHTS = (1.0, 0.75)


@functools.lru_cache(maxsize=None)
def fused(H=48, W=64, dims=(64, 64, 64), origin=to.ORIGIN_64, voxel=to.VOXEL_64, weights=FUSED_WEIGHTS):
    """the colour of ``tsdf_oracle.fused`` with the same arguments: the corner's two textured captures, weighted ``weights``, in a
    fresh colour volume by the restatement -> dict(color, info, near, band); read only"""
    depths, Ks, c2ws = to.captures(H, W)
    return integrate(fresh(dims), origin, voxel, 3 * voxel, depths, images(H, W), Ks, c2ws, weights=weights)


def texture_error(rgb, valid, p):
    """|colour - texture| at the valid points -> (median, p90) per channel, float64 [2, 3]"""
    e = np.abs(rgb[valid].astype(np.float64) - texture(np.asarray(p)[valid]))
    return np.stack([np.median(e, 0), np.percentile(e, 90, 0)])


# ---- files ----------------------------------------------------------------------------------------------------------------
def read_ply(path):
    """a PLY file with colours back with numpy, from its own header -> (the names of the double columns, their rows [V, 3 or 6],
    colours uint8 [V, 3], faces [T, 3])"""
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    lines = raw[:end].decode('ascii').split('\n')
    assert lines[:2] == ['ply', 'format binary_little_endian 1.0']
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith('element')}
    props = [ln.split()[1:] for ln in lines if ln.startswith('property')]
    cols = [p[1] for p in props if p[0] == 'double']
    assert props[len(cols):] == [['uchar', 'red'], ['uchar', 'green'], ['uchar', 'blue'], ['list', 'uchar', 'int', 'vertex_indices']]
    v = np.frombuffer(raw, np.dtype([('d', '<f8', (len(cols),)), ('c', 'u1', (3,))]), counts['vertex'], end)
    f = np.frombuffer(raw, np.dtype([('n', 'u1'), ('v', '<i4', (3,))]), counts['face'], end + v.nbytes)
    assert end + v.nbytes + f.nbytes == len(raw) and (f['n'] == 3).all()
    return cols, v['d'], v['c'], f['v']
