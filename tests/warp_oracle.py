"""numpy restatement of cotr_warp_map / cotr_warp_perspective and nothing else: coordinates and sums in int64,
the perspective positions in float64 in the stated order of operations.  The GPU tests ask the library to be identical to
it.  ``exact`` is the bilinear value in float64 from the unquantised coordinates with the gradients of its cell: the
independent bound |restatement - exact| <= 0.5 + (Gx + Gy) / 64 (tests/test_warp_cpu.py)."""
import numpy as np

OUTSIDE = -(1 << 31)        # a fixed-point coordinate whose taps are outside every source
LIMIT = float(1 << 26)      # |v| >= 2^26 px, or a non-finite v: all four taps outside
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def fix(v):
    """map values -> X = rint(v * 32) as int64 (ties to even), OUTSIDE where v is not usable.  float64 is rounded to float32
    first; v * 32 is exact in float32, and is formed in float64 here"""
    with np.errstate(over='ignore', invalid='ignore'):
        v = np.asarray(v).astype(np.float32)
        ok = np.abs(v) < LIMIT                                   # False for NaN and inf
    X = np.rint(np.where(ok, v, 0).astype(np.float64) * 32.0).astype(np.int64)
    return np.where(ok, X, OUTSIDE)


def sample(src, X, Y, background=None):
    """src uint8 [Hs, Ws(, C)], X / Y int64 [Hd, Wd] in 1/32 px -> (dst uint8 [Hd, Wd(, C)], cover bool [Hd, Wd])"""
    src = np.asarray(src)
    s3 = src if src.ndim == 3 else src[..., None]
    Hs, Ws, C = s3.shape
    ix, iy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31              # >> floors, & 31 is the non-negative remainder
    acc = np.zeros(X.shape + (C,), np.int64)
    cover = np.zeros(X.shape, bool)
    for dy, dx, w in ((0, 0, (32 - fx) * (32 - fy)), (0, 1, fx * (32 - fy)), (1, 0, (32 - fx) * fy), (1, 1, fx * fy)):
        x, y = ix + dx, iy + dy
        inside = (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
        p = s3[np.clip(y, 0, Hs - 1), np.clip(x, 0, Ws - 1)].astype(np.int64) * inside[..., None]   # the border value is 0
        acc += w[..., None] * p
        cover |= inside & (w != 0)
    dst = ((acc + 512) >> 10).astype(np.uint8)
    if background is not None:
        bg = np.asarray(background)
        dst = np.where(cover[..., None], dst, bg if bg.ndim == 3 else bg[..., None])
    return (dst if src.ndim == 3 else dst[..., 0]), cover


def remap(src, map_, background=None):
    """cotr_warp_map: map_ [Hd, Wd, 2] = (x, y), float32 or float64"""
    map_ = np.asarray(map_)
    return sample(src, fix(map_[..., 0]), fix(map_[..., 1]), background)


def perspective_coords(Minv, Hd, Wd):
    """(X, Y) int64 [Hd, Wd] of cotr_warp_perspective: Minv is destination -> source; numpy evaluates every product and sum
    separately (no fused multiply-add), in the order written"""
    m = np.asarray(Minv, dtype=np.float64).reshape(9)
    x = np.arange(Wd, dtype=np.float64)[None, :]
    y = np.arange(Hd, dtype=np.float64)[:, None]
    with np.errstate(all='ignore'):
        W = (m[6] * x + m[7] * y) + m[8]
        horizon = W == 0
        W = np.where(horizon, 0.0, 32.0 / np.where(horizon, 1.0, W))
        out = []
        for a, b, c in ((m[0], m[1], m[2]), (m[3], m[4], m[5])):
            f = ((a * x + b * y) + c) * W
            bad = horizon | np.isnan(f)
            X = np.rint(np.clip(np.where(bad, 0.0, f), float(INT_MIN), float(INT_MAX))).astype(np.int64)
            out.append(np.where(bad, OUTSIDE, X))
    return out


def warp_perspective(src, Minv, Hd, Wd, background=None):
    X, Y = perspective_coords(Minv, Hd, Wd)
    return sample(src, X, Y, background)


def exact(src, map_):
    """the bilinear value from the UNQUANTISED float32 coordinates in float64, border 0 -> (value float64 [Hd, Wd, C],
    Gx, Gy float64 [Hd, Wd, C]: the largest absolute differences between horizontally / vertically adjacent taps of the
    cell floor(v) that holds the coordinate, border taps included).  A coordinate the rule does not use (non-finite,
    |v| >= 2^26) has all its taps outside: value 0, G 0."""
    src = np.asarray(src)
    s3 = src if src.ndim == 3 else src[..., None]
    Hs, Ws, C = s3.shape
    with np.errstate(over='ignore', invalid='ignore'):
        v = np.asarray(map_).astype(np.float32)
        ok = (np.abs(v) < LIMIT).all(axis=-1)
    v = np.where(ok[..., None], v, -4.0).astype(np.float64)     # (-4, -4): every tap outside
    x0, y0 = np.floor(v[..., 0]), np.floor(v[..., 1])
    a, b = (v[..., 0] - x0)[..., None], (v[..., 1] - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def tap(dy, dx):
        x, y = x0 + dx, y0 + dy
        inside = (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
        return s3[np.clip(y, 0, Hs - 1), np.clip(x, 0, Ws - 1)].astype(np.float64) * inside[..., None]
    t00, t01, t10, t11 = tap(0, 0), tap(0, 1), tap(1, 0), tap(1, 1)
    value = (t00 * (1 - a) + t01 * a) * (1 - b) + (t10 * (1 - a) + t11 * a) * b
    Gx = np.maximum(np.abs(t01 - t00), np.abs(t11 - t10))
    Gy = np.maximum(np.abs(t10 - t00), np.abs(t11 - t01))
    return value, Gx, Gy


# ---- inputs shared by the CPU tests, the GPU tests and tools/bench_warp.py ---------------------------------------------------
def image(H, W, C, seed):
    """a smooth picture plus noise, so that neighbouring taps differ by a few and by many grey levels"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 127 + 90 * np.sin(xx / 17.0 + seed)[..., None] * np.cos(yy[..., None] / 23.0 + np.arange(C))
    return np.clip(base + rng.integers(-30, 31, (H, W, C)), 0, 255).astype(np.uint8)


def identity_map(Hd, Wd, dtype=np.float32):
    yy, xx = np.mgrid[0:Hd, 0:Wd]
    return np.stack([xx, yy], -1).astype(dtype)


def smooth_map(Hd, Wd, Hs, Ws, seed, dtype=np.float32, margin=0.0):
    """a smooth random warp of the destination grid into the source (sums of a few low-frequency waves); margin > 0 pushes
    that fraction of the range outside the source on every side"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:Hd, 0:Wd]
    u, v = xx / max(Wd - 1, 1), yy / max(Hd - 1, 1)
    ph = rng.uniform(0, 2 * np.pi, 4)
    du = 0.03 * np.sin(2 * np.pi * (1.5 * v + 0.5 * u) + ph[0]) + 0.02 * np.cos(2 * np.pi * 2.5 * u + ph[1])
    dv = 0.03 * np.cos(2 * np.pi * (1.5 * u - 0.5 * v) + ph[2]) + 0.02 * np.sin(2 * np.pi * 2.5 * v + ph[3])
    x = ((u + du) * (1 + 2 * margin) - margin) * (Ws - 1)
    y = ((v + dv) * (1 + 2 * margin) - margin) * (Hs - 1)
    return np.stack([x, y], -1).astype(dtype)


def demo_corners(Hb, Wb):
    """four corners in an Hb x Wb image in the proportions of demo_homography.py:36-39 (a 3000 x 4000 photograph)"""
    c = np.array([[932, 1025], [2469, 901], [908, 2927], [2436, 3080]], np.float64) / [3000.0, 4000.0]
    return (c * [Wb, Hb]).astype(np.float32)
