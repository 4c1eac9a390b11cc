"""numpy restatement of cotr_rotate_captures / cotr_amd.data.rotate_captures, written from the rule of DESIGN.md 3l (OpenCV's
warpAffine about the centre, and the reference's rotate_camera_pose) and not from cotr_amd/data.py: the matrix in float64,
the fixed-point coordinates and sums in int64, the 8-bit bilinear body of tests/warp_oracle.py (the rule of 3i, which the
image half continues with).  The GPU tests ask the library to be identical to it.  ``exact`` is the bilinear value in float64
at the unquantised affine position with the tap differences of the 3 x 3 cells around it: the independent bound
|restatement - exact| <= 0.5 + (Gx + Gy) (1/64 + 1/1024) (tests/test_rotate_cpu.py).  Test infrastructure."""
import math

import numpy as np

from tests import warp_oracle as wo

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
POS_ERR = 1 / 64 + 1 / 1024        # px per axis: the +16 >> 5 step, and the two table roundings together


def matrix(shape_hw, angle):
    """m0..m5 float64, destination -> source: getRotationMatrix2D((W/2, H/2), angle, 1) as a 2 x 3 array, then warpAffine's
    inversion statement by statement"""
    H, W = shape_hw
    t = float(angle) * (math.pi / 180)
    alpha, beta = math.cos(t), math.sin(t)
    cx, cy = W / 2, H / 2
    M = np.array([[alpha, beta, (1 - alpha) * cx - beta * cy],
                  [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[1, 1] * D, M[0, 0] * D
    M[0, 0] = A11
    M[0, 1] *= -D
    M[1, 0] *= -D
    M[1, 1] = A22
    b1 = -M[0, 0] * M[0, 2] - M[0, 1] * M[1, 2]
    b2 = -M[1, 0] * M[0, 2] - M[1, 1] * M[1, 2]
    M[0, 2], M[1, 2] = b1, b2
    return M.reshape(6)


def _rint(v):
    """round half to even of a double, saturated to the int32 range, as int64"""
    return np.clip(np.rint(v), float(INT_MIN), float(INT_MAX)).astype(np.int64)


def sums(m, H, W):
    """(X0 + ad, Y0 + bd) int64 [H, W] in 1/1024 px; numpy evaluates every product and sum separately, in the order written"""
    m = np.asarray(m, dtype=np.float64).reshape(6)
    x = np.arange(W, dtype=np.float64)
    y = np.arange(H, dtype=np.float64)
    ad, bd = _rint((m[0] * x) * 1024.0), _rint((m[3] * x) * 1024.0)
    X0, Y0 = _rint(((m[1] * y) + m[2]) * 1024.0), _rint(((m[4] * y) + m[5]) * 1024.0)
    return X0[:, None] + ad[None, :], Y0[:, None] + bd[None, :]


def linear_coords(m, H, W):
    """the image's source position in 1/32 px, int64 [H, W] each"""
    SX, SY = sums(m, H, W)
    return (SX + 16) >> 5, (SY + 16) >> 5


def nearest_coords(m, H, W):
    """the depth's source pixel, int64 [H, W] each"""
    SX, SY = sums(m, H, W)
    return (SX + 512) >> 10, (SY + 512) >> 10


def warp_linear(image, m):
    """cv2.warpAffine(image, M, (W, H), flags=INTER_LINEAR) of a uint8 [H, W(, C)] image, border 0"""
    H, W = image.shape[:2]
    X, Y = linear_coords(m, H, W)
    return wo.sample(image, X, Y)[0]


def warp_nearest(depth, m):
    """cv2.warpAffine(depth, M, (W, H), flags=INTER_NEAREST) of a [H, W] map: the elements are copied, the border is 0"""
    depth = np.asarray(depth)
    H, W = depth.shape
    X, Y = nearest_coords(m, H, W)
    inside = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
    out = np.zeros_like(depth)
    out[inside] = depth[Y[inside], X[inside]]
    return out


def rotated_c2w(c2w, angle):
    """rotate_camera_pose without the float32 storage of its result"""
    r = angle / 180 * np.pi
    rz = np.eye(4)
    rz[0, 0], rz[0, 1], rz[1, 0], rz[1, 1] = np.cos(r), np.sin(r), -np.sin(r), np.cos(r)
    return np.linalg.inv(rz @ np.linalg.inv(np.asarray(c2w, dtype=np.float64)))


def rotate_capture(cap, angle):
    """(image, depth, K, c2w) of a capture tuple, rotated; angle 0 returns the capture's own arrays"""
    image, depth, K, c2w = cap
    if angle == 0:
        return type(cap)(image, depth, K, c2w) if hasattr(cap, '_fields') else (image, depth, K, c2w)
    m = matrix(depth.shape, angle)
    out = (None if image is None else warp_linear(image, m), warp_nearest(depth, m), K, rotated_c2w(c2w, angle))
    return type(cap)(*out) if hasattr(cap, '_fields') else out


def affine_position(m, H, W):
    """the unquantised source position (u, v) float64 [H, W] each"""
    m = np.asarray(m, dtype=np.float64).reshape(6)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]


def exact(image, m):
    """the bilinear value at the UNQUANTISED affine position in float64, border 0 -> (value float64 [H, W, C], Gx, Gy float64
    [H, W, C]: the largest absolute differences between horizontally / vertically adjacent taps over the 3 x 3 cells around the
    cell floor(u), floor(v) that holds the position, border taps included)"""
    src = np.asarray(image)
    s3 = src if src.ndim == 3 else src[..., None]
    H, W, C = s3.shape
    u, v = affine_position(m, H, W)
    x0, y0 = np.floor(u), np.floor(v)
    a, b = (u - x0)[..., None], (v - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def tap(dy, dx):
        x, y = x0 + dx, y0 + dy
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return s3[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.float64) * inside[..., None]
    t = {(dy, dx): tap(dy, dx) for dy in range(-1, 3) for dx in range(-1, 3)}        # the taps of the 3 x 3 cells
    value = (t[0, 0] * (1 - a) + t[0, 1] * a) * (1 - b) + (t[1, 0] * (1 - a) + t[1, 1] * a) * b
    Gx = np.maximum.reduce([np.abs(t[dy, dx + 1] - t[dy, dx]) for dy in range(-1, 3) for dx in range(-1, 2)])
    Gy = np.maximum.reduce([np.abs(t[dy + 1, dx] - t[dy, dx]) for dy in range(-1, 2) for dx in range(-1, 3)])
    return value, Gx, Gy


# ---- inputs shared by the CPU tests, the GPU tests and tools/bench_rotate.py --------------------------------------------------
def depth_map(H, W, seed, special=True):
    """a float32 depth map with holes; with ``special``, -0.0, a denormal, inf and a NaN with a payload among ordinary values"""
    rng = np.random.default_rng(seed)
    d = (rng.random((H, W), dtype=np.float32) * 10 + 1).astype(np.float32)
    d[rng.random((H, W)) < 0.1] = 0.0
    if special:
        bits = d.view(np.uint32).reshape(-1)
        words = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFF800001], dtype=np.uint32)
        where = rng.integers(0, bits.size, max(bits.size // 16, min(bits.size, len(words))))
        bits[where] = words[np.arange(where.size) % len(words)]
    return d


# ---- the property that pins both sign conventions (tests/test_rotate_cpu.py, tests/test_rotate_gpu.py) ------------------------
def property_case(angle, H=48, W=64):
    """a capture of constant depth 5 with a centred K (fx = fy) and a random pose, and the matrix of `angle`"""
    K = np.array([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1]])
    rng = np.random.default_rng(4)
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = q, rng.uniform(-3, 3, 3)
    from cotr_amd.data import Capture
    return Capture(None, np.full((H, W), 5.0, np.float32), K, c2w), matrix((H, W), angle)


def check_turns_the_same_way(cap, rot, m, rows=None):
    """the pose and the image turn the same way: un-project pixel (x, y) of the rotated capture `rot` with its pose, project it
    into the original `cap` (depth_corrs' oracle, or with `rows` the device's depth_corrs rows) - it lands on m . (x, y, 1).
    Every pixel with a depth takes part; what the reprojection keeps is decided exactly by the target's own inside rule."""
    from tests import dataset_oracle as do
    H, W = cap.depth.shape
    X, Y = nearest_coords(m, H, W)
    inside = ((X >= 0) & (X < W) & (Y >= 0) & (Y < H)).reshape(-1)
    depth = rot.depth.cpu().numpy() if hasattr(rot.depth, 'cpu') else np.asarray(rot.depth)
    assert np.array_equal(depth.reshape(-1) > 0, inside) and (depth.reshape(-1)[inside] == 5.0).all()
    assert 0 < inside.sum() < H * W
    r = do.reproject(depth, cap.depth, rot.K, rot.c2w, cap.K, cap.c2w)
    u, v = (p.reshape(-1) for p in affine_position(m, H, W))
    # (u, v) of EVERY pixel whose nearest-rule source lies inside, kept or not
    err = max(np.abs(r['uv'][inside, 0] - u[inside]).max(), np.abs(r['uv'][inside, 1] - v[inside]).max())
    print('largest |(u, v) - m . (x, y, 1)|', err)
    assert err <= 1e-9
    # kept: exactly those of them that the target's rule 0 <= u < W - 1, 0 <= v < H - 1 admits (a position within 1e-9 of one of
    # these borders - at 90 degrees whole rows sit on them - may fall either way)
    t = 1e-9
    must = inside & (u >= t) & (u < W - 1 - t) & (v >= t) & (v < H - 1 - t)
    may = inside & (u >= -t) & (u < W - 1 + t) & (v >= -t) & (v < H - 1 + t)
    keep = r['keep']
    assert (keep[must]).all() and not keep[~may].any() and must.sum() > H * W // 4
    if rows is not None:
        got_px = (rows[:, 1] * W + rows[:, 0]).astype(np.int64)
        assert np.array_equal(rows[:, :2], np.floor(rows[:, :2])) and np.array_equal(got_px, np.sort(got_px))
        dev_keep = np.zeros(H * W, bool)
        dev_keep[got_px] = True
        assert len(got_px) == dev_keep.sum() and dev_keep[must].all() and not dev_keep[~may].any()
        assert max(np.abs(rows[:, 2] - u[got_px]).max(), np.abs(rows[:, 3] - v[got_px]).max()) <= 1e-9
