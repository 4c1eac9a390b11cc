"""The rule of cotr_detect_keypoints (include/cotr_hip.h) restated in numpy int64 / float64, one image at a
time and one step after the other, and the generators the keypoint tests share.  Nothing here is tuned to the device: every
step is the sentence of the rule it stands for."""
import numpy as np

SCORES = ('min_eig', 'harris')


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def sobel(img):
    """uint8 [H,W] -> (Ix, Iy) int64 [H,W]: 1-2-1 Sobel, right minus left and below minus above; 0 on the outermost ring, whose
    support leaves the image (no key reads it)"""
    I = img.astype(np.int64)
    Ix, Iy = np.zeros_like(I), np.zeros_like(I)
    Ix[1:-1, 1:-1] = (I[:-2, 2:] + 2 * I[1:-1, 2:] + I[2:, 2:]) - (I[:-2, :-2] + 2 * I[1:-1, :-2] + I[2:, :-2])
    Iy[1:-1, 1:-1] = (I[2:, :-2] + 2 * I[2:, 1:-1] + I[2:, 2:]) - (I[:-2, :-2] + 2 * I[:-2, 1:-1] + I[:-2, 2:])
    return Ix, Iy


def box_sum(v, r):
    """int64 [H,W] -> the sum over the (2r+1)^2 box around every pixel, zeros outside the image"""
    H, W = v.shape
    p = np.zeros((H + 2 * r, W + 2 * r), np.int64)
    p[r:r + H, r:r + W] = v
    out = np.zeros_like(v)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out += p[dy:dy + H, dx:dx + W]
    return out


def tensor(img, r):
    Ix, Iy = sobel(img)
    return box_sum(Ix * Ix, r), box_sum(Ix * Iy, r), box_sum(Iy * Iy, r)


def keys_of(img, mask, score, r, border):
    """-> (key int64 [H,W], S float64 [H,W]: the score map, S where key > 0 and 0 elsewhere)"""
    H, W = img.shape
    a, b, c = tensor(img, r)
    if score == 'harris':
        key = 64 * (a * c - b * b) - 3 * (a + c) * (a + c)
        S = key.astype(np.float64)
    else:
        S = (a + c).astype(np.float64) - np.sqrt(((a - c) * (a - c) + 4 * b * b).astype(np.float64))
        key = np.where(S > 0, S, 0.0).view(np.int64)
    key = np.where(S > 0, key, 0)
    m = max(border, r + 1)
    inner = np.zeros((H, W), bool)
    inner[m:H - m, m:W - m] = True
    key = np.where(inner, key, 0)
    if mask is not None:
        key = np.where(mask != 0, key, 0)
    return key, np.where(key > 0, S, 0.0)


def candidates(key, S, R, min_score):
    """-> bool [H,W]"""
    H, W = key.shape
    p = np.zeros((H + 2 * R, W + 2 * R), np.int64)
    p[R:R + H, R:R + W] = key
    ok = (key > 0) & (S >= min_score)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dy == 0 and dx == 0:
                continue
            q = p[R + dy:R + dy + H, R + dx:R + dx + W]
            behind = dy > 0 or (dy == 0 and dx > 0)      # q has the larger raster index
            ok &= (q <= key) if behind else (q < key)
    return ok


def offset(sm, s0, sp):
    den = (sm - s0) + (sp - s0)
    with np.errstate(divide='ignore', invalid='ignore'):
        off = np.where(den < 0, 0.5 * (sm - sp) / den, 0.0)
    return np.clip(off, -0.5, 0.5)


def detect_one(img, mask=None, score='min_eig', r=2, R=4, border=0, quality=0.01, min_score=0.0, K=2048):
    """-> (xy float64 [K,2], S float64 [K], pixel int32 [K], info int32 [4])"""
    H, W = img.shape
    assert img.dtype == np.uint8 and score in SCORES and min(H, W) >= 2 * max(border, r + 1) + 1
    key, S = keys_of(img, mask, score, r, border)
    ys, xs = np.nonzero(candidates(key, S, R, min_score))
    xy, s_out, pixel, info = np.full((K, 2), np.nan), np.full(K, np.nan), np.full(K, -1, np.int32), np.zeros(4, np.int32)
    info[0] = len(ys)
    if len(ys) == 0:
        return xy, s_out, pixel, info
    ck, cs, idx = key[ys, xs], S[ys, xs], ys * W + xs
    alive = cs >= np.float64(quality) * cs.max()
    ys, xs, ck, cs, idx = ys[alive], xs[alive], ck[alive], cs[alive], idx[alive]
    order = np.lexsort((idx, -ck))
    info[1] = len(order)
    order = order[:K]
    k = info[2] = len(order)
    ys, xs = ys[order], xs[order]
    xy[:k, 0] = xs + offset(S[ys, xs - 1], S[ys, xs], S[ys, xs + 1])
    xy[:k, 1] = ys + offset(S[ys - 1, xs], S[ys, xs], S[ys + 1, xs])
    s_out[:k], pixel[:k] = cs[order], idx[order]
    return xy, s_out, pixel, info


def detect(images, mask=None, score='min_eig', r=2, R=4, border=0, quality=0.01, min_score=0.0, K=2048):
    """images uint8 [n,H,W] -> dict(keypoints [n,K,2], scores [n,K], pixel [n,K], info [n,4])"""
    rows = [detect_one(im, None if mask is None else mask[i], score, r, R, border, quality, min_score, K) for i, im in enumerate(images)]
    return dict(keypoints=np.stack([x[0] for x in rows]), scores=np.stack([x[1] for x in rows]), pixel=np.stack([x[2] for x in rows]),
                info=np.stack([x[3] for x in rows]))


# ---- generators ---------------------------------------------------------------------------------------------------------------
def noise(n, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, H, W), dtype=np.uint8)


def textured(n, H, W, seed):
    """noise over smooth blobs: a few strong corners and many weak ones, so that the quality test and K both cut somewhere"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        img = rng.integers(0, 40, size=(H, W)).astype(np.int64) + 40
        for _ in range(max(1, H * W // 300)):
            y, x, h, w = rng.integers(0, H), rng.integers(0, W), rng.integers(2, 9), rng.integers(2, 9)
            img[y:y + h, x:x + w] = rng.integers(0, 256)
        out[i] = np.clip(img + rng.integers(-3, 4, size=(H, W)), 0, 255)
    return out


def random_mask(n, H, W, seed):
    rng = np.random.default_rng(seed)
    m = (rng.random((n, H, W)) < 0.8).astype(np.uint8)
    m[:, :, W // 2:W // 2 + 2] = 0
    return m * rng.integers(1, 256, size=(n, H, W), dtype=np.uint8)     # any value that is not 0 counts


def checkerboard(H, W, square, lo=0, hi=255):
    y, x = np.mgrid[:H, :W]
    return np.where(((y // square) + (x // square)) % 2 == 0, lo, hi).astype(np.uint8)


def rectangles(seed, H=96, W=128, cell=32, background=60, noise_amp=3):
    """The ground-truth scene: background 60, a grid of 32-pixel cells with one axis-aligned rectangle of side 10 to 15 and
    level 120 to 250 in each, uniform noise of +-3 -> (uint8 [H,W], corners float64 [4 * cells, 2] as (x, y): the corner
    pixel of the rectangle, i.e. its outermost pixel along both axes)"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), background, np.int64)
    corners = []
    for cy in range(H // cell):
        for cx in range(W // cell):
            h, w = rng.integers(10, 16, size=2)
            y = cy * cell + rng.integers(8, cell - 8 - h + 1)
            x = cx * cell + rng.integers(8, cell - 8 - w + 1)
            img[y:y + h, x:x + w] = rng.integers(120, 251)
            corners += [(x, y), (x + w - 1, y), (x, y + h - 1), (x + w - 1, y + h - 1)]
    img = img + rng.integers(-noise_amp, noise_amp + 1, size=(H, W))
    return np.clip(img, 0, 255).astype(np.uint8), np.array(corners, np.float64)


def corner_report(xy, corners):
    """-> (the distance from every corner to its nearest keypoint, the distance from every keypoint to its nearest corner)"""
    d = np.linalg.norm(xy[:, None, :] - corners[None, :, :], axis=2)
    return d.min(axis=0), d.min(axis=1)
