"""A numpy float64 restatement of cotr_amd/scene.py, written from the rule of DESIGN.md 3k (not from the reference's code):
the world points of a capture, the overlap of an ordered pair of captures with the number of candidates that sit within
1e-9 of a decision, the neighbour pools and the draw.  ``canvas_rule`` selects the rule ('last' in source order) or one of
the two mistakes the fixtures must tell apart from it ('first' writer, 'minz' z-buffer).  Test infrastructure."""
import numpy as np

EPS = 1e-9
THRESH = 0.1          # VALID_NN_OVERLAPPING_THRESH of the reference


def _near(value, at):
    return np.abs(value - at) < EPS


def world_points(cap):
    """step 1 -> (xyz float32 [H W, 3] with NaN where invalid, valid bool [H W], ambiguous bool [H W]: c.z or w.w within
    EPS of 0, or a depth within EPS of 0 that is not 0 itself - a hole (z == 0 exactly) is an input, compared exactly by
    every implementation, and not a computed value near a decision)"""
    depth = np.asarray(cap.depth)
    H, W = depth.shape
    idx = np.arange(H * W)
    x, y = (idx % W).astype(np.float64), (idx // W).astype(np.float64)
    z = depth.reshape(-1).astype(np.float64)
    k = np.linalg.inv(np.asarray(cap.K, dtype=np.float64)).ravel()
    m = np.asarray(cap.c2w, dtype=np.float64).ravel()
    with np.errstate(all='ignore'):
        c0, c1, c2 = (((k[3 * i] * x + k[3 * i + 1] * y) + k[3 * i + 2]) * z for i in range(3))
        w = [((m[4 * i] * c0 + m[4 * i + 1] * c1) + m[4 * i + 2] * c2) + m[4 * i + 3] for i in range(4)]
        valid = (z > 0) & (c2 > 0) & (w[3] != 0)
        xyz = np.stack([w[0] / w[3], w[1] / w[3], w[2] / w[3]], 1).astype(np.float32)
        ambiguous = ((z != 0) & _near(z, 0)) | ((z > 0) & (_near(c2, 0) | _near(w[3], 0)))
    xyz[~valid] = np.nan
    return xyz, valid, ambiguous


def float32_ties(cap):
    """how many coordinates of the float64 world points sit within round-off (2^-50 relative) of the midpoint of two
    float32 values: there the float32 result would depend on the last bit of the float64 arithmetic"""
    depth = np.asarray(cap.depth)
    H, W = depth.shape
    idx = np.arange(H * W)
    x, y = (idx % W).astype(np.float64), (idx // W).astype(np.float64)
    z = depth.reshape(-1).astype(np.float64)
    k = np.linalg.inv(np.asarray(cap.K, dtype=np.float64)).ravel()
    m = np.asarray(cap.c2w, dtype=np.float64).ravel()
    with np.errstate(all='ignore'):
        c0, c1, c2 = (((k[3 * i] * x + k[3 * i + 1] * y) + k[3 * i + 2]) * z for i in range(3))
        w = [((m[4 * i] * c0 + m[4 * i + 1] * c1) + m[4 * i + 2] * c2) + m[4 * i + 3] for i in range(4)]
        valid = (z > 0) & (c2 > 0) & (w[3] != 0)
        w64 = np.stack([w[0] / w[3], w[1] / w[3], w[2] / w[3]], 1)[valid]
    f = w64.astype(np.float32).astype(np.float64)
    half_ulp = np.spacing(np.abs(f).astype(np.float32)).astype(np.float64) / 2
    return int((np.abs(np.abs(w64 - f) - half_ulp) < np.abs(w64) * 2.0 ** -50).sum())


def overlap(q, d, d_points=None, canvas_rule='last'):
    """steps 2-4 for the query capture q and the database capture d -> dict: 'ratio' float32, 'good', 'union' ints,
    'ambiguous' the number of candidates within EPS of a decision, 'canvas' float64 [Hq, Wq], 'hit' / 'contended' /
    'crowded' the number of canvas pixels on which at least one / more than one / at least four points land"""
    xyz, valid, amb1 = world_points(d) if d_points is None else d_points
    dq = np.asarray(q.depth)
    Hq, Wq = dq.shape
    P = np.matmul(np.asarray(q.K, dtype=np.float64), np.linalg.inv(np.asarray(q.c2w, dtype=np.float64))[0:3, :]).ravel()
    X = xyz.astype(np.float64)
    with np.errstate(all='ignore'):
        p0, p1, p2 = (((P[4 * i] * X[:, 0] + P[4 * i + 1] * X[:, 1]) + P[4 * i + 2] * X[:, 2]) + P[4 * i + 3] for i in range(3))
        front = valid & (p2 > 0)
        u, v = p0 / p2, p1 / p2
        keep = front & (u >= 0) & (u < Wq - 1) & (v >= 0) & (v < Hq - 1)
        amb = amb1 | (valid & _near(p2, 0))
        edge = _near(u, 0) | _near(u, Wq - 1) | _near(v, 0) | _near(v, Hq - 1)
        amb |= front & edge
        half = _near(u - np.floor(u), 0.5) | _near(v - np.floor(v), 0.5)
        amb |= keep & half
    src = np.flatnonzero(keep)
    ix = np.clip(np.rint(u[src]), 0, Wq - 1).astype(np.int64)
    iy = np.clip(np.rint(v[src]), 0, Hq - 1).astype(np.int64)
    cell = iy * Wq + ix
    pz = p2[src]
    if canvas_rule == 'last':
        order = np.arange(src.size)
    elif canvas_rule == 'first':
        order = np.arange(src.size)[::-1]
    elif canvas_rule == 'minz':
        order = np.argsort(-pz, kind='stable')           # the nearest point is written last
    else:
        raise ValueError(canvas_rule)
    # the point written LAST under `order` owns the pixel (np.maximum.at on the write rank: no reliance on what a fancy
    # assignment does with repeated indices)
    rank = np.empty(src.size, dtype=np.int64)
    rank[order] = np.arange(src.size)
    last = np.full(Hq * Wq, -1, dtype=np.int64)
    np.maximum.at(last, cell, rank)
    winner = np.where(last >= 0, order[np.maximum(last, 0)], -1) if src.size else last
    canvas = np.where(winner >= 0, pz[np.maximum(winner, 0)], 0.0) if src.size else np.zeros(Hq * Wq)
    qm = dq.reshape(-1) > 0
    rm = canvas > 0
    diff = np.abs(dq.reshape(-1).astype(np.float64) - canvas)
    good = int((qm & rm & (diff < 1.0)).sum())
    union = int((qm | rm).sum())
    # |depth - canvas| at 1.0 is a decision of every point that lands on a pixel with depth, winner or not under another rule
    landed_depth = dq.reshape(-1)[cell].astype(np.float64)
    amb_land = (landed_depth > 0) & _near(np.abs(landed_depth - pz), 1.0)
    ratio = np.float32(good / union) if union else np.float32(0.0)
    load = np.bincount(cell, minlength=Hq * Wq)
    return {'ratio': ratio, 'good': good, 'union': union, 'ambiguous': int(amb.sum()) + int(amb_land.sum()),
            'canvas': canvas.reshape(Hq, Wq), 'hit': int((load > 0).sum()), 'contended': int((load > 1).sum()),
            'crowded': int((load >= 4).sum())}


def overlap_pairs(caps, pairs, canvas_rule='last'):
    """-> (ratio float32 [n], counts int64 [n, 2] = (good, union), ambiguous int64 [n])"""
    points = {}
    ratio, counts, amb = [], [], []
    for q, d in np.asarray(pairs).reshape(-1, 2):
        if d not in points:
            points[d] = world_points(caps[d])
        r = overlap(caps[q], caps[d], points[d], canvas_rule)
        ratio.append(r['ratio'])
        counts.append((r['good'], r['union']))
        amb.append(r['ambiguous'])
    return np.array(ratio, dtype=np.float32), np.array(counts, dtype=np.int64).reshape(-1, 2), np.array(amb, dtype=np.int64)


def overlap_matrix(caps, covisible=None, canvas_rule='last'):
    """-> (dist float32 [N, N], ambiguous int64 [N, N]); cells where covisible is False are 0 and not computed"""
    n = len(caps)
    cov = np.ones((n, n), dtype=bool) if covisible is None else np.asarray(covisible, dtype=bool)
    pairs = np.argwhere(cov)
    ratio, _, amb = overlap_pairs(caps, pairs, canvas_rule)
    dist, ambiguous = np.zeros((n, n), dtype=np.float32), np.zeros((n, n), dtype=np.int64)
    dist[pairs[:, 0], pairs[:, 1]] = ratio
    ambiguous[pairs[:, 0], pairs[:, 1]] = amb
    return dist, ambiguous


def num_pos(dist, db_mask=None):
    dist = np.asarray(dist)
    inside = np.ones(dist.shape[0], dtype=bool)
    if db_mask is not None:
        inside[:] = False
        inside[np.asarray(db_mask, dtype=np.int64)] = True
    return ((dist > np.float32(THRESH)) & inside[None, :]).sum(1)


def knn_pool(dist, k, db_mask=None):
    """the neighbour lists of every query row, ties to the lower index -> (indices int64 [N, k] padded with -1, counts [N])"""
    dist = np.asarray(dist, dtype=np.float32)
    n = dist.shape[0]
    pos = num_pos(dist, db_mask)
    temp = dist.copy()
    if db_mask is not None:
        outside = np.setdiff1d(np.arange(n), np.asarray(db_mask, dtype=np.int64))
        temp[:, outside] = -1
    out = np.full((n, k), -1, dtype=np.int64)
    counts = np.zeros(n, dtype=np.int64)
    for i in range(n):
        order = np.argsort(-temp[i], kind='stable')
        if pos[i] > k:
            ind = [int(j) for j in order[:k + 1]]
            ind = [j for j in ind if j != i] if i in ind else ind[:k]
        else:
            ind = [int(j) for j in order[:max(int(pos[i]), 1)]]
        out[i, :len(ind)] = ind
        counts[i] = len(ind)
    return out, counts


def draw_pairs(pool, counts, u):
    """entry floor(u count) of every row's pool"""
    pool, counts = np.asarray(pool), np.asarray(counts)
    j = np.minimum(np.floor(np.asarray(u, dtype=np.float64) * counts).astype(np.int64), counts - 1)
    return pool[np.arange(pool.shape[0]), np.maximum(j, 0)]
