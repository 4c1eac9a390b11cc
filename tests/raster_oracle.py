"""numpy restatement of cotr_raster_mesh: the coverage rule in exact int64 arithmetic, values in float64,
highest index wins.  The GPU tests compare the library against it (coverage identical, values within 1e-3 px)."""
import numpy as np

LIMIT = 1 << 30     # snapped coordinates of magnitude >= 2^30 (2^22 px) make a triangle be skipped


def snap(verts, H, W):
    """float32 normalised (u, v) -> (X, Y) in 1/256 px as int64, and which vertices are usable"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        X = np.rint(v[:, 0] * W * 256.0)
        Y = np.rint(v[:, 1] * H * 256.0)
        ok = (np.abs(X) < LIMIT) & (np.abs(Y) < LIMIT)
    return np.where(ok, X, 0).astype(np.int64), np.where(ok, Y, 0).astype(np.int64), ok


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _edge_in(e, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return (e > 0) | ((e == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))


def raster(verts, attrs, tris, H, W):
    """-> (out float64 [H,W,2], mask bool [H,W], ids int64 [H,W] (-1 where uncovered), count int64 [H,W] (how many triangles
    cover each sample))"""
    X, Y, vok = snap(verts, H, W)
    nv = len(X)
    attrs = np.asarray(attrs, dtype=np.float32).astype(np.float64)
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    ids = np.full((H, W), -1, dtype=np.int64)
    count = np.zeros((H, W), dtype=np.int64)
    out = np.zeros((H, W, 2))
    for t, tri in enumerate(tris):
        if not ((tri >= 0) & (tri < nv)).all() or not vok[tri].all():
            continue
        a, b, c = (int(k) for k in tri)
        a2 = int(_edge(X[a], Y[a], X[b], Y[b], X[c], Y[c]))
        if a2 < 0:
            b, c, a2 = c, b, -a2
        if a2 == 0:
            continue
        xs, ys = X[[a, b, c]], Y[[a, b, c]]
        j0, j1 = max(-((128 - xs.min()) >> 8), 0), min((xs.max() - 128) >> 8, W - 1)
        i0, i1 = max(-((128 - ys.min()) >> 8), 0), min((ys.max() - 128) >> 8, H - 1)
        if j0 > j1 or i0 > i1:
            continue
        py, px = np.mgrid[i0:i1 + 1, j0:j1 + 1].astype(np.int64)
        py, px = py * 256 + 128, px * 256 + 128
        e_ab = _edge(X[a], Y[a], X[b], Y[b], px, py)
        e_bc = _edge(X[b], Y[b], X[c], Y[c], px, py)
        e_ca = _edge(X[c], Y[c], X[a], Y[a], px, py)
        inside = (_edge_in(e_ab, X[a], Y[a], X[b], Y[b]) & _edge_in(e_bc, X[b], Y[b], X[c], Y[c]) &
                  _edge_in(e_ca, X[c], Y[c], X[a], Y[a]))
        if not inside.any():
            continue
        val = (e_bc[..., None] / a2 * attrs[a] + e_ca[..., None] / a2 * attrs[b] + e_ab[..., None] / a2 * attrs[c])
        win = (slice(i0, i1 + 1), slice(j0, j1 + 1))
        ids[win][inside] = t
        count[win] += inside
        out[win][inside] = val[inside]
    return out, ids >= 0, ids, count


def jittered_grid(nx, ny, jitter, seed, lo=0.0, hi=1.0):
    """(nx+1) x (ny+1) points over [lo, hi]^2 with the inner ones moved by up to jitter cells, two triangles per cell
    (alternating diagonals) -> verts float32 [N,2], tris int32 [T,3]"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.linspace(lo, hi, nx + 1), np.linspace(lo, hi, ny + 1))
    pts = np.stack([gx, gy], -1).reshape(-1, 2)
    inner = np.ones((ny + 1, nx + 1), bool)
    inner[[0, -1], :] = inner[:, [0, -1]] = False
    step = np.array([(hi - lo) / nx, (hi - lo) / ny])
    pts[inner.ravel()] += rng.uniform(-jitter, jitter, (int(inner.sum()), 2)) * step
    tris = []
    for y in range(ny):
        for x in range(nx):
            p = y * (nx + 1) + x
            q = [p, p + 1, p + nx + 1, p + nx + 2]
            if (x + y) % 2:
                tris += [[q[0], q[1], q[3]], [q[0], q[3], q[2]]]
            else:
                tris += [[q[0], q[1], q[2]], [q[1], q[3], q[2]]]
    return pts.astype(np.float32), np.array(tris, dtype=np.int32)
