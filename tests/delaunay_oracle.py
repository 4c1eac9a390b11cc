"""Restatement of cotr_delaunay's rule in exact integers, twice:

  form='int'    Python integers, the definitions taken literally: any float32 input (full 24-bit coordinates)
  form='int64'  vectorised numpy int64 for points on the k/4096 lattice inside [-2, 2]: there X = 4096 k, the coordinates
                are divided by 4096 first (every predicate keeps its sign), differences then have at most 15 bits and the
                in-circle determinant stays below 2^60

Both return (tris int32 [T, 3] in the rule's order, status).  ``properties`` and ``is_unique`` check a triangulation."""
import numpy as np

SCALE = 1 << 24
LIMIT = 1 << 26


def snap(P):
    """float32 [n, 2] -> list of (X, Y) Python ints, None for an invalid point"""
    P = np.asarray(P, dtype=np.float32).reshape(-1, 2)
    out, seen = [], set()
    for u, v in P:
        xy = None
        if np.isfinite(u) and np.isfinite(v):
            X, Y = int(np.rint(np.float64(u) * SCALE)), int(np.rint(np.float64(v) * SCALE))
            if abs(X) <= LIMIT and abs(Y) <= LIMIT and (X, Y) not in seen:
                seen.add((X, Y))
                xy = (X, Y)
        out.append(xy)
    return out


def orient(p, q, r):
    return (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])


def det0(a, b, c, d):
    ax, ay, bx, by, cx, cy = a[0] - d[0], a[1] - d[1], b[0] - d[0], b[1] - d[1], c[0] - d[0], c[1] - d[1]
    return ((ax * ax + ay * ay) * (bx * cy - by * cx) - (bx * bx + by * by) * (ax * cy - ay * cx) +
            (cx * cx + cy * cy) * (ax * by - ay * bx))


class _IntForm:
    def __init__(self, S):
        self.S = S
        self.valid = [i for i, s in enumerate(S) if s is not None]

    def inside(self, ia, ib, ic, id_):
        a, b, c, d = self.S[ia], self.S[ib], self.S[ic], self.S[id_]
        det = det0(a, b, c, d)
        if det != 0:
            return det > 0
        cof = {ia: orient(b, c, d), ib: -orient(a, c, d), ic: orient(a, b, d), id_: -orient(a, b, c)}
        for i in sorted(cof):
            if cof[i] != 0:
                return cof[i] > 0
        raise AssertionError('C_d is never zero')

    def nearest(self, p):
        best, bd = -1, None
        P = self.S[p]
        for j in self.valid:
            if j != p:
                d = (self.S[j][0] - P[0]) ** 2 + (self.S[j][1] - P[1]) ** 2
                if bd is None or d < bd:
                    best, bd = j, d
        return best

    def apex(self, ia, ib):
        a, b = self.S[ia], self.S[ib]
        best = -1
        for j in self.valid:
            if orient(a, b, self.S[j]) > 0 and (best < 0 or self.inside(ia, ib, best, j)):
                best = j
        return best


class _Int64Form:
    def __init__(self, S):
        self.valid = np.array([i for i, s in enumerate(S) if s is not None], dtype=np.int64)
        XY = np.array([s if s is not None else (0, 0) for s in S], dtype=np.int64).reshape(-1, 2)
        assert (XY % 4096 == 0).all(), 'int64 form: points must lie on the k/4096 lattice'
        XY //= 4096
        assert np.abs(XY).max(initial=0) <= 1 << 13, 'int64 form: points must lie inside [-2, 2]'
        self.X, self.Y = XY[:, 0].copy(), XY[:, 1].copy()
        self.ok = np.zeros(len(S), dtype=bool)
        self.ok[self.valid] = True

    def nearest(self, p):
        d = (self.X - self.X[p]) ** 2 + (self.Y - self.Y[p]) ** 2
        d[~self.ok] = np.iinfo(np.int64).max
        d[p] = np.iinfo(np.int64).max
        j = int(np.argmin(d))                       # the first minimum: the lowest index
        return j if self.ok[j] and j != p else -1

    def inside_many(self, ia, ib, ic, idx):
        """inside(a, b, c, d) for every d in idx (none equal to a, b or c)"""
        X, Y = self.X, self.Y
        dx, dy = X[idx], Y[idx]
        ax, ay, bx, by, cx, cy = X[ia] - dx, Y[ia] - dy, X[ib] - dx, Y[ib] - dy, X[ic] - dx, Y[ic] - dy
        Ca, Cb, Cc = bx * cy - by * cx, -(ax * cy - ay * cx), ax * by - ay * bx
        det = (ax * ax + ay * ay) * Ca + (bx * bx + by * by) * Cb + (cx * cx + cy * cy) * Cc
        out = det > 0
        tie = np.flatnonzero(det == 0)
        if tie.size:
            Cd = -int((X[ib] - X[ia]) * (Y[ic] - Y[ia]) - (Y[ib] - Y[ia]) * (X[ic] - X[ia]))
            assert Cd != 0
            ids = idx[tie]
            res, decided = np.zeros(tie.size, dtype=bool), np.zeros(tie.size, dtype=bool)
            for i, C in sorted([(ia, Ca[tie]), (ib, Cb[tie]), (ic, Cc[tie])], key=lambda t: t[0]):
                m = ~decided & (ids < i)            # d's index comes before i: its cofactor is never zero
                res[m], decided = Cd > 0, decided | m
                m = ~decided & (C != 0)
                res[m], decided = C[m] > 0, decided | m
            res[~decided] = Cd > 0
            out[tie] = res
        return out

    def apex(self, ia, ib):
        X, Y = self.X, self.Y
        o = (X[ib] - X[ia]) * (Y - Y[ia]) - (Y[ib] - Y[ia]) * (X - X[ia])
        idx = np.flatnonzero(self.ok & (o > 0))
        if not idx.size:
            return -1
        # a float guess (the largest angle a-d-b, i.e. the smallest cotangent), then exact passes until nobody beats it
        ax, ay, bx, by = (X[ia] - X[idx]).astype(float), (Y[ia] - Y[idx]).astype(float), (X[ib] - X[idx]).astype(float), \
            (Y[ib] - Y[idx]).astype(float)
        cot = (ax * bx + ay * by) / (ax * by - ay * bx)
        best = int(idx[np.argmin(cot)])
        while True:
            rest = idx[idx != best]
            ins = self.inside_many(ia, ib, best, rest)
            if not ins.any():
                return best
            k = np.flatnonzero(ins)
            best = int(rest[k[np.argmin(cot[idx != best][k])]])


def triangulate(P, form='int'):
    """the rule's triangles of float32 points P [n, 2], in the rule's order -> (int32 [T, 3], status)"""
    S = snap(P)
    n = len(S)
    F = _IntForm(S) if form == 'int' else _Int64Form(S)
    tris, status = [], 0

    def emit(p, q, c):
        if p < q and p < c:
            tris.append((p, q, c))

    for p in (int(i) for i in F.valid):
        q0 = F.nearest(p)
        if q0 < 0:
            continue
        steps, q, closed, stopped = 0, q0, False, False
        while True:
            if steps >= n:
                status, stopped = 1, True
                break
            steps += 1
            c = F.apex(p, q)
            if c < 0:
                break
            emit(p, q, c)
            q = c
            if c == q0:
                closed = True
                break
        if closed or stopped:
            continue
        q = q0
        while True:
            if steps >= n:
                status = 1
                break
            steps += 1
            c = F.apex(q, p)
            if c < 0:
                break
            emit(p, c, q)
            q = c
    return np.array(tris, dtype=np.int32).reshape(-1, 3), status


# ---- checks of a triangulation -------------------------------------------------------------------------------------------
def _columns(S):
    """coordinates of the valid points as numpy columns in which the in-circle determinant is exact: int64 for small
    lattice points, Python ints (object) otherwise"""
    valid = np.array([i for i, s in enumerate(S) if s is not None], dtype=np.int64)
    XY = [S[i] for i in valid]
    small = all(x % 4096 == 0 and y % 4096 == 0 and abs(x) <= 1 << 25 and abs(y) <= 1 << 25 for x, y in XY)
    if small:
        A = np.array(XY, dtype=np.int64).reshape(-1, 2) // 4096
    else:
        A = np.array(XY, dtype=object).reshape(-1, 2)
    return valid, A[:, 0], A[:, 1]


def _det_many(a, b, c, X, Y):
    ax, ay, bx, by, cx, cy = a[0] - X, a[1] - Y, b[0] - X, b[1] - Y, c[0] - X, c[1] - Y
    return (ax * ax + ay * ay) * (bx * cy - by * cx) - (bx * bx + by * by) * (ax * cy - ay * cx) + \
        (cx * cx + cy * cy) * (ax * by - ay * bx)


def hull_area2(pts):
    """twice the area of the convex hull of integer points (monotone chain)"""
    pts = sorted(set(pts))
    if len(pts) < 3:
        return 0

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and orient(h[-2], h[-1], p) <= 0:
                h.pop()
            h.append(p)
        return h
    hull = half(pts)[:-1] + half(pts[::-1])[:-1]
    return sum(hull[i][0] * hull[(i + 1) % len(hull)][1] - hull[(i + 1) % len(hull)][0] * hull[i][1] for i in range(len(hull)))


def properties(P, tris):
    """asserts: counter-clockwise triangles, lowest index first, area sum == hull area, non-strict empty circles, every
    valid point a vertex (when there is any triangle), every edge used at most twice"""
    S = snap(P)
    tris = np.asarray(tris).reshape(-1, 3)
    valid, X, Y = _columns(S)
    pos = {int(v): k for k, v in enumerate(valid)}
    area2, edges = 0, {}
    for t in tris:
        i, j, k = (int(x) for x in t)
        assert i in pos and j in pos and k in pos, f'triangle {t} names an invalid point'
        assert i < j and i < k, f'triangle {t}: the lowest index does not come first'
        a, b, c = S[i], S[j], S[k]
        o = orient(a, b, c)
        assert o > 0, f'triangle {t} is not counter-clockwise'
        area2 += o
        pa, pb, pc = ((X[pos[v]], Y[pos[v]]) for v in (i, j, k))
        assert not (_det_many(pa, pb, pc, X, Y) > 0).any(), f'a point lies strictly inside the circle of {t}'
        for e in ((i, j), (j, k), (k, i)):
            e = (min(e), max(e))
            edges[e] = edges.get(e, 0) + 1
    assert area2 == hull_area2([S[int(v)] for v in valid]), 'the triangles do not tile the hull'
    assert all(v <= 2 for v in edges.values()), 'an edge is used more than twice'
    if len(tris):
        assert set(int(x) for x in tris.ravel()) == set(pos), 'a valid point is no vertex'


def is_unique(P, tris):
    """True when no fourth valid point is exactly cocircular with a triangle: the Delaunay triangulation is then unique"""
    S = snap(P)
    valid, X, Y = _columns(S)
    pos = {int(v): k for k, v in enumerate(valid)}
    for t in np.asarray(tris).reshape(-1, 3):
        pa, pb, pc = ((X[pos[int(v)]], Y[pos[int(v)]]) for v in t)
        if int((_det_many(pa, pb, pc, X, Y) == 0).sum()) > 3:
            return False
    return True


def as_set(tris):
    """triangles as a set of sorted index triples"""
    return {tuple(sorted(int(x) for x in t)) for t in np.asarray(tris).reshape(-1, 3)}
