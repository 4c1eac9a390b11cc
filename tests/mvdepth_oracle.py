"""A numpy float64 restatement of cotr_amd/csrc/mvdepth.hip, written from the rules of include/cotr_hip.h:
``corr_depth`` (cotr_corr_depth) and ``depth_consistency`` (cotr_depth_consistency), vectorised over the pixels, every sum over
views written out in the device's order and every expression bracketed as the header brackets it, so that the device's bits
are reproduced.  Both count the decisions that fall within EPS of a threshold (``ambiguous``): the vote and the filters, ``rint``
at half-integers, a depth at 0.  Test infrastructure."""
import numpy as np

EPS = 1e-9
F32 = np.float32


def _near(value, at):
    return np.abs(value - at) < EPS


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(F32)


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def w2c_rows(c2ws):
    """camera-to-world [V,4,4] -> world-to-camera rows [V,12], the inverse of a rigid pose"""
    out = []
    for m in np.asarray(c2ws, dtype=np.float64):
        R, t = m[:3, :3], m[:3, 3]
        out.append(np.concatenate([R.T, -(R.T @ t)[:, None]], axis=1).reshape(12))
    return np.stack(out)


def cam_rows(Ks):
    k = np.asarray(Ks, dtype=np.float64)
    return np.stack([k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2], k[:, 0, 1]], axis=1)


def reproject(depth, K, c2w, K_b, c2w_b, depth_b=None, tol=1e-3):
    """The exact correspondence map of a depth map: every pixel (x, y) with a depth lifted through (K, c2w) and projected
    through (K_b, c2w_b) -> (corr float64 [H,W,2] with NaN where there is no depth, visible bool [H,W]: in front of B, inside
    B's image and, with ``depth_b``, not occluded there: B's depth at the nearest pixel within ``tol`` (relative) of the point's)"""
    H, W = depth.shape
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    z = depth.astype(np.float64)
    K, K_b = np.asarray(K, np.float64), np.asarray(K_b, np.float64)
    yn = (ys - K[1, 2]) / K[1, 1]
    xn = (xs - K[0, 2] - K[0, 1] * yn) / K[0, 0]
    Y = np.stack([xn * z, yn * z, z], -1)
    P = Y @ c2w[:3, :3].T + c2w[:3, 3]
    Q = (P - c2w_b[:3, 3]) @ c2w_b[:3, :3]
    with np.errstate(all='ignore'):
        u = K_b[0, 0] * Q[..., 0] / Q[..., 2] + K_b[0, 1] * Q[..., 1] / Q[..., 2] + K_b[0, 2]
        v = K_b[1, 1] * Q[..., 1] / Q[..., 2] + K_b[1, 2]
    has = z > 0
    vis = has & (Q[..., 2] > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    if depth_b is not None:
        iu, iv = np.clip(np.rint(np.where(vis, u, 0)), 0, W - 1).astype(int), np.clip(np.rint(np.where(vis, v, 0)), 0, H - 1).astype(int)
        db = depth_b[iv, iu].astype(np.float64)
        vis &= (db > 0) & (np.abs(db - Q[..., 2]) <= tol * Q[..., 2])
    corr = np.stack([u, v], -1)
    corr[~has] = np.nan
    return corr, vis


_scenes = {}


def scene(H, W, K, seed=0):
    """K + 1 captures on the arc of ``synth_scene`` (the middle one first: the reference) and the exact correspondence maps of the
    reference's depth into the others -> dict: caps, Ks [K+1,3,3], c2ws [K+1,4,4], cams [K+1,5], poses [K+1,12], corr64
    [K,H,W,2], corr float32 (NaN where the reference has no depth), vis bool [K,H,W] (inside the neighbour and not occluded
    there), depth float32 [H,W] (the truth).  Cached: callers copy before they change anything."""
    key = (H, W, K, seed)
    if key not in _scenes:
        from cotr_amd.utils.synth import synth_scene
        caps = synth_scene(seed, K + 3, H, W)[:K + 1]
        mid = (K + 1) // 2
        caps = [caps[mid]] + caps[:mid] + caps[mid + 1:]
        both = [reproject(caps[0].depth, caps[0].K, caps[0].c2w, c.K, c.c2w, c.depth) for c in caps[1:]]
        corr64 = np.stack([b[0] for b in both])
        Ks, c2ws = np.stack([c.K for c in caps]), np.stack([c.c2w for c in caps])
        _scenes[key] = dict(caps=caps, Ks=Ks, c2ws=c2ws, cams=cam_rows(Ks), poses=w2c_rows(c2ws), corr64=corr64, corr=corr64.astype(F32),
                            vis=np.stack([b[1] for b in both]), depth=caps[0].depth)
    return _scenes[key]


def parallax_deg(sc):
    """the angle at every reference pixel's true point between the reference centre and each neighbour's -> float64 [K,H,W]"""
    cap = sc['caps'][0]
    H, W = cap.depth.shape
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    z = cap.depth.astype(np.float64)
    yn = (ys - cap.K[1, 2]) / cap.K[1, 1]
    xn = (xs - cap.K[0, 2] - cap.K[0, 1] * yn) / cap.K[0, 0]
    P = np.stack([xn * z, yn * z, z], -1) @ cap.c2w[:3, :3].T + cap.c2w[:3, 3]
    out = []
    with np.errstate(all='ignore'):
        for m in sc['c2ws'][1:]:
            a, b = cap.c2w[:3, 3] - P, m[:3, 3] - P
            cs = (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))
            out.append(np.degrees(np.arccos(np.clip(cs, -1.0, 1.0))))
    return np.stack(out)


# ---- cotr_corr_depth ----------------------------------------------------------------------------------------------------------
def view_table(cams, poses):
    """the Prepare rule of cotr_triangulate_views -> one dict per view: k (fx, fy, cx, cy, skew), R [3,3], t, c, ok"""
    views = []
    for k, P in zip(np.asarray(cams, np.float64).reshape(-1, 5), np.asarray(poses, np.float64).reshape(-1, 12)):
        R, t = P.reshape(3, 4)[:, :3], P.reshape(3, 4)[:, 3]
        with np.errstate(all='ignore'):
            c = np.array([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)])
        ok = bool(np.isfinite(k).all() and k[0] != 0 and k[1] != 0 and np.isfinite(P).all() and np.isfinite(c).all())
        views.append(dict(k=k, R=R, t=t, c=c, ok=ok))
    return views


def _normalise(k, u, v):
    u, v = _f32(u).astype(np.float64), _f32(v).astype(np.float64)
    yy = (v - k[3]) / k[1]
    return (u - k[2] - k[4] * yy) / k[0], yy


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def ray(view, u, v):
    x, y = _normalise(view['k'], u, v)
    R = view['R']
    return [(R[0, i] * x + R[1, i] * y) + R[2, i] for i in range(3)]


def project(view, u, v, X):
    """the Projection rule of cotr_triangulate_views -> dict z, xn, yn, du, dv, e"""
    R, t, k = view['R'], view['t'], view['k']
    p = [((R[i, 0] * X[0] + R[i, 1] * X[1]) + R[i, 2] * X[2]) + t[i] for i in range(3)]
    z = p[2]
    xn, yn = p[0] / z, p[1] / z
    du = ((k[0] * xn + k[4] * yn) + k[2]) - u
    dv = (k[1] * yn + k[3]) - v
    return dict(z=z, xn=xn, yn=yn, du=du, dv=dv, e=du * du + dv * dv)


class Pixels:
    """the per-pixel state of one cotr_corr_depth call: the view table, the maps flattened to [K, HW], the reference rays"""

    def __init__(self, corr, valid, cams, poses):
        corr = np.asarray(corr)
        assert corr.dtype == F32 and corr.ndim == 4 and corr.shape[3] == 2
        self.K, self.H, self.W = corr.shape[:3]
        self.V = self.K + 1
        self.views = view_table(cams, poses)
        assert len(self.views) == self.V
        HW = self.H * self.W
        self.u = corr[..., 0].reshape(self.K, HW).astype(np.float64)
        self.v = corr[..., 1].reshape(self.K, HW).astype(np.float64)
        self.finite = np.isfinite(self.u) & np.isfinite(self.v)
        self.valid = np.ones((self.K, HW), bool) if valid is None else (np.asarray(valid).reshape(self.K, HW) != 0)
        idx = np.arange(HW)
        with np.errstate(all='ignore'):
            self.r = ray(self.views[0], (idx % self.W).astype(np.float64), (idx // self.W).astype(np.float64))

    def point(self, s):
        c0 = self.views[0]['c']
        return [c0[i] + s * self.r[i] for i in range(3)]

    def candidate(self, j, max_cos):
        """-> (parallax, ok, s, near: a decision of this candidate within EPS of its threshold)"""
        vw = self.views[j]
        rk = ray(vw, self.u[j - 1], self.v[j - 1])
        r = self.r
        a, b, e = _dot(r, r), _dot(r, rk), _dot(rk, rk)
        w = [vw['c'][i] - self.views[0]['c'][i] for i in range(3)]
        rw, kw = _dot(r, w), _dot(rk, w)
        den = a * e - b * b
        s = (rw * e - b * kw) / den
        cs = b / np.sqrt(a * e)
        parallax = cs <= max_cos
        ok = (den != 0) & np.isfinite(den) & np.isfinite(s) & (s > 0)
        near = _near(cs, max_cos) | (parallax & (_near(s, 0) | _near(den, 0)))
        return parallax, ok, s, near

    def project(self, j, X):
        return project(self.views[j], self.u[j - 1], self.v[j - 1], X)

    def normal(self, U, s):
        """E(s), front, A, g over the views of the bit masks U, ascending"""
        X = self.point(s)
        E, A, g = np.zeros_like(s), np.zeros_like(s), np.zeros_like(s)
        front = np.ones(s.shape, bool)
        for j in range(1, self.V):
            m = (U >> j & 1) != 0
            if not m.any():
                continue
            pr = self.project(j, X)
            R, k = self.views[j]['R'], self.views[j]['k']
            q = [(R[i, 0] * self.r[0] + R[i, 1] * self.r[1]) + R[i, 2] * self.r[2] for i in range(3)]
            a, b = (q[0] - pr['xn'] * q[2]) / pr['z'], (q[1] - pr['yn'] * q[2]) / pr['z']
            ju, jv = k[0] * a + k[4] * b, k[1] * b
            E = np.where(m, E + pr['e'], E)
            front &= ~m | (pr['z'] > 0)
            A = np.where(m, A + (ju * ju + jv * jv), A)
            g = np.where(m, g + (ju * pr['du'] + jv * pr['dv']), g)
        return E, front, A, g


def corr_depth(corr, valid, cams, poses, found=None, threshold=2.0, max_cos=1.0, distance_thresh=50.0, min_views=1, refine_iters=10):
    """-> dict: depth float32 [H,W], views uint8 [H,W], err float32 [H,W], info int32 [8], ambiguous (pixels with a decision
    within EPS of its threshold), and for the tests U uint32 [H,W] (the winner's inlier views as bits, bit j = view j), s0
    float64 [H,W] (the winner's s before the refit), steps int [H,W], trace (per pixel the E of every evaluation kept)."""
    px = Pixels(corr, valid, cams, poses)
    H, W, V, HW = px.H, px.W, px.V, px.H * px.W
    thr = F32(float(threshold) * float(threshold))
    on = (found is None or int(np.asarray(found).reshape(-1)[0]) != 0) and px.views[0]['ok']
    depth, views, err = np.zeros(HW, F32), np.zeros(HW, np.uint8), np.full(HW, np.nan, F32)
    info = np.zeros(8, np.int32)
    info[0] = 1 if found is None else int(int(np.asarray(found).reshape(-1)[0]) != 0)
    out = dict(depth=depth.reshape(H, W), views=views.reshape(H, W), err=err.reshape(H, W), info=info, ambiguous=0, U=np.zeros((H, W), np.uint32),
               s0=np.zeros((H, W)), steps=np.zeros((H, W), np.int64), trace=[])
    if not on:
        return out
    amb = np.zeros(HW, bool)
    with np.errstate(all='ignore'):
        P = np.zeros(HW, np.uint32)
        any_cand = np.zeros(HW, bool)
        cands = {}
        for j in range(1, V):
            if not px.views[j]['ok']:
                continue
            sees = px.valid[j - 1] & px.finite[j - 1]
            parallax, ok, s, near = px.candidate(j, max_cos)
            amb |= sees & near
            m = sees & parallax
            P |= np.where(m, np.uint32(1 << j), np.uint32(0))
            any_cand |= m & ok
            cands[j] = (m & ok, s)
        U, best, s = np.zeros(HW, np.uint32), np.zeros(HW, np.int64), np.zeros(HW)
        for k, (ok, sk) in cands.items():
            if not ok.any():
                continue
            X = px.point(sk)
            inl = np.zeros(HW, np.uint32)
            for j in cands:
                inP = (P >> j & 1) != 0
                pr = px.project(j, X)
                hit = inP & (pr['z'] > 0) & (pr['e'].astype(F32) <= thr)
                amb |= ok & inP & (_near(pr['z'], 0) | ((pr['z'] > 0) & _near(pr['e'], float(thr))))
                inl |= np.where(hit, np.uint32(1 << j), np.uint32(0))
            cnt = _popcount(inl)
            take = ok & (cnt > best)
            best, U, s = np.where(take, cnt, best), np.where(take, inl, U), np.where(take, sk, s)
        few = any_cand & (best < min_views)
        live = any_cand & ~few
        s = np.where(live, s, 1.0)
        U = np.where(live, U, np.uint32(0))
        out['U'], out['s0'] = U.reshape(H, W).copy(), np.where(live, s, 0.0).reshape(H, W)
        E, front, A, g = px.normal(U, s)
        steps = np.zeros(HW, np.int64)
        going = live & front
        trace = [E.copy()]
        for _ in range(int(refine_iters)):
            going = going & (A > 0) & (A < np.inf)
            sn = s - g / A
            going = going & (sn > 0)
            if not going.any():
                break
            En, front_n, An, gn = px.normal(U, np.where(going, sn, s))
            going = going & front_n & (En < E)
            s, E, A, g = np.where(going, sn, s), np.where(going, En, E), np.where(going, An, A), np.where(going, gn, g)
            steps += going
            trace.append(np.where(going, E, np.nan))
        X = px.point(s)
        err_ok = np.ones(HW, bool)
        for j in range(1, V):
            m = (U >> j & 1) != 0
            if not m.any():
                continue
            pr = px.project(j, X)
            err_ok &= ~m | (pr['e'].astype(F32) <= thr)
            amb |= live & m & _near(pr['e'], float(thr))
        depth_ok = (s > 0) & (s < distance_thresh)
        amb |= live & (_near(s, distance_thresh) | _near(s, 0))
        good = live & depth_ok & err_ok
        depth[good] = s[good].astype(F32)
        views[good] = best[good].astype(np.uint8)
        err[good] = (E[good] / best[good].astype(np.float64)).astype(F32)
        info[1:6] = [good.sum(), few.sum(), (~any_cand).sum(), (live & ~depth_ok).sum(), (live & depth_ok & ~err_ok).sum()]
        info[7] = steps[live].sum()
        out['steps'], out['trace'], out['ambiguous'] = np.where(live, steps, 0).reshape(H, W), trace, int(amb.sum())
    return out


def _popcount(x):
    x = x.astype(np.uint64)
    n = np.zeros(x.shape, np.int64)
    for b in range(32):
        n += (x >> np.uint64(b) & np.uint64(1)).astype(np.int64)
    return n


# ---- cotr_depth_consistency ---------------------------------------------------------------------------------------------------
def _vertex(depth, K, xs, ys):
    """ic_vertex at integer pixels -> (Y [3], valid)"""
    z = depth.astype(np.float64)
    valid = (z > 0) & (z < np.inf)
    yn = (ys - K[1, 2]) / K[1, 1]
    xn = (xs - K[0, 2] - K[0, 1] * yn) / K[0, 0]
    return [xn * z, yn * z, z], valid


def _to_world(m, Y):
    return [((m[a, 0] * Y[0] + m[a, 1] * Y[1]) + m[a, 2] * Y[2]) + m[a, 3] for a in range(3)]


def _to_pixel(m, K, P):
    d = [P[a] - m[a, 3] for a in range(3)]
    Yx, Yy, Yz = ((m[0, a] * d[0] + m[1, a] * d[1]) + m[2, a] * d[2] for a in range(3))
    xn, yn = Yx / Yz, Yy / Yz
    return Yz, (K[0, 0] * xn + K[0, 1] * yn) + K[0, 2], K[1, 1] * yn + K[1, 2]


def depth_consistency(depths, Ks, c2ws, found=None, pairs=None, px_thresh=1.0, rel_thresh=0.01, min_views=2, max_violations=-1):
    """-> dict: depth float32 [n,H,W], count uint8 [n,H,W], info int32 [n,4], ambiguous, and for the tests violations [n,H,W]
    and mean float64 [n,H,W] (the kept depth before it is rounded to float32, 0 elsewhere)."""
    depths = np.asarray(depths)
    assert depths.dtype == F32 and depths.ndim == 3
    n, H, W = depths.shape
    Ks = np.broadcast_to(np.asarray(Ks, np.float64), (n, 3, 3))
    c2ws = np.asarray(c2ws, np.float64).reshape(n, 4, 4)
    found = np.ones(n, np.int64) if found is None else np.asarray(found).reshape(n)
    pairs = np.ones((n, n), np.uint8) if pairs is None else np.asarray(pairs).reshape(n, n)
    px2 = float(px_thresh) * float(px_thresh)
    out_d, out_c, info = np.zeros((n, H, W), F32), np.zeros((n, H, W), np.uint8), np.zeros((n, 4), np.int32)
    viol_all, mean_all = np.zeros((n, H, W), np.int64), np.zeros((n, H, W))
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    amb_total = 0
    with np.errstate(all='ignore'):
        for i in range(n):
            if found[i] == 0:
                continue
            info[i, 0] = 1
            Y, ok = _vertex(depths[i], Ks[i], xs, ys)
            z = Y[2]
            P = _to_world(c2ws[i], Y)
            cons, viol, total = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64), z.copy()
            amb = np.zeros((H, W), bool)
            for j in range(n):
                if j == i or found[j] == 0 or pairs[i, j] == 0:
                    continue
                Yz, u, v = _to_pixel(c2ws[j], Ks[j], P)
                front = ok & (Yz > 0)
                amb |= ok & _near(Yz, 0)
                ru, rv = np.rint(u), np.rint(v)
                inside = front & (ru >= 0) & (ru < W) & (rv >= 0) & (rv < H)
                amb |= front & (_near(u - np.floor(u), 0.5) | _near(v - np.floor(v), 0.5))
                iu, iv = np.where(inside, ru, 0).astype(np.int64), np.where(inside, rv, 0).astype(np.int64)
                Yj, okj = _vertex(depths[j][iv, iu], Ks[j], iu.astype(np.float64), iv.astype(np.float64))
                seen = inside & okj
                Q = _to_world(c2ws[j], Yj)
                z2, u2, v2 = _to_pixel(c2ws[i], Ks[i], Q)
                du, dv = u2 - xs, v2 - ys
                d2 = du * du + dv * dv
                good = seen & (z2 > 0) & (d2 <= px2) & (np.abs(z2 - z) <= rel_thresh * z)
                amb |= seen & (_near(z2, 0) | _near(d2, px2) | _near(np.abs(z2 - z), rel_thresh * z))
                bad = seen & ~good & (Yj[2] > Yz * (1.0 + rel_thresh))
                amb |= seen & ~good & _near(Yj[2], Yz * (1.0 + rel_thresh))
                cons += good
                total = np.where(good, total + z2, total)
                viol += bad
            enough = ok & (cons >= min_views)
            through = enough & (max_violations >= 0) & (viol > max_violations)
            keep = enough & ~through
            mean = total / (1 + cons).astype(np.float64)
            out_d[i] = np.where(keep, mean, 0.0).astype(F32)
            out_c[i] = cons.astype(np.uint8)
            info[i, 1:] = [ok.sum(), keep.sum(), through.sum()]
            viol_all[i], mean_all[i] = viol, np.where(keep, mean, 0.0)
            amb_total += int(amb.sum())
    return dict(depth=out_d, count=out_c, info=info, ambiguous=amb_total, violations=viol_all, mean=mean_all)
