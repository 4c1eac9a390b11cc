"""numpy restatement of the N-view triangulation rules of DESIGN.md 3h-6 (cotr_triangulate_views in
cotr_amd/csrc/structure.hip): the view table, the rays, the ray least squares with its cofactor solve, the pair vote of the
robust mode, the Gauss-Newton fit on the pixel error, the demo's rule, the quality figures, the mask and the counters.
Vectorised over the points; every sum over views is written out term by term in the device's order (no np.sum / dot /
einsum on the compared path), so the device is expected to give the same bits.  Also: the N-view scene builder of the tests
and the demo's own route (un-project at depth 2 through the camera-to-world matrix, subtract the centre) as a second path.
numpy only.  Test infrastructure."""
import numpy as np

MAX_VIEWS = 32


def f32(x):
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


# ---- the view table -------------------------------------------------------------------------------------------------------
def prepare(cams, poses):
    """cams [V,5], poses [V,12] -> dict(k [V,5], R [V,9], t [V,3], c [V,3], ok [V])"""
    k = np.asarray(cams, np.float64).reshape(-1, 5)
    P = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    R, t = P[:, :, :3].reshape(-1, 9), P[:, :, 3]
    with np.errstate(all='ignore'):
        c = np.stack([-((R[:, j] * t[:, 0] + R[:, 3 + j] * t[:, 1]) + R[:, 6 + j] * t[:, 2]) for j in range(3)], axis=1)
    ok = np.isfinite(k).all(axis=1) & (k[:, 0] != 0) & (k[:, 1] != 0) & np.isfinite(R).all(axis=1) & np.isfinite(t).all(axis=1) & \
        np.isfinite(c).all(axis=1)
    return dict(k=k, R=R, t=t, c=c, ok=ok)


# ---- per-view arithmetic, over all points ---------------------------------------------------------------------------------
def ray(tab, v, u, w):
    """unit ray of the rounded pixels (u, w) [N] of view v -> (d0, d1, d2)"""
    fx, fy, cx, cy, s = tab['k'][v]
    R = tab['R'][v]
    y = (w - cy) / fy
    x = (u - cx - s * y) / fx
    r0, r1, r2 = (R[0] * x + R[3] * y) + R[6], (R[1] * x + R[4] * y) + R[7], (R[2] * x + R[5] * y) + R[8]
    length = np.sqrt((r0 * r0 + r1 * r1) + r2 * r2)
    return r0 / length, r1 / length, r2 / length


def accum(tab, v, u, w, sel, acc):
    """acc (9 arrays) += the view's terms where sel"""
    d0, d1, d2 = ray(tab, v, u, w)
    c = tab['c'][v]
    dc = (d0 * c[0] + d1 * c[1]) + d2 * c[2]
    new = [acc[0] + (1.0 - d0 * d0), acc[1] - d0 * d1, acc[2] - d0 * d2, acc[3] + (1.0 - d1 * d1), acc[4] - d1 * d2,
           acc[5] + (1.0 - d2 * d2), acc[6] + (c[0] - d0 * dc), acc[7] + (c[1] - d1 * dc), acc[8] + (c[2] - d2 * dc)]
    return [np.where(sel, n, a) for n, a in zip(new, acc)]


def solve(m, b):
    """symmetric 3 x 3 (00 01 02 11 12 22) by cofactors -> (x [3 arrays], ok)"""
    c00, c01, c02 = m[3] * m[5] - m[4] * m[4], m[2] * m[4] - m[1] * m[5], m[1] * m[4] - m[2] * m[3]
    c11, c12, c22 = m[0] * m[5] - m[2] * m[2], m[1] * m[2] - m[0] * m[4], m[0] * m[3] - m[1] * m[1]
    det = (m[0] * c00 + m[1] * c01) + m[2] * c02
    x = [((c00 * b[0] + c01 * b[1]) + c02 * b[2]) / det, ((c01 * b[0] + c11 * b[1]) + c12 * b[2]) / det,
         ((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det]
    return x, (det != 0) & np.isfinite(det) & np.isfinite(x[0]) & np.isfinite(x[1]) & np.isfinite(x[2])


def project(tab, v, u, w, X):
    """X (3 arrays) in view v against the rounded pixels -> dict(z, xn, yn, du, dv, e)"""
    fx, fy, cx, cy, s = tab['k'][v]
    R, t = tab['R'][v], tab['t'][v]
    p0 = ((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + t[0]
    p1 = ((R[3] * X[0] + R[4] * X[1]) + R[5] * X[2]) + t[1]
    z = ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + t[2]
    xn, yn = p0 / z, p1 / z
    du = ((fx * xn + s * yn) + cx) - u
    dv = (fy * yn + cy) - w
    return dict(z=z, xn=xn, yn=yn, du=du, dv=dv, e=du * du + dv * dv)


# ---- per-point loops over sets of views (bool [V,N]) ----------------------------------------------------------------------
def rays_point(tab, pix, sets, views=None):
    n = pix.shape[1]
    acc = [np.zeros(n) for _ in range(9)]
    for v in (range(pix.shape[0]) if views is None else views):
        if sets[v].any():
            acc = accum(tab, v, pix[v, :, 0], pix[v, :, 1], sets[v], acc)
    return solve(acc[:6], acc[6:])


def normal(tab, pix, sets, X):
    """-> (err, front, A [6 arrays], g [3 arrays]) of X over the sets"""
    n = pix.shape[1]
    err, front = np.zeros(n), np.ones(n, bool)
    A, g = [np.zeros(n) for _ in range(6)], [np.zeros(n) for _ in range(3)]
    for v in range(pix.shape[0]):
        sel = sets[v]
        if not sel.any():
            continue
        fx, fy, _, _, s = tab['k'][v]
        R = tab['R'][v]
        r = project(tab, v, pix[v, :, 0], pix[v, :, 1], X)
        err = np.where(sel, err + r['e'], err)
        front = np.where(sel, front & (r['z'] > 0), front)
        ju, jv = [], []
        for k in range(3):
            a, b = (R[k] - r['xn'] * R[6 + k]) / r['z'], (R[3 + k] - r['yn'] * R[6 + k]) / r['z']
            ju.append(fx * a + s * b)
            jv.append(fy * b)
        for i, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            A[i] = np.where(sel, A[i] + (ju[a] * ju[b] + jv[a] * jv[b]), A[i])
        for k in range(3):
            g[k] = np.where(sel, g[k] + (ju[k] * r['du'] + jv[k] * r['dv']), g[k])
    return err, front, A, g


def triangulate(points, cams, poses, visible=None, threshold=4.0, max_cos=None, distance_thresh=50.0, refine_iters=10, robust=True,
                rule=0, found=1, min_angle=1.5, trace=None):
    """The whole call -> dict(X [N,3], used [V,N] uint8, quality [N,5], mask [N] uint8, info [8] int32).  ``trace``: a list
    that receives the summed error of every point before the fit and after every step."""
    points = np.asarray(points, np.float64)
    V, N = points.shape[:2]
    if max_cos is None:
        max_cos = float(np.cos(np.deg2rad(min_angle)))
    if not found:
        return dict(X=np.zeros((N, 3)), used=np.zeros((V, N), np.uint8), quality=np.zeros((N, 5)), mask=np.zeros(N, np.uint8),
                    info=np.zeros(8, np.int32))
    with np.errstate(all='ignore'):
        tab = prepare(cams, poses)
        pix = f32(points)
        thr = np.float32(float(threshold) * float(threshold))
        vis = np.ones((V, N), bool) if visible is None else np.asarray(visible).reshape(V, N) != 0
        S = vis & tab['ok'][:, None] & np.isfinite(pix).all(axis=2)
        count = np.zeros(N, np.int64)
        for v in range(V):
            count = count + S[v]
        enough = count >= 2
        U = S & enough[None]
        if robust:
            best, U = np.zeros(N, np.int64), np.zeros((V, N), bool)
            for i in range(V):
                for j in range(i + 1, V):
                    sel = enough & S[i] & S[j]
                    if not sel.any():
                        continue
                    pair = np.zeros((V, N), bool)
                    pair[i] = pair[j] = sel
                    Xp, ok = rays_point(tab, pix, pair, (i, j))
                    ok = ok & sel
                    inl, cnt = np.zeros((V, N), bool), np.zeros(N, np.int64)
                    for v in range(V):
                        r = project(tab, v, pix[v, :, 0], pix[v, :, 1], Xp)
                        inl[v] = ok & S[v] & (r['z'] > 0) & (r['e'].astype(np.float32) <= thr)
                        cnt = cnt + inl[v]
                    better = cnt > best
                    best = np.where(better, cnt, best)
                    U = np.where(better[None], inl, U)
            enough = enough & (best >= 2)
            U = U & enough[None]
        kept = np.zeros(N, np.int64)
        if rule == 1:
            da, db = ray(tab, 0, pix[0, :, 0], pix[0, :, 1]), ray(tab, 1, pix[1, :, 0], pix[1, :, 1])
            ca, cb = tab['c'][0], tab['c'][1]
            w = [cb[0] - ca[0], cb[1] - ca[1], cb[2] - ca[2]]
            ab = (da[0] * db[0] + da[1] * db[1]) + da[2] * db[2]
            aw, bw = (da[0] * w[0] + da[1] * w[1]) + da[2] * w[2], (db[0] * w[0] + db[1] * w[1]) + db[2] * w[2]
            den = 1.0 - ab * ab
            s = (aw - ab * bw) / den
            X = [ca[0] + s * da[0], ca[1] + s * da[1], ca[2] + s * da[2]]
            solved = enough & (den != 0) & np.isfinite(den) & np.isfinite(X[0]) & np.isfinite(X[1]) & np.isfinite(X[2])
        else:
            X, ok = rays_point(tab, pix, U)
            solved = enough & ok
            if refine_iters > 0:
                err, front, A, g = normal(tab, pix, U, X)
                act = solved & front
                if trace is not None:
                    trace.append(np.where(act, err, np.nan))
                for _ in range(refine_iters):
                    if not act.any():
                        break
                    step, ok = solve(A, g)
                    act = act & ok
                    Xn = [X[0] - step[0], X[1] - step[1], X[2] - step[2]]
                    err_n, front_n, An, gn = normal(tab, pix, U, Xn)
                    act = act & front_n & (err_n < err)
                    X = [np.where(act, a, b) for a, b in zip(Xn, X)]
                    err = np.where(act, err_n, err)
                    A = [np.where(act, a, b) for a, b in zip(An, A)]
                    g = [np.where(act, a, b) for a, b in zip(gn, g)]
                    kept = kept + act
                    if trace is not None:
                        trace.append(np.where(act, err, np.nan))
        # quality over U at X
        ssum, emax = np.zeros(N), np.zeros(N)
        zmin, zmax, cmin = np.full(N, np.inf), np.full(N, -np.inf), np.full(N, np.inf)
        depth_ok, err_ok, nu = np.ones(N, bool), np.ones(N, bool), np.zeros(N, np.int64)
        for v in range(V):
            sel = U[v]
            r = project(tab, v, pix[v, :, 0], pix[v, :, 1], X)
            ssum = np.where(sel, ssum + r['e'], ssum)
            emax = np.where(sel & (r['e'] > emax), r['e'], emax)
            zmin = np.where(sel & (r['z'] < zmin), r['z'], zmin)
            zmax = np.where(sel & (r['z'] > zmax), r['z'], zmax)
            depth_ok = np.where(sel, depth_ok & (r['z'] > 0) & (r['z'] < distance_thresh), depth_ok)
            err_ok = np.where(sel, err_ok & (r['e'].astype(np.float32) <= thr), err_ok)
            nu = nu + sel
        rays = [ray(tab, v, pix[v, :, 0], pix[v, :, 1]) for v in range(V)]
        for i in range(V):
            for j in range(i + 1, V):
                cs = (rays[i][0] * rays[j][0] + rays[i][1] * rays[j][1]) + rays[i][2] * rays[j][2]
                cmin = np.where(U[i] & U[j] & (cs < cmin), cs, cmin)
        good = solved & depth_ok & err_ok & (cmin <= max_cos)
        quality = np.stack([ssum / nu.astype(np.float64), emax, zmin, zmax, cmin], axis=1)
    Xo = np.where(solved[:, None], np.stack(X, axis=1), np.nan)
    quality = np.where(solved[:, None], quality, np.nan)
    used = (U & solved[None]).astype(np.uint8)
    info = np.array([1, good.sum(), (~enough).sum(), (enough & ~solved).sum(), (solved & ~depth_ok).sum(),
                     (solved & depth_ok & ~err_ok).sum(), (solved & depth_ok & err_ok & ~good).sum(), kept[solved].sum()], np.int32)
    return dict(X=Xo, used=used, quality=quality, mask=good.astype(np.uint8), info=info)


def reversed_views(points, cams, poses, visible=None, **kw):
    """the same call with the views in descending order (what the order of the sums changes), its ``used`` turned back"""
    r = triangulate(np.asarray(points)[::-1], np.asarray(cams)[::-1], np.asarray(poses)[::-1],
                    None if visible is None else np.asarray(visible)[::-1], **kw)
    r['used'] = r['used'][::-1]
    return r


# ---- cameras and scenes ---------------------------------------------------------------------------------------------------
def rotation(axis_angle):
    a = np.asarray(axis_angle, np.float64)
    th = np.linalg.norm(a)
    if th == 0:
        return np.eye(3)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def camera_matrix(cam):
    fx, fy, cx, cy, s = cam
    return np.array([[fx, s, cx], [0, fy, cy], [0, 0, 1.0]])


def pose_rows(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3, 1)], axis=1).reshape(12)


def c2w_of(pose):
    P = np.asarray(pose, np.float64).reshape(3, 4)
    m = np.eye(4)
    m[:3, :3] = P[:, :3].T
    m[:3, 3] = -P[:, :3].T @ P[:, 3]
    return m


def pose_of_c2w(c2w):
    m = np.asarray(c2w, np.float64)
    R = m[:3, :3].T
    return pose_rows(R, -R @ m[:3, 3])


def observe(X, cams, poses):
    """exact pixels [V,N,2] and depths [V,N] of the world points X [N,3]"""
    pts, z = [], []
    for cam, pose in zip(cams, poses):
        P = np.asarray(pose).reshape(3, 4)
        Y = X @ P[:, :3].T + P[:, 3]
        q = (Y / Y[:, 2:]) @ camera_matrix(cam).T
        pts.append(q[:, :2])
        z.append(Y[:, 2])
    return np.stack(pts), np.stack(z)


def scene(V, N, noise=0.5, outlier_frac=0.0, seed=0, baseline=0.6):
    """N points 4 to 9 units in front of V cameras on a baseline (camera v near (baseline v, +-0.1, 0.05 v), turned by a few
    degrees; view 0 at the origin), pixel noise of ``noise`` px, and per point up to floor(outlier_frac V) planted outlier
    views (20 to 60 px off, never view 0) -> dict(points [V,N,2] rounded to float32, cams, poses, X, bad [V,N])"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, N) + baseline * (V - 1) / 2, rng.uniform(-1.5, 1.5, N), rng.uniform(4, 9, N)], axis=1)
    cams = np.stack([[500.0 + 3 * v, 510.0 - 2 * v, 320.0 + v, 240.0 - v, 0.25 * (v % 3)] for v in range(V)])
    poses = []
    for v in range(V):
        R = rotation(rng.normal(size=3) * 0.05) if v else np.eye(3)
        c = np.array([baseline * v, 0.1 * (v % 2), 0.05 * v])
        poses.append(pose_rows(R, -R @ c))
    poses = np.stack(poses)
    pts, _ = observe(X, cams, poses)
    pts = pts + rng.normal(size=pts.shape) * noise
    bad = np.zeros((V, N), bool)
    most = int(np.floor(outlier_frac * V))
    if most > 0:
        for p in range(N):
            k = rng.integers(0, most + 1)
            bad[rng.choice(np.arange(1, V), size=k, replace=False), p] = True
        off = rng.uniform(20, 60, size=(int(bad.sum()), 2)) * rng.choice([-1.0, 1.0], size=(int(bad.sum()), 2))
        pts[bad] += off
    return dict(points=f32(pts), cams=cams, poses=poses, X=X, bad=bad)


def dyadic_scene(n=40, seed=0):
    """Three axis-aligned cameras at dyadic centres with power-of-two focal lengths and points on a dyadic grid: every pixel
    is a dyadic rational that float32 holds exactly"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.integers(-8, 9, n) / 4.0, rng.integers(-8, 9, n) / 4.0, np.full(n, 4.0)], axis=1)
    cams = np.array([[256.0, 256.0, 320.0, 240.0, 0.0], [512.0, 256.0, 300.0, 200.0, 0.0], [256.0, 512.0, 256.0, 256.0, 0.0]])
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    poses = np.stack([pose_rows(np.eye(3), [0, 0, 0]), pose_rows(np.eye(3), [-1.0, 0.5, 0.0]), pose_rows(Rz, [0.5, 1.0, 4.0])])
    pts, _ = observe(X, cams, poses)
    assert np.array_equal(pts, f32(pts))
    return dict(points=pts, cams=cams, poses=poses, X=X)


# ---- the demo's route -----------------------------------------------------------------------------------------------------
def demo_rays(pixels, K, c2w, depth=2.0):
    """a point per pixel at ``depth`` along the camera's axis, taken to the world through c2w, minus the camera centre"""
    h = np.concatenate([np.asarray(pixels, np.float64), np.ones((len(pixels), 1))], axis=1)
    cam = (np.linalg.inv(K) @ h.T).T * depth
    world = cam @ c2w[:3, :3].T + c2w[:3, 3]
    return world - c2w[:3, 3]


def nearest_on_ray_a(centre_a, dirs_a, centre_b, dirs_b):
    """the point of every ray A nearest its ray B, the directions of any length (the general form of the rule)"""
    a = dirs_a / np.linalg.norm(dirs_a, axis=1, keepdims=True)
    b = dirs_b / np.linalg.norm(dirs_b, axis=1, keepdims=True)
    w = np.asarray(centre_b) - np.asarray(centre_a)
    aa, bb, ab = (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)
    s = ((a @ w) * bb - ab * (b @ w)) / (aa * bb - ab * ab)
    return centre_a + a * s[:, None]


def demo_route(pts_a, pts_b, K_a, K_b, c2w_a, c2w_b):
    return nearest_on_ray_a(c2w_a[:3, 3], demo_rays(pts_a, K_a, c2w_a), c2w_b[:3, 3], demo_rays(pts_b, K_b, c2w_b))


# what the CPU tests measured on their fixtures (tests/test_structure_cpu.py asserts them); a bound on the device, where one is
# needed, is 1000 times these
ORDER_NOISE_RAYS = 7.7e-15  # largest relative change of X between ascending and descending sums, ray least squares alone (7.641e-15)
ORDER_NOISE = 2.6e-9       # the same after the refit (2.527e-09: the two orders may stop one Gauss-Newton step apart)
DEMO_ROUTES = 1.1e-13     # largest relative difference between rule 1 and the demo's own route (measured 1.072e-13)
