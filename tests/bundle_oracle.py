"""numpy restatement of the bundle adjustment rules of DESIGN.md 3h-7 (cotr_bundle_adjust in cotr_amd/csrc/bundle.hip): the
round's set with its frozen views and landmarks, the exact Jacobians, the per-point blocks with the damped cofactor inverse, the
reduced system by the Schur complement, its Cholesky solve, the back-substitution, the candidate and the keep/reject rule with
its damping schedule.  Vectorised over the points; scenes, ``prepare``, ``project`` and ``rotation`` are those of
tests/structure_oracle.py.

Summation order (its own, documented): every per-point sum runs over the views in ascending order, term by term as the device
writes it; every sum over points (the entries of S and b, the cost) is one sequential pass over the points, ascending with
``order='asc'`` and descending with ``order='desc'`` (np.cumsum, which adds one term after the other).  The device sums the
same terms per thread, wavefront and chunk, a third order, so it is held to 1000 times the noise measured between the two
orders here (the constants at the end), not to bit equality.  ``dense_step`` solves the full damped (6 F + 3 N) normal system
instead, as a second route to the same step.  numpy only.  Test infrastructure."""
import numpy as np

from tests import structure_oracle as so

MIN_VIEW_OBS = 4
LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12
TRI = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def psum(a, order='asc'):
    """sequential sum over the last axis, ascending or descending"""
    a = np.asarray(a, np.float64)
    if a.shape[-1] == 0:
        return np.zeros(a.shape[:-1])
    return np.cumsum(a if order == 'asc' else a[..., ::-1], axis=-1)[..., -1]


def rodrigues_rotate(w, R):
    """R <- exp([w]x) R, the rule of cotr_amd/csrc/rodrigues.h; R [9] row-major"""
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    a, b = (np.sin(th) / th, (1.0 - np.cos(th)) / th2) if th > 1e-8 else (1.0, 0.5)
    W = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    E = [(((1.0 if i == j else 0.0) + a * W[i * 3 + j]) + b * ((W[i * 3] * W[j] + W[i * 3 + 1] * W[3 + j]) + W[i * 3 + 2] * W[6 + j]))
         for i in range(3) for j in range(3)]
    return np.array([(E[i * 3] * R[j] + E[i * 3 + 1] * R[3 + j]) + E[i * 3 + 2] * R[6 + j] for i in range(3) for j in range(3)])


def observe(tab, v, u, w, X):
    """residual and exact Jacobians of X (3 arrays) in view v -> (proj dict, cu [6], cv [6], pu [3], pv [3]): rows (u, v) of
    d(du, dv) / d(w, dt) and of d(du, dv) / dX"""
    r = so.project(tab, v, u, w, X)
    fx, fy, _, _, s = tab['k'][v]
    R = tab['R'][v]
    pu, pv = [], []
    for k in range(3):
        a, b = (R[k] - r['xn'] * R[6 + k]) / r['z'], (R[3 + k] - r['yn'] * R[6 + k]) / r['z']
        pu.append(fx * a + s * b)
        pv.append(fy * b)
    q0, q1, q2 = ((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2], (R[3] * X[0] + R[4] * X[1]) + R[5] * X[2],
                  (R[6] * X[0] + R[7] * X[1]) + R[8] * X[2])
    a0, a2, b2 = 1.0 / r['z'], (-r['xn']) / r['z'], (-r['yn']) / r['z']
    u0, u1, u2 = fx * a0, s * a0, fx * a2 + s * b2
    v1, v2 = fy * a0, fy * b2
    cu = [u2 * q1 - u1 * q2, u0 * q2 - u2 * q0, u1 * q0 - u0 * q1, u0, u1, u2]
    cv = [v2 * q1 - v1 * q2, -(v2 * q0), v1 * q0, np.zeros_like(v1), v1, v2]
    return r, cu, cv, pu, pv


def table(cams, poses):
    return so.prepare(cams, np.asarray(poses, np.float64).reshape(-1, 12))


def select(tab, pix, vis, X, fixed, first, thr, dist):
    """the round's set -> (set bool [V,N], frozen bool [V], landmark bool [N], counts before the starved views leave, margin: the
    smallest relative distance of an eligible observation's e from the threshold and z from the distance; inf in round 1)"""
    V, N = pix.shape[:2]
    Xl = [X[:, 0], X[:, 1], X[:, 2]]
    Xok = np.isfinite(X).all(axis=1)
    sets = np.zeros((V, N), bool)
    margin = np.inf
    for v in range(V):
        el = vis[v] & tab['ok'][v] & np.isfinite(pix[v]).all(axis=1) & Xok
        r = so.project(tab, v, pix[v, :, 0], pix[v, :, 1], Xl)
        take = r['z'] > 0 if first else (r['z'] > 0) & (r['z'] < dist) & (r['e'].astype(np.float32) <= thr)
        sets[v] = el & take
        if not first and el.any():
            margin = min(margin, float(np.abs(r['e'][el] / np.float64(thr) - 1.0).min()), float(np.abs(r['z'][el] / dist - 1.0).min()))
    counts = sets.sum(axis=1)
    frozen = ~fixed & (counts < MIN_VIEW_OBS)
    sets[frozen] = False
    return sets, frozen, sets.sum(axis=0) < 2, counts, margin


def cost(tab, pix, sets, X, order='asc'):
    """-> (summed e over the set, every observation in front)"""
    V, N = pix.shape[:2]
    Xl = [X[:, 0], X[:, 1], X[:, 2]]
    e, front = np.zeros(N), True
    for v in range(V):
        if not sets[v].any():
            continue
        r = so.project(tab, v, pix[v, :, 0], pix[v, :, 1], Xl)
        e = np.where(sets[v], e + r['e'], e)
        front = front and bool((r['z'][sets[v]] > 0).all())
    return psum(e, order), front


def point_blocks(tab, pix, sets, landmark, X, lam):
    """-> (Vinv [6 arrays] of the damped V_p (0 where the point takes no step), h = Vinv g [3 arrays], moves bool [N], A, g)"""
    V, N = pix.shape[:2]
    Xl = [X[:, 0], X[:, 1], X[:, 2]]
    A, g = [np.zeros(N) for _ in range(6)], [np.zeros(N) for _ in range(3)]
    for v in range(V):
        sel = sets[v]
        if not sel.any():
            continue
        r, _, _, pu, pv = observe(tab, v, pix[v, :, 0], pix[v, :, 1], Xl)
        for i, (a, b) in enumerate(TRI):
            A[i] = np.where(sel, A[i] + (pu[a] * pu[b] + pv[a] * pv[b]), A[i])
        for k in range(3):
            g[k] = np.where(sel, g[k] + (pu[k] * r['du'] + pv[k] * r['dv']), g[k])
    damp = 1.0 + lam
    m = [A[0] * damp, A[1], A[2], A[3] * damp, A[4], A[5] * damp]
    c00, c01, c02 = m[3] * m[5] - m[4] * m[4], m[2] * m[4] - m[1] * m[5], m[1] * m[4] - m[2] * m[3]
    c11, c12, c22 = m[0] * m[5] - m[2] * m[2], m[1] * m[2] - m[0] * m[4], m[0] * m[3] - m[1] * m[1]
    det = (m[0] * c00 + m[1] * c01) + m[2] * c02
    go = ~landmark & (det != 0) & np.isfinite(det)
    z = np.zeros(N)
    Vinv = [np.where(go, c / det, z) for c in (c00, c01, c02, c11, c12, c22)]
    h = [np.where(go, ((c00 * g[0] + c01 * g[1]) + c02 * g[2]) / det, z), np.where(go, ((c01 * g[0] + c11 * g[1]) + c12 * g[2]) / det, z),
         np.where(go, ((c02 * g[0] + c12 * g[1]) + c22 * g[2]) / det, z)]
    return Vinv, h, go, A, g


def view_blocks(tab, pix, sets, free, X):
    """per free view: W [6,3,N] = Jc^T Jp, cu, cv [6,N], du, dv"""
    Xl = [X[:, 0], X[:, 1], X[:, 2]]
    out = {}
    for v in np.flatnonzero(free):
        r, cu, cv, pu, pv = observe(tab, v, pix[v, :, 0], pix[v, :, 1], Xl)
        W = np.stack([np.stack([cu[i] * pu[k] + cv[i] * pv[k] for k in range(3)]) for i in range(6)])
        out[v] = dict(W=W, cu=np.stack(cu), cv=np.stack(cv), du=r['du'], dv=r['dv'])
    return out


def reduced_system(tab, pix, sets, landmark, free, X, lam, order='asc'):
    """-> dict(S [m,m], b [m], Vinv, h, moves, blocks, views): the Schur complement of the points"""
    Vinv, h, moves, _, _ = point_blocks(tab, pix, sets, landmark, X, lam)
    blocks = view_blocks(tab, pix, sets, free, X)
    views = list(np.flatnonzero(free))
    m = 6 * len(views)
    S, b = np.zeros((m, m)), np.zeros(m)
    damp = 1.0 + lam
    i00, i01, i02, i11, i12, i22 = Vinv
    T = {}
    for v in views:
        W = blocks[v]['W']
        T[v] = np.stack([(W[:, 0] * i00 + W[:, 1] * i01) + W[:, 2] * i02, (W[:, 0] * i01 + W[:, 1] * i11) + W[:, 2] * i12,
                         (W[:, 0] * i02 + W[:, 1] * i12) + W[:, 2] * i22], axis=1)   # [6,3,N]
    with np.errstate(all='ignore'):
        for a, v in enumerate(views):
            bv, sel = blocks[v], sets[v]
            U = np.zeros((6, 6))
            for i in range(6):
                for j in range(i, 6):
                    U[i, j] = U[j, i] = psum(np.where(sel, bv['cu'][i] * bv['cu'][j] + bv['cv'][i] * bv['cv'][j], 0.0), order)
            # b_v: per point first the view's own term, then minus W h (the order of the device's accumulator)
            gv = bv['cu'] * bv['du'] + bv['cv'] * bv['dv']
            wh = (bv['W'][:, 0] * h[0] + bv['W'][:, 1] * h[1]) + bv['W'][:, 2] * h[2]
            terms = np.stack([np.where(sel, gv, 0.0), np.where(sel & moves, -wh, 0.0)], axis=2).reshape(6, -1)
            b[6 * a:6 * a + 6] = psum(terms, order)
            for c, w in enumerate(views[a:], start=a):
                both = sel & sets[w] & moves
                Tw, Ww = T[v], blocks[w]['W']
                Y = (Tw[:, None, 0] * Ww[None, :, 0] + Tw[:, None, 1] * Ww[None, :, 1]) + Tw[:, None, 2] * Ww[None, :, 2]   # [6,6,N]
                Y = psum(np.where(both[None, None], Y, 0.0), order)
                if w == v:
                    D = np.tril(U * (np.eye(6) * lam + 1.0) - Y)
                    S[6 * a:6 * a + 6, 6 * a:6 * a + 6] = D + np.tril(D, -1).T
                else:
                    S[6 * c:6 * c + 6, 6 * a:6 * a + 6] = -Y.T
                    S[6 * a:6 * a + 6, 6 * c:6 * c + 6] = -Y
    return dict(S=S, b=b, Vinv=Vinv, h=h, moves=moves, blocks=blocks, views=views)


def cholesky_solve(S, b):
    """S x = b by Cholesky, column after column, the right-hand side carried along -> x, or None at a pivot <= 0 or not finite"""
    L, y = np.array(S, np.float64), np.array(b, np.float64)
    m = len(y)
    with np.errstate(all='ignore'):
        for k in range(m):
            piv = L[k, k]
            if not (piv > 0 and np.isfinite(piv)):
                return None
            d = np.sqrt(piv)
            L[k + 1:, k] = L[k + 1:, k] / d
            L[k, k] = d
            y[k] = y[k] / d
            L[k + 1:, k + 1:] -= np.tril(np.outer(L[k + 1:, k], L[k + 1:, k]))
            y[k + 1:] -= y[k] * L[k + 1:, k]
        x = np.zeros(m)
        for k in range(m - 1, -1, -1):
            x[k] = y[k] / L[k, k]
            y[:k] -= L[k, :k] * x[k]
    return x


def back_substitute(sys, sets, dc):
    """-> dX [N,3] (0 where the point takes no step)"""
    N = sets.shape[1]
    a = [np.zeros(N) for _ in range(3)]
    for s, v in enumerate(sys['views']):
        W, d = sys['blocks'][v]['W'], dc[6 * s:6 * s + 6]
        for k in range(3):
            t = ((((W[0, k] * d[0] + W[1, k] * d[1]) + W[2, k] * d[2]) + W[3, k] * d[3]) + W[4, k] * d[4]) + W[5, k] * d[5]
            a[k] = np.where(sets[v], a[k] + t, a[k])
    i00, i01, i02, i11, i12, i22 = sys['Vinv']
    h = sys['h']
    d = [h[0] - ((i00 * a[0] + i01 * a[1]) + i02 * a[2]), h[1] - ((i01 * a[0] + i11 * a[1]) + i12 * a[2]),
         h[2] - ((i02 * a[0] + i12 * a[1]) + i22 * a[2])]
    return np.where(sys['moves'][:, None], np.stack(d, axis=1), 0.0)


def apply_step(poses, X, views, dc, dX, moves):
    """the candidate: the state minus the steps; views and points without a step keep their bits"""
    P = np.array(poses, np.float64).reshape(-1, 3, 4)
    for s, v in enumerate(views):
        d = dc[6 * s:6 * s + 6]
        P[v, :, :3] = rodrigues_rotate(-d[:3], P[v, :, :3].reshape(9)).reshape(3, 3)
        P[v, :, 3] = P[v, :, 3] - d[3:]
    Xn = np.array(X, np.float64)
    Xn[moves] = X[moves] - dX[moves]
    return P.reshape(-1, 12), Xn


def dense_step(tab, pix, sets, landmark, free, X, lam):
    """the same step from the full damped normal system (6 F + 3 N_moving unknowns), solved densely -> (dc, dX [N,3], moves)"""
    _, _, moves, _, _ = point_blocks(tab, pix, sets, landmark, X, lam)
    views = list(np.flatnonzero(free))
    Xl = [X[:, 0], X[:, 1], X[:, 2]]
    N = X.shape[0]
    cols = {p: 6 * len(views) + 3 * i for i, p in enumerate(np.flatnonzero(moves))}
    n = 6 * len(views) + 3 * len(cols)
    rows, res = [], []
    for v in range(pix.shape[0]):
        if not sets[v].any():
            continue
        r, cu, cv, pu, pv = observe(tab, v, pix[v, :, 0], pix[v, :, 1], Xl)
        for p in np.flatnonzero(sets[v]):
            for jc, jp, rr in ((cu, pu, r['du']), (cv, pv, r['dv'])):
                row = np.zeros(n)
                if v in views:
                    s = views.index(v)
                    row[6 * s:6 * s + 6] = [jc[i][p] if np.ndim(jc[i]) else jc[i] for i in range(6)]
                if p in cols:
                    row[cols[p]:cols[p] + 3] = [jp[k][p] for k in range(3)]
                rows.append(row)
                res.append(rr[p])
    J, r = np.array(rows), np.array(res)
    H = J.T @ J
    H[np.diag_indices(n)] *= 1.0 + lam
    d = np.linalg.solve(H, J.T @ r)
    dX = np.zeros((N, 3))
    for p, c in cols.items():
        dX[p] = d[c:c + 3]
    return d[:6 * len(views)], dX, moves


def bundle_adjust(points, cams, poses, X, visible=None, fixed_views=(0,), threshold=4.0, distance_thresh=50.0, rounds=1, iters=10,
                  lambda0=1e-3, found=1, order='asc', trace=None):
    """The whole call -> dict(poses [V,12], X [N,3], used [V,N] uint8, stats [4], info [8] int32; frozen, landmark of the last
    round, margin of ``select`` over the rounds).  ``trace``: a list that receives per iteration dict(round, lam, cost, cand, kept,
    front, solved)."""
    points = np.asarray(points, np.float64)
    V, N = points.shape[:2]
    poses = np.array(poses, np.float64).reshape(V, 12)
    X = np.array(X, np.float64).reshape(N, 3)
    if not found:
        return dict(poses=np.zeros((V, 12)), X=np.zeros((N, 3)), used=np.zeros((V, N), np.uint8), stats=np.zeros(4),
                    info=np.zeros(8, np.int32))
    fixed = np.zeros(V, bool)
    fixed[np.asarray(fixed_views) if np.asarray(fixed_views).dtype != bool else np.flatnonzero(fixed_views)] = True
    pix = so.f32(points)
    thr = np.float32(float(threshold) * float(threshold))
    vis = np.ones((V, N), bool) if visible is None else np.asarray(visible).reshape(V, N) != 0
    kept = rejected = 0
    lam, first_cost, cur, margin = lambda0, 0.0, 0.0, np.inf
    with np.errstate(all='ignore'):
        for rnd in range(rounds):
            tab = table(cams, poses)
            sets, frozen, landmark, _, m = select(tab, pix, vis, X, fixed, rnd == 0, thr, distance_thresh)
            margin = min(margin, m)
            free = ~fixed & ~frozen
            cur, _ = cost(tab, pix, sets, X, order)
            if rnd == 0:
                first_cost = cur
            lam = lambda0
            done = not free.any() or not sets.any()
            for _ in range(iters):
                if done:
                    break
                sys = reduced_system(tab, pix, sets, landmark, free, X, lam, order)
                dc = cholesky_solve(sys['S'], sys['b'])
                solved = dc is not None
                cand, front, ok = np.nan, True, False
                if solved:
                    dX = back_substitute(sys, sets, dc)
                    Pn, Xn = apply_step(poses, X, sys['views'], dc, dX, sys['moves'])
                    tabn = table(cams, Pn)
                    cand, front = cost(tabn, pix, sets, Xn, order)
                    ok = bool(front and cand < cur)
                if trace is not None:
                    trace.append(dict(round=rnd, lam=lam, cost=cur, cand=cand, kept=ok, front=front, solved=solved))
                if ok:
                    poses, X, tab, cur = Pn, Xn, tabn, cand
                    kept += 1
                    lam = max(lam / 10.0, LAMBDA_MIN)
                else:
                    rejected += 1
                    lam = 10.0 * lam
                if lam > LAMBDA_MAX:
                    done = True
    info = np.array([1, sets.sum(), free.sum(), frozen.sum(), landmark.sum(), kept, rejected, rounds], np.int32)
    return dict(poses=poses, X=X, used=sets.astype(np.uint8), stats=np.array([first_cost, cur, lam, 0.0]), info=info,
                frozen=frozen, landmark=landmark, margin=margin)


# ---- fixtures -------------------------------------------------------------------------------------------------------------
def perturbed(sc, rot_deg=0.5, shift=0.02, seed=7, keep=(0, 1)):
    """the scene's poses turned by about rot_deg degrees (a normal axis-angle vector of that scale), turned about their centres, then t moved by about shift,
    the views of ``keep`` left alone"""
    rng = np.random.default_rng(seed)
    out = []
    for v, pose in enumerate(np.asarray(sc['poses']).reshape(-1, 3, 4)):
        if v in keep:
            out.append(pose.reshape(12))
            continue
        w, d = rng.normal(size=3) * np.deg2rad(rot_deg), rng.normal(size=3) * shift
        R = so.rotation(w) @ pose[:, :3]
        out.append(so.pose_rows(R, so.rotation(w) @ pose[:, 3] + d))
    return np.stack(out)


def fixture(V, N, noise=0.0, outlier_frac=0.0, fixed=(0, 1), seed=None):
    """a scene, its perturbed poses, and the triangulation at them (X and its ``used`` as the observation set)"""
    sc = so.scene(V, N, noise=noise, outlier_frac=outlier_frac, seed=100 * V + N if seed is None else seed)
    poses0 = perturbed(sc, keep=fixed)
    tri = so.triangulate(sc['points'], sc['cams'], poses0, threshold=8.0)
    return dict(sc=sc, points=sc['points'], cams=sc['cams'], poses0=poses0, X0=tri['X'], used=tri['used'], fixed=fixed)


def step_fixture(V, N):
    """the fixtures of the one-iteration comparison on the device: 0.5 px noise, view 0 (and view 1 from three views on) fixed"""
    sc = so.scene(V, N, noise=0.5, seed=100 * V + N)
    fixed = (0,) if V == 2 else (0, 1)
    poses0 = perturbed(sc, keep=fixed)
    tri = so.triangulate(sc['points'], sc['cams'], poses0, threshold=8.0)
    rand = np.random.default_rng(V + N).random((V, N)) < 0.8
    return dict(sc=sc, points=sc['points'], cams=sc['cams'], poses0=poses0, X0=tri['X'], used=tri['used'], fixed=fixed,
                visibles=(('all', None), ('random', rand.astype(np.uint8)), ('used', tri['used'])))


def big_fixture(N):
    """32 views, view 0 alone fixed, the others turned and moved so little that each keeps at least 4 observations: all 31 are
    free, the reduced system has its 186 unknowns and all 496 off-diagonal blocks"""
    sc = so.scene(32, N, noise=0.7, outlier_frac=0.25, seed=3200 + N)
    poses0 = perturbed(sc, rot_deg=0.1, shift=0.01, keep=(0,))
    tri = so.triangulate(sc['points'], sc['cams'], poses0, threshold=8.0)
    return dict(sc=sc, points=sc['points'], cams=sc['cams'], poses0=poses0, X0=tri['X'], used=tri['used'], fixed=(0,))


def repeated_fixture(copies=64):
    """one point of the (5, 257) row and its start, ``copies`` times: every view's block has rank 2"""
    fx = fixture(5, 257, 0.7, 0.0)
    return dict(fx, points=np.repeat(fx['points'][:, :1], copies, axis=1), X0=np.repeat(fx['X0'][:1], copies, axis=0),
                used=np.ones((5, copies), np.uint8))


def pose_errors(poses, truth):
    """largest rotation error (degrees) and camera-centre error over the views"""
    rot = cen = 0.0
    for a, b in zip(np.asarray(poses).reshape(-1, 3, 4), np.asarray(truth).reshape(-1, 3, 4)):
        c = np.clip((np.trace(a[:, :3] @ b[:, :3].T) - 1.0) / 2.0, -1.0, 1.0)
        rot = max(rot, float(np.degrees(np.arccos(c))))
        cen = max(cen, float(np.linalg.norm(-a[:, :3].T @ a[:, 3] + b[:, :3].T @ b[:, 3])))
    return rot, cen


# what tests/test_bundle_cpu.py measured on its fixtures (it asserts them); a bound on the device is 1000 times the order noise
SCHUR_ROUTES = 3.7e-12       # Schur step against the dense solve of the full system, 10 times the measured 3.640e-13
ORDER_NOISE_SUMS = 2.3e-15   # largest relative change of S, b and the cost between ascending and descending sums (2.246e-15)
ORDER_NOISE_STEP = 5.0e-13   # of the poses, X and the cost after one iteration (4.996e-13: the sums through the Cholesky solve)
ORDER_NOISE_RUN = 5.0e-10    # after a run of 15 (4.920e-10: at the floor the two orders keep different steps)
STEP_BOUND = 1000 * ORDER_NOISE_STEP
RUN_BOUND = 1000 * ORDER_NOISE_RUN
DECISION_MARGIN = 1e-6       # a keep/reject decision or a threshold is compared only where the restatement clears it by this, relatively
