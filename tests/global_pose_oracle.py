"""numpy restatement of the rules of DESIGN.md 3h-19 (cotr_average_rotations and cotr_solve_positions in
cotr_amd/csrc/global_pose.hip): the dead edges, the greedy tree, the annealed robust steps on the graph with their log and
exp, and for the positions the rays, the sets of the rounds, the per-point blocks, the reduced matrix, the Cholesky by columns
(chol.h restated), both runs of inverse iteration, sign, scale and every output.

The order of the sums is this file's own and documented: ``order='asc'`` sums a view's edges, a point's views and the points
in ascending index, ``order='desc'`` in descending index; the sums over the points are ``np.add.reduce`` over the points so
ordered (numpy's pairwise sum).  The device sums per thread, wavefront and chunk, a third order, so it is held to 1000 times the
noise measured between these two (the *_NOISE constants below, measured by tests/test_global_pose_cpu.py, and the *_BOUND
they give), not to bit equality; the integers are compared exactly.  Also the fixtures of the tests.  numpy only.  Test
infrastructure."""
import numpy as np

from tests import structure_oracle as so

MAX_VIEWS = 32
PIVOT_TOL = 1e-9
DEG = np.pi / 180.0
AR_DEFAULTS = dict(iters=12, sigma0=32 * DEG, sigma_end=1 * DEG, edge_thresh=3 * DEG)
SP_DEFAULTS = dict(threshold=4.0, rounds=3, min_obs=8, power_iters=16)

# The order noise: the largest difference between order='asc' and order='desc' over the fixtures of
# tests/test_global_pose_cpu.py::test_order_noise (which prints them and asserts they are not above these), each relative to
# the largest magnitude of the compared array (the rotation results as rotation_differences states).  The device is held to 1000 times these.
AR_STEP_NOISE = 1.6e-16      # R after one step
AR_RUN_NOISE = 6e-15       # R, |r_e| and the cost after 12 steps
SP_ROUND_NOISE = 8e-14     # C, X, the cost after one round (the eigenvector's condition is in it); lambda0, lambda1 relative to the largest diagonal entry of S
SP_RUN_NOISE = 9e-15       # the same after 3 rounds
AR_STEP_BOUND, AR_RUN_BOUND = 1000 * AR_STEP_NOISE, 1000 * AR_RUN_NOISE
SP_ROUND_BOUND, SP_RUN_BOUND = 1000 * SP_ROUND_NOISE, 1000 * SP_RUN_NOISE


# ---- rotations ------------------------------------------------------------------------------------------------------------
def log_so3(M):
    """the rule of gp_log -> r [3]"""
    M = np.asarray(M, np.float64).reshape(9)
    a = np.array([(M[7] - M[5]) / 2.0, (M[2] - M[6]) / 2.0, (M[3] - M[1]) / 2.0])
    s = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    c = (((M[0] + M[4]) + M[8]) - 1.0) / 2.0
    th = np.arctan2(s, c)
    if s > 1e-8:
        return a * (th / s)
    if c > 0.0:
        return a
    k = 0
    if M[4] > M[k * 4]:
        k = 1
    if M[8] > M[k * 4]:
        k = 2
    b = np.array([M[i * 3 + k] + (1.0 if i == k else 0.0) for i in range(3)])
    return th * (b / np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]))


def exp_so3(w):
    """the matrix of rodrigues.h: exp([w]x)"""
    w = np.asarray(w, np.float64)
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    a, b = (np.sin(th) / th, (1.0 - np.cos(th)) / th2) if th > 1e-8 else (1.0, 0.5)
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + a * W + b * (W @ W)


def norm3(r):
    return float(np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]))


def chol_solve(S, b, admit):
    """chol.h restated: the Cholesky by columns of the symmetric S with b carried as one more row, then the back substitution
    -> (x, L) or (None, None) at the first pivot ``admit(col, pivot)`` refuses"""
    m = S.shape[0]
    L = np.zeros((m + 1, m))
    L[:m] = np.tril(S)
    L[m] = b
    for col in range(m):
        if not admit(col, L[col, col]):
            return None, None
        d = np.sqrt(L[col, col])
        L[col + 1:, col] = L[col + 1:, col] / d
        L[col, col] = d
        for i in range(col + 1, m + 1):
            end = i if i < m else m - 1
            L[i, col + 1:end + 1] -= L[i, col] * L[col + 1:end + 1, col]
    return back(L), L


def forward(L, b):
    """ch_forward: row m <- the forward solve of a fresh right-hand side"""
    m = L.shape[1]
    L[m] = b
    for col in range(m):
        y = L[m, col] / L[col, col]
        L[m, col] = y
        L[m, col + 1:] -= y * L[col + 1:m, col]


def back(L):
    m = L.shape[1]
    y = L[m].copy()
    x = np.zeros(m)
    for col in range(m - 1, -1, -1):
        x[col] = y[col] / L[col, col]
        y[:col] -= L[col, :col] * x[col]
    return x


def dead_edges(R_rel, edges, n, weights, found):
    E = len(edges)
    w = np.ones(E) if weights is None else np.asarray(weights, np.float64)
    ok = (edges[:, 0] >= 0) & (edges[:, 0] < n) & (edges[:, 1] >= 0) & (edges[:, 1] < n) & (edges[:, 0] != edges[:, 1])
    if found is not None:
        ok &= np.asarray(found) != 0
    with np.errstate(invalid='ignore'):
        ok &= (w > 0) & np.isfinite(w) & np.isfinite(R_rel.reshape(E, 9)).all(axis=1)
    return ok, np.where(ok, w, 0.0)


def greedy_tree(R_rel, edges, n, live, wt, root):
    R = np.full((n, 3, 3), np.nan)
    R[root] = np.eye(3)
    lr, parent = np.full(n, -1), np.full(n, -1)
    lr[root] = 0
    for k in range(1, n):
        new = {}
        for v in range(n):
            if lr[v] >= 0:
                continue
            best, bw = -1, 0.0
            for e in range(len(edges)):
                if not live[e]:
                    continue
                a, b = edges[e]
                other = b if a == v else (a if b == v else -1)
                if other < 0 or lr[other] < 0 or lr[other] >= k:
                    continue
                if wt[e] > bw:
                    bw, best = wt[e], e
            if best >= 0:
                new[v] = (R_rel[best] @ R[edges[best][0]] if edges[best][1] == v else R_rel[best].T @ R[edges[best][1]], best)
        for v, (Rv, e) in new.items():
            R[v], lr[v], parent[v] = Rv, k, e
    return R, lr, parent


def laplacian_step(n, edges, part, ew, er, free, order='asc'):
    """the normal system of one step over the free views (in index order) -> (S [3F,3F], b [3F], diag0 [3F])"""
    F = len(free)
    slot = {v: i for i, v in enumerate(free)}
    lap, rhs = np.zeros((n, n)), np.zeros((n, 3))
    idx = range(len(edges)) if order == 'asc' else range(len(edges) - 1, -1, -1)
    for v in range(n):
        d, g = 0.0, np.zeros(3)
        for e in idx:
            if not part[e]:
                continue
            a, b = edges[e]
            if a != v and b != v:
                continue
            d = d + ew[e]
            lap[v, b if a == v else a] -= ew[e]
            g = g - ew[e] * er[e] if a == v else g + ew[e] * er[e]
        lap[v, v], rhs[v] = d, g
    S, b = np.zeros((3 * F, 3 * F)), np.zeros(3 * F)
    for v in free:
        for u in free:
            for c in range(3):
                S[3 * slot[v] + c, 3 * slot[u] + c] = lap[v, u]
        b[3 * slot[v]:3 * slot[v] + 3] = rhs[v]
    return S, b, np.diag(S).copy()


def average_rotations(R_rel, edges, n, weights=None, found=None, root=0, iters=12, sigma0=32 * DEG, sigma_end=1 * DEG,
                      edge_thresh=3 * DEG, order='asc'):
    """The whole call -> dict(R [n,3,3], edge [E,4], view_info [n,4] int32, info [8] int32, stats [2], tree [n,3,3]: the
    rotations of the greedy start, parent [n]: the edge each view took them through, -1 for the root and a view never reached)."""
    R_rel = np.asarray(R_rel, np.float64).reshape(-1, 3, 3)
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    E = len(edges)
    live, wt = dead_edges(R_rel, edges, n, weights, found)
    R, lr, parent = greedy_tree(R_rel, edges, n, live, wt, root)
    tree = R.copy()
    free = [v for v in range(n) if v != root and lr[v] >= 0]
    part = np.array([bool(live[e]) and lr[edges[e][0]] >= 0 and lr[edges[e][1]] >= 0 for e in range(E)])
    ew, rn, er = wt.copy(), np.full(E, np.nan), np.zeros((E, 3))
    steps = reason = 0
    k = 0
    while True:
        for e in np.flatnonzero(part):
            er[e] = log_so3(R[edges[e][1]].T @ (R_rel[e] @ R[edges[e][0]]))
            rn[e] = norm3(er[e])
        if k == iters:
            break
        if not free:
            reason = 1
            break
        sigma = max(sigma_end, np.ldexp(sigma0, -k))
        nw = ew.copy()
        for e in np.flatnonzero(part):
            d = 1.0 + (rn[e] / sigma) ** 2
            nw[e] = wt[e] / (d * d)
        S, b, diag0 = laplacian_step(n, edges, part, nw, er, free, order)
        x, _ = chol_solve(S, b, lambda col, p: np.isfinite(p) and p > 0.0 and p > PIVOT_TOL * diag0[col])
        if x is None:
            reason = 2
            break
        ew = nw                                                   # the step is taken: its weights are the last ones
        for i, v in enumerate(free):
            R[v] = (exp_so3(-x[3 * i:3 * i + 3]) @ R[v].T).T
        steps += 1
        k += 1
    with np.errstate(invalid='ignore'):
        inl = part & (rn <= edge_thresh)
    edge = np.stack([np.where(part, rn, np.nan), np.where(part, ew, 0.0), live.astype(np.float64), inl.astype(np.float64)], axis=1)
    view_info = np.zeros((n, 4), np.int32)
    for v in range(n):
        touch = live & ((edges[:, 0] == v) | (edges[:, 1] == v))
        view_info[v] = (lr[v] >= 0, lr[v], touch.sum(), (touch & inl).sum())
    cost = 0.0
    for e in range(E):
        if part[e]:
            cost = cost + ew[e] * (rn[e] * rn[e])
    info = np.array([len(free) >= 1 and reason != 2, len(free) + 1, live.sum(), inl.sum(), steps, reason, 0, 0], np.int32)
    return dict(R=R, edge=edge, view_info=view_info, info=info, stats=np.array([cost, rn[inl].max() if inl.any() else 0.0]), tree=tree, parent=parent)


def rotation_error_deg(R, truth, root=0):
    """the largest angle between R_v and truth_v truth_root^T over the located views, in degrees"""
    worst = 0.0
    for v in range(len(R)):
        if np.isfinite(R[v]).all():
            worst = max(worst, norm3(log_so3((R[v].T @ (truth[v] @ truth[root].T)))) / DEG)
    return worst


# ---- positions ------------------------------------------------------------------------------------------------------------
def sym_full(P):
    """[...,6] (00 01 02 11 12 22) -> [...,3,3]"""
    return np.stack([np.stack([P[..., 0], P[..., 1], P[..., 2]], -1), np.stack([P[..., 1], P[..., 3], P[..., 4]], -1),
                     np.stack([P[..., 2], P[..., 4], P[..., 5]], -1)], -2)


def symv(P, x):
    return np.stack([(P[..., 0] * x[..., 0] + P[..., 1] * x[..., 1]) + P[..., 2] * x[..., 2],
                     (P[..., 1] * x[..., 0] + P[..., 3] * x[..., 1]) + P[..., 4] * x[..., 2],
                     (P[..., 2] * x[..., 0] + P[..., 4] * x[..., 1]) + P[..., 5] * x[..., 2]], -1)


def cofactors(m):
    c = np.stack([m[..., 3] * m[..., 5] - m[..., 4] * m[..., 4], m[..., 2] * m[..., 4] - m[..., 1] * m[..., 5],
                  m[..., 1] * m[..., 4] - m[..., 2] * m[..., 3], m[..., 0] * m[..., 5] - m[..., 2] * m[..., 2],
                  m[..., 1] * m[..., 2] - m[..., 0] * m[..., 4], m[..., 0] * m[..., 3] - m[..., 1] * m[..., 1]], -1)
    return c, (m[..., 0] * c[..., 0] + m[..., 1] * c[..., 1]) + m[..., 2] * c[..., 2]


def rays(points, cams, R):
    """-> (d [V,N,3] unit rays in the world, finite [V,N]: both rounded coordinates are finite)"""
    pix = so.f32(points)
    V = pix.shape[0]
    d = np.zeros(pix.shape[:2] + (3,))
    with np.errstate(all='ignore'):
        for v in range(V):
            tab = dict(k=cams, R=np.asarray(R, np.float64).reshape(V, 9))
            d[v] = np.stack(so.ray(tab, v, pix[v, :, 0], pix[v, :, 1]), axis=1)
    return d, np.isfinite(pix).all(axis=2)


def proj(d):
    return np.stack([1.0 - d[..., 0] * d[..., 0], -(d[..., 0] * d[..., 1]), -(d[..., 0] * d[..., 2]), 1.0 - d[..., 1] * d[..., 1],
                     -(d[..., 1] * d[..., 2]), 1.0 - d[..., 2] * d[..., 2]], -1)


def psum(a, order):
    """the sum over the points (axis 0) in this file's order"""
    return np.add.reduce(a if order == 'asc' else a[::-1], axis=0)


def start_vector(run, m):
    i = np.arange(m)
    return 1.0 + 0.5 * (i % 3) + 0.125 * (i // 3) if run == 0 else 1.0 + 0.25 * ((i * 5) % 7) - 0.0625 * (i // 3)


def dot(a, b):
    s = 0.0
    for x, y in zip(a, b):
        s = s + x * y
    return s


def inverse_iteration(S, power_iters):
    """-> dict(ok, mu, lam0, lam1, v0, v1): Cholesky of S + mu I and the two runs, as sp_solve_kernel"""
    m = S.shape[0]
    mu = 1e-12 * max(0.0, float(np.diag(S).max()))
    x = start_vector(0, m)
    x = x / np.sqrt(dot(x, x))
    y, L = chol_solve(S + mu * np.eye(m), x, lambda col, p: p > 0.0 and np.isfinite(p))
    if y is None:
        return dict(ok=False, mu=mu)
    lam, vec = [0.0, 0.0], [None, None]
    for run in range(2):
        if run == 1:
            v0 = vec[0]
            x = start_vector(1, m)
            x = x - dot(x, v0) * v0
            x = x / np.sqrt(dot(x, x))
        for it in range(power_iters):
            if run == 1 or it > 0:
                forward(L, x)
                y = back(L)
            if run == 1:
                y = y - dot(y, v0) * v0
            with np.errstate(all='ignore'):
                lam[run] = 1.0 / dot(x, y) - mu
                x = y / np.sqrt(dot(y, y))
        vec[run] = x
    return dict(ok=True, mu=mu, lam0=lam[0], lam1=lam[1], v0=vec[0], v1=vec[1])


def reduced_matrix(P, used, Ainv, free, order='asc'):
    """S over the free views (in index order) from P [V,N,6], the set used [V,N] and A_p^-1 [N,6]"""
    F = len(free)
    S = np.zeros((3 * F, 3 * F))
    Af = Ainv
    for a, v in enumerate(free):
        rows_v = sym_full(P[v])
        for b, w in enumerate(free):
            if b < a:
                continue
            both = used[v] & used[w]
            Y = np.zeros((3, 3))
            if both.any():
                per = np.stack([symv(P[w][both], symv(Af[both], rows_v[both][:, i])) for i in range(3)], axis=1)   # [n,3,3]
                Y = psum(per, order)
            if a == b:
                U = sym_full(psum(P[v][used[v]], order)) if used[v].any() else np.zeros((3, 3))
                blk = U - Y
                blk = np.tril(blk) + np.tril(blk, -1).T
                S[3 * a:3 * a + 3, 3 * a:3 * a + 3] = blk
            else:
                S[3 * a:3 * a + 3, 3 * b:3 * b + 3] = -Y
                S[3 * b:3 * b + 3, 3 * a:3 * a + 3] = -Y.T
    return S


def solve_positions(points, cams, R, visible=None, located=None, found=1, root=0, threshold=4.0, rounds=3, min_obs=8, power_iters=16,
                    order='asc', trace=None):
    """The whole call -> dict(C [V,3], poses [V,12], X [N,3], used [V,N] uint8, stats [4], info [8] int32).  ``trace``: a list that
    receives per round dict(used, S, mu, lam0, lam1, margin: the smallest relative distance of an observation's angle from its
    threshold in the round's selection, inf in round 1, near: the observations within 10 % of it)."""
    points = np.asarray(points, np.float64)
    V, N = points.shape[:2]
    cams = np.asarray(cams, np.float64).reshape(V, 5)
    R = np.asarray(R, np.float64).reshape(V, 9)
    zero = dict(C=np.zeros((V, 3)), poses=np.zeros((V, 12)), X=np.zeros((N, 3)), used=np.zeros((V, N), np.uint8), stats=np.zeros(4),
                info=np.zeros(8, np.int32))
    valid = np.isfinite(cams).all(axis=1) & (cams[:, 0] != 0) & (cams[:, 1] != 0) & np.isfinite(R).all(axis=1)
    if located is not None:
        valid &= np.asarray(located) != 0
    if not found or not valid[root]:
        return zero
    d, finite = rays(points, cams, np.where(valid[:, None], R, 0.0))
    P = proj(d)
    vis = np.ones((V, N), bool) if visible is None else np.asarray(visible) != 0
    eligible = vis & finite & valid[:, None]
    vorder = list(range(V)) if order == 'asc' else list(range(V - 1, -1, -1))
    C = X = None
    out = None
    for rnd in range(rounds):
        sel, margin, near = eligible.copy(), np.inf, np.zeros((V, N), bool)
        if rnd > 0:
            with np.errstate(all='ignore'):
                e = X[None] - C[:, None]
                dep = (d[..., 0] * e[..., 0] + d[..., 1] * e[..., 1]) + d[..., 2] * e[..., 2]
                cr = np.stack([d[..., 1] * e[..., 2] - d[..., 2] * e[..., 1], d[..., 2] * e[..., 0] - d[..., 0] * e[..., 2],
                               d[..., 0] * e[..., 1] - d[..., 1] * e[..., 0]], -1)
                ang = np.arctan2(np.sqrt((cr[..., 0] ** 2 + cr[..., 1] ** 2) + cr[..., 2] ** 2), dep)
                thr = (threshold / np.sqrt(np.abs(cams[:, 0] * cams[:, 1])))[:, None]
                keep = (dep > 0.0) & (ang <= thr)
                rel = np.abs(ang - thr) / thr
                if (eligible & np.isfinite(rel)).any():
                    margin = float(rel[eligible & np.isfinite(rel)].min())
                    near = eligible & np.isfinite(rel) & (rel < 0.1)
            sel &= keep
        counts = sel.sum(axis=1)
        placed = valid & ((np.arange(V) == root) | (counts >= min_obs))
        sel &= placed[:, None]
        A = np.zeros((N, 6))
        for v in vorder:
            A = np.where(sel[v][:, None], A + P[v], A)
        with np.errstate(all='ignore'):
            cof, det = cofactors(A)
            go = (sel.sum(axis=0) >= 2) & (det != 0) & np.isfinite(det)
            Ainv = np.where(go[:, None], cof / det[:, None], 0.0)
        used = sel & go[None]
        free = [v for v in range(V) if v != root and placed[v]]
        dropped = int((valid & ~placed).sum())
        info = np.array([0, used.sum(), 0, dropped, go.sum(), 0, 0, rnd + 1], np.int32)
        fail = dict(C=np.full((V, 3), np.nan), poses=np.concatenate([R.reshape(V, 3, 3), np.full((V, 3, 1), np.nan)], axis=2).reshape(V, 12),
                    X=np.full((N, 3), np.nan), used=used.astype(np.uint8), stats=np.zeros(4), info=info)
        if not free:
            return fail
        S = reduced_matrix(P, used, Ainv, free, order)
        eig = inverse_iteration(S, power_iters)
        if trace is not None:
            trace.append(dict(used=used.copy(), S=S, margin=margin, near=near, free=free, **{k: eig.get(k) for k in ('mu', 'lam0', 'lam1', 'v0', 'v1')}))
        if not eig['ok']:
            return fail
        Craw = np.full((V, 3), np.nan)
        Craw[root] = 0.0
        for i, v in enumerate(free):
            Craw[v] = eig['v0'][3 * i:3 * i + 3]
        b = np.zeros((N, 3))
        for v in vorder:
            b = np.where(used[v][:, None], b + symv(P[v], np.broadcast_to(Craw[v], (N, 3))), b)
        Xraw = np.where(go[:, None], symv(Ainv, b), np.nan)
        with np.errstate(all='ignore'):
            e = Xraw[None] - Craw[:, None]
            dep = (d[..., 0] * e[..., 0] + d[..., 1] * e[..., 1]) + d[..., 2] * e[..., 2]
            q = e - d * dep[..., None]
            sq = (q[..., 0] ** 2 + q[..., 1] ** 2) + q[..., 2] ** 2
        per_point = np.zeros(N)
        for v in vorder:
            per_point = np.where(used[v], per_point + sq[v], per_point)
        cost = float(psum(per_point, order))
        pos, neg = int((used & (dep > 0)).sum()), int((used & (dep < 0)).sum())
        flip = neg > pos
        ss = 0.0
        for v in (free if order == 'asc' else free[::-1]):
            ss = ss + ((Craw[v, 0] ** 2 + Craw[v, 1] ** 2) + Craw[v, 2] ** 2)
        s2 = len(free) / ss
        s = -np.sqrt(s2) if flip else np.sqrt(s2)
        C = Craw * s
        C[root] = 0.0
        X = Xraw * s
        t = np.stack([-((R[:, 3 * r] * C[:, 0] + R[:, 3 * r + 1] * C[:, 1]) + R[:, 3 * r + 2] * C[:, 2]) for r in range(3)], axis=1)
        t[root] = 0.0
        poses = np.concatenate([R.reshape(V, 3, 3), t[:, :, None]], axis=2).reshape(V, 12)
        info[0], info[2], info[5], info[6] = 1, len(free) + 1, neg if flip else pos, pos if flip else neg
        out = dict(C=C, poses=poses, X=X, used=used.astype(np.uint8), stats=np.array([eig['lam0'], eig['lam1'], cost * s2, 0.0]), info=info)
    return out


# ---- the gauge ------------------------------------------------------------------------------------------------------------
def centre_error(C, truth_poses, root=0):
    """the largest distance between the placed centres and the true ones after the similarity gauge: the truth moved into the
    root's frame (C_v - C_root, turned by R_root) and scaled by the least-squares scale onto C"""
    P = np.asarray(truth_poses, np.float64).reshape(-1, 3, 4)
    Ct = np.stack([-(p[:, :3].T @ p[:, 3]) for p in P])
    Ct = (Ct - Ct[root]) @ P[root][:, :3].T
    ok = np.isfinite(C).all(axis=1)
    s = (C[ok] * Ct[ok]).sum() / (Ct[ok] * Ct[ok]).sum()
    return float(np.abs(C[ok] - s * Ct[ok]).max()), float(s)


# ---- the fixtures: the recipes of the issue's prototype -------------------------------------------------------------------
SHAPES = [(3, 12), (3, 64), (5, 257), (8, 300), (32, 65)]


def true_rotations(sc):
    return np.asarray(sc['poses'], np.float64).reshape(-1, 3, 4)[:, :, :3]


def graph_fixture(V, N, plant=True, noise_deg=0.3, seed=None):
    """edges (i, j), i < j, j - i <= 3; R_ij = R_j R_i^T with ``noise_deg`` normal noise per axis; with ``plant`` one fifth of the
    non-consecutive edges (rounded down: none at 3 views) turned by a further ~20 degrees per axis -> dict(sc, edges [E,2]
    int32, R_rel [E,3,3], planted bool [E], truth [V,3,3])"""
    sc = so.scene(V, N, seed=100 * V + N, outlier_frac=0.25)
    rng = np.random.default_rng(7 * (100 * V + N) + 1 if seed is None else seed)
    Rt = true_rotations(sc)
    edges = np.array([(i, j) for i in range(V) for j in range(i + 1, min(V, i + 4))], np.int32)
    far = np.flatnonzero(edges[:, 1] - edges[:, 0] > 1)
    planted = np.zeros(len(edges), bool)
    if plant and far.size:
        planted[rng.choice(far, size=far.size // 5, replace=False)] = True
    R_rel = []
    for e, (i, j) in enumerate(edges):
        M = Rt[j] @ Rt[i].T
        M = exp_so3(rng.normal(size=3) * noise_deg * DEG) @ M
        if planted[e]:
            M = exp_so3(rng.normal(loc=20.0, scale=3.0, size=3) * rng.choice([-1.0, 1.0], size=3) * DEG) @ M
        R_rel.append(M)
    return dict(sc=sc, edges=edges, R_rel=np.stack(R_rel), planted=planted, truth=Rt)


def position_fixture(V, N, hidden=0.03, R=None):
    """``visible`` = the planted-outlier mask of the scene removed, plus ``hidden`` of the rest moved by 6 to 12 px and left in; R: the rotations
    the solve is given (None: the true ones)"""
    sc = so.scene(V, N, seed=100 * V + N, outlier_frac=0.25)
    rng = np.random.default_rng(11 * (100 * V + N) + 5)
    pts = sc['points'].copy()
    visible = ~sc['bad']
    hide = visible & (rng.uniform(size=visible.shape) < hidden)
    hide[0] = False
    k = int(hide.sum())
    ang = rng.uniform(0, 2 * np.pi, k)
    pts[hide] += (rng.uniform(6, 12, k)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1))
    fx = dict(sc=sc, points=so.f32(pts), cams=sc['cams'], visible=visible, hidden=hide, R=true_rotations(sc) if R is None else R)
    # the condition of the tests, met by construction: a point with an observation within 10 % of its angle threshold in any
    # round of the restatement's run is taken out of ``visible`` altogether, until a run has none
    for _ in range(8):
        trace = []
        solve_positions(fx['points'], fx['cams'], fx['R'], visible=fx['visible'], trace=trace)
        near = np.any([t['near'] for t in trace], axis=0).any(axis=0)
        if not near.any():
            return fx
        fx['visible'] = fx['visible'] & ~near[None]
    raise AssertionError(f'position_fixture({V}, {N}) keeps observations near the threshold')


def clean_fixture(V, N):
    """noise-free observations of the scene, rounded to float32 as every input"""
    sc = so.scene(V, N, seed=100 * V + N, noise=0.0)
    return dict(sc=sc, points=sc['points'], cams=sc['cams'], R=true_rotations(sc))


# ---- the fixtures of the shape sweeps -------------------------------------------------------------------------------------
AR_SHAPES = [(2, 1), (2, 2), (3, 1), (3, 3), (5, 1), (5, 3), (5, 20)] + [(32, E) for E in (1, 3, 63, 64, 65, 255, 256, 257, 992)]


def random_graph(n, E, seed=None):
    """E edges over n views with 0.3 degree noise: a chain from view 0 first (as far as E reaches), then random ordered pairs,
    so repeated and reversed pairs occur; integer weights with ties; from E = 16 on one edge of every dead kind (an index out of
    range, i = j, found 0, a weight of 0, a NaN weight, a NaN and an infinite matrix entry) -> dict(R_rel, edges int32, weights,
    found int32, truth, dead: the indices made dead)"""
    rng = np.random.default_rng(1000 * n + E if seed is None else seed)
    truth = np.stack([so.rotation(rng.normal(size=3) * 0.3) if v else np.eye(3) for v in range(n)])
    edges = [(v, v + 1) if v % 2 == 0 else (v + 1, v) for v in range(min(E, n - 1))]
    while len(edges) < E:
        a, b = rng.choice(n, size=2, replace=False)
        edges.append((int(a), int(b)))
    edges = np.array(edges, np.int32)
    R_rel = np.stack([exp_so3(rng.normal(size=3) * 0.3 * DEG) @ truth[j] @ truth[i].T for i, j in edges])
    weights = rng.integers(20, 40, E).astype(np.float64)
    found = np.ones(E, np.int32)
    dead = []
    if E >= 16:
        dead = [int(e) for e in rng.choice(np.arange(n - 1, E) if E > n + 8 else np.arange(E), size=7, replace=False)]
        edges[dead[0], 1] = n
        edges[dead[1], 1] = edges[dead[1], 0]
        found[dead[2]] = 0
        weights[dead[3]] = 0.0
        weights[dead[4]] = np.nan
        R_rel[dead[5], 1, 1] = np.nan
        R_rel[dead[6], 0, 2] = np.inf
    return dict(R_rel=R_rel, edges=edges, weights=weights, found=found, truth=truth, dead=dead)


def singular_graph():
    """three views whose root is held by two weak, conflicting copies of one edge (10 degrees apart, weight 6.2e-10 each against 1 on
    the edge 1-2): as sigma shrinks their robust weights fall, and at the third step the last pivot is below 1e-9 of its diagonal
    entry - stop reason 2 after two steps"""
    T = [np.eye(3), so.rotation([0.1, 0.2, -0.1]), so.rotation([-0.2, 0.1, 0.3])]
    R01 = T[1] @ T[0].T
    return dict(R_rel=np.stack([R01, exp_so3(np.array([10 * DEG, 0.0, 0.0])) @ R01, T[2] @ T[1].T]), edges=np.array([(0, 1), (0, 1), (1, 2)], np.int32),
                weights=np.array([6.2e-10, 6.2e-10, 1.0]))


SP_NS = [1, 4, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]   # 256: a workgroup of points, 2048: a chunk of the block sums
SP_VS = [2, 3, 5]


# a shape whose first scene the restatement does not find determined (lambda1 / lambda0 about 5 at 5 views of 4 points) takes the
# next seed at which it is, so that no shape from 4 points on goes without the comparison of C and X
STEP_SEEDS = {(5, 4): 1}


def step_fixture(V, N):
    """the scene at 0.5 px noise with rotations 0.1 degree off -> dict(points, cams, R, visibles: (name, visible) for None and a
    random 80 %, min_obs: 8 from 16 points on, 2 below, 1 at one point (where two observations are all there is: the solution is
    not determined, the call still succeeds and its eigenvalues are compared))"""
    seed = STEP_SEEDS.get((V, N), 0)
    sc = so.scene(V, N, seed=100 * V + N + 1000 * seed)
    rng = np.random.default_rng(13 * (100 * V + N) + 2 + seed)
    R = np.stack([exp_so3(rng.normal(size=3) * 0.1 * DEG) @ Rv if v else Rv for v, Rv in enumerate(true_rotations(sc))])
    vis = rng.uniform(size=(V, N)) < 0.8
    return dict(sc=sc, points=sc['points'], cams=sc['cams'], R=R, visibles=[('all', None), ('80%', vis)], min_obs=8 if N >= 16 else (2 if N > 1 else 1))


def determined(tr):
    """the restatement's own verdict on a round: the smallest eigenvalue is apart from the next (a factor of 10), so the centres
    are what the input fixes and not what rounding does"""
    return tr['lam1'] is not None and tr['lam1'] >= 10.0 * max(tr['lam0'], 0.0) and tr['lam1'] > 1e-9 * max(float(np.diag(tr['S']).max()), 1e-300)


def rel(a, b, floor=1e-300):
    """the largest difference relative to the largest magnitude of b (at least ``floor``); NaN must sit where NaN sits"""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    ok = ~np.isnan(b)
    return float(np.abs(a[ok] - b[ok]).max() / max(np.abs(b[ok]).max(), floor)) if ok.any() else 0.0


def rotation_differences(got, want):
    """what two results of the rotation averaging are compared by, in the noise measurement and on the device alike: R and the
    robust weights relative to their largest magnitude; the residuals in radians (they are read off products of matrix entries of
    unit size, so their error does not shrink with them: on a tree they are rounding alone); the cost sum w r^2 relative to
    2 sum w |r|, which is what a residual error of that size moves it by"""
    part = ~np.isnan(want['edge'][:, 0])
    slope = 2.0 * float((want['edge'][part, 1] * want['edge'][part, 0]).sum())
    return dict(R=rel(got['R'], want['R']), residual=rel(got['edge'][:, 0], want['edge'][:, 0], 1.0), weight=rel(got['edge'][:, 1], want['edge'][:, 1]),
                cost=abs(float(got['stats'][0]) - float(want['stats'][0])) / max(slope, 1e-300), worst=rel(got['stats'][1:], want['stats'][1:], 1.0))
