"""A numpy float64 restatement of cotr_amd/csrc/photodepth.hip, written from the rule of include/cotr_hip.h:
``photo_depth`` (cotr_photo_depth), vectorised over the pixels that take a step, every sum over taps and views written out in
the device's order and every expression bracketed as the header brackets it, so that the device's bits are reproduced.  It
counts the pixels with a decision within EPS of a threshold or of a tie (``ambiguous``): min_var, min_score, the range, the
winner against the runner-up by the tie rule, den at 0, the clip of the sub-step, and a tap within EPS of an image edge or of an
integer.  The view table, the ray and the projection are those of tests/mvdepth_oracle.py.  Test infrastructure."""
import numpy as np

from tests.mvdepth_oracle import EPS, F32, cam_rows, project, ray, view_table, w2c_rows  # noqa: F401 (cam_rows, w2c_rows: for the callers)


def _near(value, at):
    return np.abs(value - at) < EPS


def grey_of(images):
    """uint8 [..., H, W, 3] -> uint8 [..., H, W] by the integer rule of ``to_grey``: (77 R + 150 G + 29 B + 128) >> 8"""
    c = np.asarray(images).astype(np.int64)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


# ---- scenes -----------------------------------------------------------------------------------------------------------------
_scenes = {}


def scene(H, W, K, seed=0):
    """K + 1 captures on the arc of ``synth_scene`` (the middle one first: the reference) -> dict: caps, grey uint8 [K+1,H,W]
    (``grey_of`` their images), Ks, c2ws, cams [K+1,5], poses [K+1,12], depth float32 [H,W] (the truth).  Cached: callers copy
    before they change anything."""
    key = (H, W, K, seed)
    if key not in _scenes:
        from cotr_amd.utils.synth import synth_scene
        caps = synth_scene(seed, K + 3, H, W)[:K + 1]
        mid = (K + 1) // 2
        caps = [caps[mid]] + caps[:mid] + caps[mid + 1:]
        Ks, c2ws = np.stack([c.K for c in caps]), np.stack([c.c2w for c in caps])
        _scenes[key] = dict(caps=caps, grey=grey_of(np.stack([c.image for c in caps])), Ks=Ks, c2ws=c2ws, cams=cam_rows(Ks), poses=w2c_rows(c2ws),
                            depth=caps[0].depth)
    return _scenes[key]


def perturbed(depth, amount=0.01, seed=0):
    """the depth map times a smooth factor within 1 +- ``amount`` (two slow waves over the map, their phases from ``seed``)"""
    H, W = depth.shape
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, 2)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    wave = 0.5 * (np.sin(2 * np.pi * xs / max(W, 8) * 1.3 + ph[0]) + np.cos(2 * np.pi * ys / max(H, 8) * 0.9 + ph[1]))
    return (depth.astype(np.float64) * (1.0 + amount * wave)).astype(F32)


def plane_scene(H, W, K, depth=6.0, baseline=1.0, focal=None):
    """A textured plane z = ``depth`` seen without noise by a reference camera at the origin and K cameras beside it, all looking
    along z (so the fronto-parallel patch is exact) -> dict like ``scene``.  The images are the texture at every pixel's own point
    of the plane, rounded to uint8."""
    f = float(focal or 2.0 * W)   # a disparity of a third of the width: 1 % of depth moves a neighbour's patch by a third of a pixel at W = 48
    Km = np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    c2ws = []
    for j in range(K + 1):
        m = np.eye(4)
        if j:
            side = (j + 1) // 2 * (1 if j % 2 else -1)
            m[:3, 3] = [baseline * side, 0.13 * baseline * side, 0.0]
        c2ws.append(m)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    imgs = []
    for m in c2ws:
        X = (xs - Km[0, 2]) / f * depth + m[0, 3]
        Y = (ys - Km[1, 2]) / f * depth + m[1, 3]
        period = 7.0 * depth / f   # about 7 pixels
        tex = np.sin(2 * np.pi * X / period) * np.cos(2 * np.pi * Y / (1.3 * period)) + 0.6 * np.sin(2 * np.pi * (X + 0.7 * Y) / (2.9 * period))
        imgs.append(np.clip(np.rint(127.5 + 70.0 * tex), 0, 255).astype(np.uint8))
    Ks, c2ws = np.stack([Km] * (K + 1)), np.stack(c2ws)
    return dict(grey=np.stack(imgs), Ks=Ks, c2ws=c2ws, cams=cam_rows(Ks), poses=w2c_rows(c2ws), depth=np.full((H, W), depth, F32))


# ---- the winner of a sweep -------------------------------------------------------------------------------------------------------
def winner(F, S):
    """F float64 [2 S + 1, n]: f(s_k) of k = -S .. S for n pixels, NaN where it does not exist -> (have bool [n], k* int [n], f(k*),
    the sub-step d, near bool [n]: the winner within EPS of another k's f, den within EPS of 0, or the clip within EPS of its bound)"""
    F = np.asarray(F, np.float64)
    n = F.shape[1]
    ks = [0] + [k for a in range(1, S + 1) for k in (-a, a)]   # the tie rule: the smallest |k|, then the negative one
    best, kb = np.full(n, -np.inf), np.zeros(n, np.int64)
    have = np.zeros(n, bool)
    with np.errstate(all='ignore'):
        for k in ks:
            f = F[k + S]
            take = ~np.isnan(f) & (~have | (f > best))
            best, kb, have = np.where(take, f, best), np.where(take, k, kb), have | take
        near = np.zeros(n, bool)
        for k in range(-S, S + 1):
            f = F[k + S]
            near |= have & ~np.isnan(f) & (kb != k) & _near(f, best)
        cols = np.arange(n)
        inner = have & (np.abs(kb) < S)
        fm, fp = F[np.clip(kb - 1 + S, 0, 2 * S), cols], F[np.clip(kb + 1 + S, 0, 2 * S), cols]
        both = inner & ~np.isnan(fm) & ~np.isnan(fp)
        den = (fm - 2.0 * best) + fp
        step = both & (den < 0)
        raw = 0.5 * (fm - fp) / den
        d = np.where(step, np.minimum(np.maximum(raw, -0.5), 0.5), 0.0)
        near |= both & _near(den, 0.0)
        near |= step & (_near(raw, -0.5) | _near(raw, 0.5))
    return have, kb, np.where(have, best, np.nan), d, near


# ---- cotr_photo_depth ---------------------------------------------------------------------------------------------------------
def _sample(g, u, v, ok):
    """the bilinear sample of image g at (u, v) where ok (0 elsewhere)"""
    H, W = g.shape
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    x0 = np.maximum(np.minimum(np.floor(u).astype(np.int64), W - 2), 0)
    y0 = np.maximum(np.minimum(np.floor(v).astype(np.int64), H - 2), 0)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    au, av = u - x0.astype(np.float64), v - y0.astype(np.float64)
    g = g.astype(np.float64)
    b0 = (1.0 - au) * g[y0, x0] + au * g[y0, x1]
    b1 = (1.0 - au) * g[y1, x0] + au * g[y1, x1]
    return (1.0 - av) * b0 + av * b1


def photo_depth(grey, depth_in, cams, poses, found=None, radius=2, steps=4, sweeps=3, rel_step=0.004, min_var=4.0, min_score=0.5, min_views=1,
                distance_thresh=50.0, keep_input=True):
    """-> dict: depth float32 [H,W], score float32 [H,W], views uint8 [H,W], info int32 [8], ambiguous (pixels with a decision
    within EPS of its threshold), amb bool [H,W] (which), and for the tests what int [H,W] (0 refined, 1 no input depth, 2 rim, 3
    flat, 4 no f in the last sweep, 5 below min_score, 6 dropped by range; -1 where the call is empty), centre float64 [H,W] (the
    depth before it is rounded, 0 where no step was taken) and F (the last sweep's f, [2 S + 1, pixels that took a step])."""
    grey, depth_in = np.asarray(grey), np.asarray(depth_in)
    assert grey.dtype == np.uint8 and grey.ndim == 3 and depth_in.dtype == F32 and depth_in.shape == grey.shape[1:]
    V, H, W = grey.shape
    R, S = int(radius), int(steps)
    views = view_table(cams, poses)
    assert len(views) == V and 1 <= min_views <= V - 1
    flag = 1 if found is None else int(int(np.asarray(found).reshape(-1)[0]) != 0)
    info = np.zeros(8, np.int32)
    info[0] = flag
    depth, score, nviews = np.zeros((H, W), F32), np.full((H, W), np.nan, F32), np.zeros((H, W), np.uint8)
    what, amb_map, centre_map = np.full((H, W), -1, np.int64), np.zeros((H, W), bool), np.zeros((H, W))
    out = dict(depth=depth, score=score, views=nviews, info=info, ambiguous=0, amb=amb_map, what=what, centre=centre_map, F=None)
    if not (flag and views[0]['ok']):
        return out
    N = float((2 * R + 1) ** 2)
    min_var_n = float(min_var) * N
    g0 = grey[0].astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    has = (depth_in > 0) & (depth_in < np.inf)
    rim = (xs < R) | (ys < R) | (xs >= W - R) | (ys >= H - R)
    what[:] = np.where(~has, 1, np.where(rim, 2, 0))
    iy, ix = np.nonzero(has & ~rim)
    taps = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
    with np.errstate(all='ignore'):
        Sa, Saa = np.zeros(len(iy)), np.zeros(len(iy))
        for dy, dx in taps:
            a = g0[iy + dy, ix + dx]
            Sa, Saa = Sa + a, Saa + a * a
        var_a = Saa - Sa * Sa / N
        flat = var_a < min_var_n
        what[iy[flat], ix[flat]] = 3
        amb_map[iy, ix] |= _near(var_a, min_var_n)
        iy, ix, Sa, var_a = iy[~flat], ix[~flat], Sa[~flat], var_a[~flat]
        n = len(iy)
        a_taps = [g0[iy + dy, ix + dx] for dy, dx in taps]
        r_taps = [ray(views[0], (ix + dx).astype(np.float64), (iy + dy).astype(np.float64)) for dy, dx in taps]
        c0 = views[0]['c']
        centre = depth_in[iy, ix].astype(np.float64)
        amb = np.zeros(n, bool)
        h = float(rel_step)
        have, fbest, nbest, F = np.zeros(n, bool), np.full(n, np.nan), np.zeros(n, np.int64), np.full((2 * S + 1, n), np.nan)
        for _ in range(int(sweeps)):
            F = np.full((2 * S + 1, n), np.nan)
            counts = np.zeros((2 * S + 1, n), np.int64)
            for k in range(-S, S + 1):
                s = centre * (1.0 + float(k) * h)
                total, cnt = np.zeros(n), np.zeros(n, np.int64)
                for j in range(1, V):
                    if not views[j]['ok']:
                        continue
                    ok = np.ones(n, bool)
                    Sb, Sbb, Sab = np.zeros(n), np.zeros(n), np.zeros(n)
                    for a, r in zip(a_taps, r_taps):
                        X = [c0[i] + s * r[i] for i in range(3)]
                        pr = project(views[j], 0.0, 0.0, X)
                        z, u, v = pr['z'], pr['du'], pr['dv']
                        inside = (z > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
                        amb |= ok & (_near(z, 0) | ((z > 0) & (_near(u, np.rint(u)) | _near(v, np.rint(v)))))
                        ok &= inside
                        b = _sample(grey[j], u, v, ok)
                        Sb, Sbb, Sab = Sb + b, Sbb + b * b, Sab + a * b
                    var_b = Sbb - Sb * Sb / N
                    amb |= ok & _near(var_b, min_var_n)
                    ok &= var_b >= min_var_n
                    sc = (Sab - Sa * Sb / N) / np.sqrt(var_a * var_b)
                    total, cnt = np.where(ok, total + sc, total), cnt + ok
                exists = cnt >= min_views
                F[k + S] = np.where(exists, total / cnt.astype(np.float64), np.nan)
                counts[k + S] = cnt
            have, kb, fbest, d, near = winner(F, S)
            amb |= near
            nbest = counts[kb + S, np.arange(n)]
            centre = np.where(have, centre * (1.0 + (kb.astype(np.float64) + d) * h), centre)
            h = h * 0.5
        df = centre.astype(F32)
        scored = have & (fbest >= min_score)
        in_range = (df > 0) & (df.astype(np.float64) < distance_thresh)
        amb |= have & _near(fbest, min_score)
        amb |= scored & (_near(df.astype(np.float64), distance_thresh) | _near(df.astype(np.float64), 0.0))
        verdict = np.where(~have, 4, np.where(~scored, 5, np.where(~in_range, 6, 0)))
    what[iy, ix] = verdict
    amb_map[iy, ix] |= amb
    centre_map[iy, ix] = centre
    good = verdict == 0
    if keep_input:
        depth[what > 1] = depth_in[what > 1]
    depth[iy[good], ix[good]] = df[good]
    score[iy[good], ix[good]] = fbest[good].astype(F32)
    nviews[iy[good], ix[good]] = nbest[good].astype(np.uint8)
    info[1:] = [(what == i).sum() for i in range(7)]
    out.update(ambiguous=int(amb_map.sum()), F=F)
    return out
