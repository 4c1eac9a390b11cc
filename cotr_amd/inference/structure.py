"""Structure from known cameras on the device: robust triangulation of correspondences seen in 2 to 32 posed views.

``triangulate_views`` is one ``cotr_triangulate_views`` call (cotr_amd/csrc/structure.hip, rules in DESIGN.md 3h-6) on the
current device and stream: per point the views that agree are chosen by a vote over view pairs, the point is fitted by ray
least squares and refitted on the pixel reprojection error, and the figures a reconstruction filters on come back with it.
``triangulate_points`` is the two-view form after ``relative_pose_tensors`` (R, t straight from the device) or with two
camera-to-world matrices, ``stack_views`` shapes the correspondences of one query set against several images, and
``reconstruct_tensors`` is what ``ZoomEngine.reconstruct`` runs after its correspondences: the last lines of
demo_reconstruction.py (``rule='demo'``: the point on ray A nearest ray B; colours: the mean of the two images at the
floored coordinates over 255) without its viewer.  No CPU fallback."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _ransac
from ._ransac import _device
from .essential import _camera, _check_distance

MAX_VIEWS = 32
MAX_REFINE = 64
RULES = {'rays': 0, 'demo': 1}


def _no_cpu_tensors(*xs):
    if any(torch.is_tensor(x) and not x.is_cuda for x in xs):
        raise _lib.CotrHipError('the triangulation runs on an MI355X only (HIP kernels, no CPU fallback): got a CPU tensor; '
                                'pass a numpy array or move the tensor with .cuda()')


def _tensor(x, dtype=np.float64):
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype)))


def _view_points(points):
    t = _tensor(points)
    if t.dim() != 3 or t.shape[2] != 2:
        raise ValueError(f'points must be [V, N, 2], got shape {tuple(t.shape)}')
    V, N = int(t.shape[0]), int(t.shape[1])
    if not 2 <= V <= MAX_VIEWS:
        raise ValueError(f'between 2 and {MAX_VIEWS} views, got {V}')
    if not 1 <= N <= _ransac.MAX_POINTS:
        raise ValueError(f'between 1 and 2^24 points, got {N}')
    return t.to(dtype=torch.float64), V, N


def _cam_rows(cameras, V):
    """[V,3,3] camera matrices, one [3,3] for every view, or [V,5] rows (fx, fy, cx, cy, skew) -> [V,5] float64 tensor"""
    if torch.is_tensor(cameras) and cameras.is_cuda:
        c = cameras.to(dtype=torch.float64)
        if c.dim() == 3 and tuple(c.shape[1:]) == (3, 3):
            c = torch.stack([c[:, 0, 0], c[:, 1, 1], c[:, 0, 2], c[:, 1, 2], c[:, 0, 1]], dim=1)
    else:
        k = np.asarray(cameras.cpu() if torch.is_tensor(cameras) else cameras, dtype=np.float64)
        if k.shape == (3, 3):
            k = np.broadcast_to(k, (V, 3, 3))
        if k.ndim == 3 and k.shape[1:] == (3, 3):
            k = np.stack([k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2], k[:, 0, 1]], axis=1)
        if k.ndim == 2 and k.shape[1] == 5 and (not np.isfinite(k).all() or (k[:, :2] == 0).any()):
            raise ValueError('cameras must be finite with focal lengths that are not 0')
        c = torch.from_numpy(np.ascontiguousarray(k))
    if c.dim() != 2 or tuple(c.shape) != (V, 5):
        raise ValueError(f'cameras must be [V, 3, 3], [3, 3] or [V, 5] for {V} views, got shape {tuple(np.shape(cameras))}')
    return c


def _pose_rows(poses, V):
    """[V,3,4] or [V,4,4] world-to-camera matrices, or [V,12] -> [V,12] float64 tensor"""
    t = _tensor(poses).to(dtype=torch.float64)
    if t.dim() == 3 and tuple(t.shape[1:]) == (4, 4):
        t = t[:, :3]
    if t.dim() == 3 and tuple(t.shape[1:]) == (3, 4):
        t = t.reshape(t.shape[0], 12)
    if t.dim() != 2 or tuple(t.shape) != (V, 12):
        raise ValueError(f'poses must be [V, 3, 4], [V, 4, 4] or [V, 12] for {V} views, got shape {tuple(np.shape(poses))}')
    return t


def _check(threshold, min_angle, distance_thresh, refine_iters, robust, rule, V):
    if not (threshold > 0 and np.isfinite(threshold)):
        raise ValueError(f'threshold must be finite and > 0, got {threshold}')
    with np.errstate(over='ignore', under='ignore'):
        sq = np.float32(float(threshold) * float(threshold))
    if not (sq > 0 and np.isfinite(sq)):
        raise ValueError(f'the squared threshold must be a finite float32 that is not 0, got threshold {threshold}')
    if not 0 <= min_angle <= 180:
        raise ValueError(f'min_angle must be in [0, 180] degrees, got {min_angle}')
    _check_distance(distance_thresh)
    if not 0 <= int(refine_iters) <= MAX_REFINE or int(refine_iters) != refine_iters:
        raise ValueError(f'refine_iters must be an integer in [0, {MAX_REFINE}], got {refine_iters}')
    if rule not in RULES:
        raise ValueError(f"rule must be 'rays' or 'demo', got {rule!r}")
    if rule == 'demo' and (V != 2 or robust or refine_iters != 0):
        raise ValueError("rule='demo' takes two views, robust=False and refine_iters=0")


def _enqueue(lib, pts, vis, cams, poses, V, N, found, threshold, max_cos, distance_thresh, refine_iters, robust, rule, device):
    nbytes = ctypes.c_size_t()
    check_op(lib.cotr_triangulate_views_scratch_bytes(V, N, ctypes.byref(nbytes)), 'cotr_triangulate_views_scratch_bytes')
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
    X = torch.empty((N, 3), dtype=torch.float64, device=device)
    used = torch.empty((V, N), dtype=torch.uint8, device=device)
    quality = torch.empty((N, 5), dtype=torch.float64, device=device)
    mask = torch.empty(N, dtype=torch.uint8, device=device)
    info = torch.empty(8, dtype=torch.int32, device=device)
    check_op(lib.cotr_triangulate_views(ptr(pts), ptr(vis), ptr(cams), ptr(poses), V, N, ptr(found), float(threshold), float(max_cos),
                                        float(distance_thresh), int(refine_iters), int(bool(robust)), RULES[rule], ptr(X), ptr(used),
                                        ptr(quality), ptr(mask), ptr(info), ptr(scratch), nbytes.value, _lib.current_stream_ptr()),
             'cotr_triangulate_views')
    return dict(X=X, used=used.bool(), quality=quality, mask=mask.bool(), info=info)


def triangulate_views(points, cameras, poses, visible=None, threshold=4.0, min_angle=1.5, distance_thresh=50.0, refine_iters=10,
                      robust=True, rule='rays', found=None, device=None):
    """One ``cotr_triangulate_views`` call on the current stream: points [V,N,2] (x, y) in pixels, the N
    correspondences as each of the V views sees them; cameras [V,3,3] upper-triangular camera matrices (one [3,3] for all, or
    [V,5] rows fx, fy, cx, cy, skew); poses [V,3,4] (or [V,4,4], [V,12]) world-to-camera [R | t]; visible [V,N] (None: every
    view sees every point) -> dict of device tensors: X float64 [N,3] (NaN where no point could be fitted), used bool [V,N]
    (the views the point was fitted on: with ``robust`` the inlier views of the view pair most views agree with at
    ``threshold`` px, otherwise the visible ones), quality float64 [N,5] = (mean and largest squared reprojection error,
    smallest and largest depth, smallest cosine between two rays) over those views, mask bool [N] (fitted, every depth in (0,
    distance_thresh), every error within the threshold, two rays at least ``min_angle`` degrees apart), info int32 [8] =
    (found, points in mask, with too few views, degenerate, dropped by depth, by error, by parallax, Gauss-Newton steps
    kept).  ``refine_iters``: the most Gauss-Newton steps on the pixel error after the ray least squares.  ``rule='demo'``
    (two views, robust=False, refine_iters=0): the point on ray A nearest ray B.  ``found``: a device int32 tensor whose
    first entry 0 zeroes every output (the flag ``relative_pose_tensors`` returns as info)."""
    pts, V, N = _view_points(points)
    cams = _cam_rows(cameras, V)
    rows = _pose_rows(poses, V)
    vis = None
    if visible is not None:
        vis = _tensor(visible, None)
        if tuple(vis.shape) != (V, N):
            raise ValueError(f'visible must be [V, N] = [{V}, {N}], got shape {tuple(vis.shape)}')
    _check(threshold, min_angle, distance_thresh, refine_iters, robust, rule, V)
    _no_cpu_tensors(points, cameras, poses, visible, found)
    device = _device(device)
    pts, cams, rows = on(pts, device, 16), on(cams, device), on(rows, device)
    if vis is not None:
        vis = (on(vis, device) != 0).to(torch.uint8)
    if found is not None:
        found = on(found, device).to(torch.int32).reshape(-1)
    max_cos = float(np.cos(np.deg2rad(float(min_angle))))
    with torch.cuda.device(device):
        return _enqueue(_lib.load_library(), pts, vis, cams, rows, V, N, found, threshold, max_cos, distance_thresh, refine_iters, robust,
                        rule, device)


def _k5(K, what):
    k = _camera(K, what)
    return [k[0], k[4], k[2], k[5], k[1]]


def _check_two_view_poses(R, t, c2w1, c2w2):
    """-> ('rt', R, t) as tensors where they were, or ('c2w', [2,12] host array of the inverted matrices)"""
    if (R is None) != (t is None) or (c2w1 is None) != (c2w2 is None) or (R is None) == (c2w1 is None):
        raise ValueError('give either R and t (camera 1 at [I | 0]) or c2w1 and c2w2')
    if R is not None:
        r, tt = _tensor(R).to(dtype=torch.float64), _tensor(t).to(dtype=torch.float64)
        if r.numel() != 9:
            raise ValueError(f'R must be [3, 3], got shape {tuple(r.shape)}')
        if tt.numel() != 3:
            raise ValueError(f't must have 3 entries, got shape {tuple(tt.shape)}')
        _no_cpu_tensors(R, t)
        return 'rt', r, tt
    rows = []
    for m, what in ((c2w1, 'c2w1'), (c2w2, 'c2w2')):
        m = np.asarray(m.cpu() if torch.is_tensor(m) else m, dtype=np.float64)
        if m.shape != (4, 4) or not np.isfinite(m).all():
            raise ValueError(f'{what} must be a finite [4, 4] matrix, got shape {m.shape}')
        rows.append(np.linalg.inv(m)[:3].reshape(12))
    return 'c2w', np.stack(rows)


def _two_view_poses(spec, device):
    """-> [2,12] float64 device tensor; (R, t) on the device stay there (torch ops only, no host wait)"""
    if spec[0] == 'c2w':
        return torch.from_numpy(spec[1]).to(device)
    first = torch.eye(3, 4, dtype=torch.float64, device=device).reshape(1, 12)
    second = torch.cat([spec[1].to(device).reshape(3, 3), spec[2].to(device).reshape(3, 1)], dim=1).reshape(1, 12)
    return torch.cat([first, second], dim=0)


def triangulate_points_tensors(points1, points2, K1, K2=None, R=None, t=None, c2w1=None, c2w2=None, device=None, **kw):
    """The two-view form of ``triangulate_views`` -> its dict: either ``R``, ``t`` (x2 ~ R x1 + t, camera 1 at [I | 0]; device
    tensors, e.g. straight from ``relative_pose_tensors`` with its info as ``found``, are assembled on the device without a
    host wait) or the two camera-to-world matrices.  ``kw``: visible, threshold, min_angle, distance_thresh, refine_iters,
    robust, rule, found."""
    p1, p2, n = _ransac.pairs(points1, points2, 1, 'at least one correspondence')
    k1 = _k5(K1, 'K1')
    k2 = k1 if K2 is None else _k5(K2, 'K2')
    spec = _check_two_view_poses(R, t, c2w1, c2w2)
    check = dict(threshold=4.0, min_angle=1.5, distance_thresh=50.0, refine_iters=10, robust=True, rule='rays')
    check.update({k: v for k, v in kw.items() if k in check})
    _check(V=2, **check)
    _no_cpu_tensors(points1, points2, kw.get('visible'), kw.get('found'))
    device = _device(device)
    poses = _two_view_poses(spec, device)
    pts = torch.stack([p1.to(device), p2.to(device)], dim=0)
    return triangulate_views(pts, np.array([k1, k2]), poses, device=device, **kw)


def triangulate_points(points1, points2, K1, K2=None, R=None, t=None, c2w1=None, c2w2=None, **kw):
    """``triangulate_points_tensors`` with host arrays back -> (X float64 [n,3], mask uint8 [n,1])."""
    r = triangulate_points_tensors(points1, points2, K1, K2, R, t, c2w1, c2w2, **kw)
    return r['X'].cpu().numpy(), r['mask'].cpu().numpy().astype(np.uint8).reshape(-1, 1)


def stack_views(corrs_list):
    """Correspondences [N,4] (xa, ya, xb, yb) of ONE query set against several images, their rows aligned (as
    ``cotr_corr_multiscale(..., queries_a=q, force=True)`` delivers them) -> points float64 [1 + len, N, 2]: the queries as
    view 0, then each image's points."""
    cs = [np.asarray(c, dtype=np.float64) for c in corrs_list]
    if not cs:
        raise ValueError('stack_views needs at least one set of correspondences')
    for c in cs:
        if c.ndim != 2 or c.shape[1] != 4 or c.shape != cs[0].shape:
            raise ValueError(f'every set of correspondences must be [N, 4] with the same N, got shapes {[x.shape for x in cs]}')
        if not np.array_equal(c[:, :2], cs[0][:, :2]):
            raise ValueError('the query points (columns 0, 1) of every set must be the same rows in the same order')
    return np.stack([cs[0][:, :2]] + [c[:, 2:] for c in cs])


def _colours(img_a, img_b, pa, pb, device):
    """the demo's colours: the images at the floored coordinates, over 255, averaged -> (float64 [n,3], inside bool [n])"""
    cols, inside = [], None
    for img, p in ((img_a, pa), (img_b, pb)):
        im = img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img))
        im = im.to(device)
        ij = torch.floor(p).to(torch.int64)
        ok = (ij[:, 0] >= 0) & (ij[:, 0] < im.shape[1]) & (ij[:, 1] >= 0) & (ij[:, 1] < im.shape[0])
        x, y = ij[:, 0].clamp(0, im.shape[1] - 1), ij[:, 1].clamp(0, im.shape[0] - 1)
        px = im[y, x].to(torch.float64)
        cols.append(px / torch.full_like(px, 255.0))   # a true division: by a Python scalar torch multiplies by 1 / 255
        inside = ok if inside is None else inside & ok
    col = (cols[0] + cols[1]) / 2
    return torch.where(inside[:, None], col, torch.zeros_like(col)), inside


def reconstruct_tensors(corrs, img_a, img_b, K_a, K_b, c2w_a=None, c2w_b=None, rule='rays', pose_kw=None, device=None, bundle_rounds=0,
                        **kw):
    """What follows the correspondences [n,4] of two images: with both camera-to-world poses the demo's triangulation
    (``rule='demo'`` for its own formula), without them ``relative_pose_tensors(**pose_kw)`` and the triangulation in A's frame
    as one device sequence -> dict of device tensors: X [n,3], mask bool [n] (also 0 where a floored coordinate falls
    outside its image), colors float64 [n,3], and the rest of ``triangulate_views``' dict (with pose: the pose dict).
    ``bundle_rounds`` > 0: ``bundle_adjust_tensors`` follows the triangulation as one more call of the same
    device sequence, with that many rounds, view 0 fixed, the observations ``used`` of the points in ``mask`` and the found
    flag chained; X is then the adjusted points, ``poses`` [2,3,4] the adjusted world-to-camera poses and ``bundle`` the rest of
    its dict.  With only view 0 fixed nothing pins the scale: the damping leaves it where the input put it, and the translation
    of view 1 is no longer of unit length.  0 (the default): the outputs are those of the triangulation alone, bit for bit."""
    from .essential import relative_pose_tensors
    c = _tensor(corrs).to(dtype=torch.float64)
    if c.dim() != 2 or c.shape[1] != 4:
        raise ValueError(f'corrs must be [N, 4], got shape {tuple(c.shape)}')
    if (c2w_a is None) != (c2w_b is None):
        raise ValueError('give both c2w_a and c2w_b, or neither')
    for img, what in ((img_a, 'img_a'), (img_b, 'img_b')):
        if len(img.shape) != 3 or img.shape[2] != 3:
            raise ValueError(f'{what} must be [H, W, 3], got shape {tuple(img.shape)}')
    if int(bundle_rounds) != bundle_rounds or bundle_rounds < 0:
        raise ValueError(f'bundle_rounds must be an integer >= 0, got {bundle_rounds}')
    device = _device(device)
    c = c.to(device)
    pa, pb = c[:, :2].contiguous(), c[:, 2:].contiguous()
    if rule == 'demo':
        kw = dict(dict(robust=False, refine_iters=0), **kw)
    with torch.cuda.device(device):
        if c2w_a is not None:
            r = triangulate_points_tensors(pa, pb, K_a, K_b, c2w1=c2w_a, c2w2=c2w_b, rule=rule, device=device, **kw)
            spec = _check_two_view_poses(None, None, c2w_a, c2w_b)
        else:
            pose = relative_pose_tensors(pa, pb, K_a, K_b, device=device, **dict(dict(refine_rounds=4), **(pose_kw or {})))
            r = triangulate_points_tensors(pa, pb, K_a, K_b, R=pose['R'], t=pose['t'], found=pose['info'], rule=rule, device=device, **kw)
            r['pose'] = pose
            spec = ('rt', pose['R'], pose['t'])
        if bundle_rounds > 0:
            from .bundle import bundle_adjust_tensors
            k_a = _k5(K_a, 'K_a')
            ba = bundle_adjust_tensors(torch.stack([pa, pb], dim=0), np.array([k_a, k_a if K_b is None else _k5(K_b, 'K_b')]),
                                       _two_view_poses(spec, device), r['X'], visible=r['used'] & r['mask'][None], fixed_views=(0,),
                                       rounds=int(bundle_rounds), found=r['info'], device=device,
                                       **{k: v for k, v in kw.items() if k in ('threshold', 'distance_thresh')})
            r['X'], r['poses'] = ba['X'], ba['poses']
            r['bundle'] = dict(used=ba['used'], stats=ba['stats'], info=ba['info'])
        r['colors'], inside = _colours(img_a, img_b, pa, pb, device)
        r['mask'] = r['mask'] & inside
    r['corrs'] = c
    return r
