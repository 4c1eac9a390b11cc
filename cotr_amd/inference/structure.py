"""Structure from known cameras on the device: robust triangulation of correspondences seen in 2 to 32 posed views.

``triangulate_views`` is one ``cotr_triangulate_views`` call (cotr_amd/csrc/structure.hip, rules in DESIGN.md 3h-6) on the
current device and stream: per point the views that agree are chosen by a vote over view pairs, the point is fitted by ray
least squares and refitted on the pixel reprojection error, and the figures a reconstruction filters on come back with it.
``triangulate_points`` is the two-view form after ``relative_pose_tensors`` (R, t straight from the device) or with two
camera-to-world matrices, ``stack_views`` shapes the correspondences of one query set against several images, and
``reconstruct_tensors`` is what ``ZoomEngine.reconstruct`` runs after its correspondences: the last lines of
demo_reconstruction.py (``rule='demo'``: the point on ray A nearest ray B; colours: the mean of the two images at the
floored coordinates over 255) without its viewer.  No CPU fallback."""
import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args, _ransac
from ._args import F64, I32, MAX_VIEWS, U8  # noqa: F401 (MAX_VIEWS: the limit of this module's calls)

MAX_REFINE = 64
RULES = {'rays': 0, 'demo': 1}
_SUBJECT = 'the triangulation runs'


def _check(threshold, min_angle, distance_thresh, refine_iters, robust, rule, V):
    _args.check_positive('threshold', threshold)
    _args.check_sq_float32(threshold)
    if not 0 <= min_angle <= 180:
        raise ValueError(f'min_angle must be in [0, 180] degrees, got {min_angle}')
    _args.check_distance(distance_thresh)
    _args.check_int_range('refine_iters', refine_iters, 0, MAX_REFINE)
    if rule not in RULES:
        raise ValueError(f"rule must be 'rays' or 'demo', got {rule!r}")
    if rule == 'demo' and (V != 2 or robust or refine_iters != 0):
        raise ValueError("rule='demo' takes two views, robust=False and refine_iters=0")


def _enqueue(lib, pts, vis, cams, poses, V, N, found, threshold, max_cos, distance_thresh, refine_iters, robust, rule, device):
    scratch, nbytes = _args.scratch(lib, 'cotr_triangulate_views_scratch_bytes', V, N, device=device)
    X, used, quality, mask, info = _args.empty(device, ((N, 3), F64), ((V, N), U8), ((N, 5), F64), (N, U8), (8, I32))
    check_op(lib.cotr_triangulate_views(ptr(pts), ptr(vis), ptr(cams), ptr(poses), V, N, ptr(found), float(threshold), float(max_cos),
                                        float(distance_thresh), int(refine_iters), int(bool(robust)), RULES[rule], ptr(X), ptr(used),
                                        ptr(quality), ptr(mask), ptr(info), ptr(scratch), nbytes, _lib.current_stream_ptr()),
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
    pts, V, N = _args.view_points(points)
    cams, rows, vis = _args.cam_rows(cameras, V), _args.pose_rows(poses, V), _args.visible(visible, V, N)
    _check(threshold, min_angle, distance_thresh, refine_iters, robust, rule, V)
    _args.no_cpu_tensors(_SUBJECT, points, cameras, poses, visible, found)
    device = _args.device(device)
    pts, cams, rows = on(pts, device, 16), on(cams, device), on(rows, device)
    vis, found = _args.mask_u8(vis, (V, N), device), _args.found_i32(found, device)
    max_cos = float(np.cos(np.deg2rad(float(min_angle))))
    with torch.cuda.device(device):
        return _enqueue(_lib.load_library(), pts, vis, cams, rows, V, N, found, threshold, max_cos, distance_thresh, refine_iters, robust,
                        rule, device)


def _k5(K, what):
    k = _args.camera(K, what)
    return [k[0], k[4], k[2], k[5], k[1]]


def _check_two_view_poses(R, t, c2w1, c2w2):
    """-> ('rt', R, t) as tensors where they were, or ('c2w', [2,12] host array of the inverted matrices)"""
    if (R is None) != (t is None) or (c2w1 is None) != (c2w2 is None) or (R is None) == (c2w1 is None):
        raise ValueError('give either R and t (camera 1 at [I | 0]) or c2w1 and c2w2')
    if R is not None:
        r, tt = _args.flat(R, 'R', 9), _args.flat(t, 't', 3, 'have 3 entries')
        _args.no_cpu_tensors(_SUBJECT, R, t)
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
    _args.no_cpu_tensors(_SUBJECT, points1, points2, kw.get('visible'), kw.get('found'))
    device = _args.device(device)
    poses = _two_view_poses(spec, device)
    pts = torch.stack([p1.to(device), p2.to(device)], dim=0)
    return triangulate_views(pts, np.array([k1, k2]), poses, device=device, **kw)


def triangulate_points(points1, points2, K1, K2=None, R=None, t=None, c2w1=None, c2w2=None, **kw):
    """``triangulate_points_tensors`` with host arrays back -> (X float64 [n,3], mask uint8 [n,1])."""
    r = triangulate_points_tensors(points1, points2, K1, K2, R, t, c2w1, c2w2, **kw)
    return r['X'].cpu().numpy(), _args.mask_column(r['mask'])


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
    c = _args.tensor(corrs).to(dtype=torch.float64)
    if c.dim() != 2 or c.shape[1] != 4:
        raise ValueError(f'corrs must be [N, 4], got shape {tuple(c.shape)}')
    if (c2w_a is None) != (c2w_b is None):
        raise ValueError('give both c2w_a and c2w_b, or neither')
    for img, what in ((img_a, 'img_a'), (img_b, 'img_b')):
        if len(img.shape) != 3 or img.shape[2] != 3:
            raise ValueError(f'{what} must be [H, W, 3], got shape {tuple(img.shape)}')
    if int(bundle_rounds) != bundle_rounds or bundle_rounds < 0:
        raise ValueError(f'bundle_rounds must be an integer >= 0, got {bundle_rounds}')
    device = _args.device(device)
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


def _k3(row):
    """a camera row (fx, fy, cx, cy, skew) -> the [3,3] camera matrix"""
    fx, fy, cx, cy, s = (float(v) for v in row)
    return np.array([[fx, s, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def _check_blocks(blocks, V):
    """-> [(anchor, neighbours, points tensor [1 + k, Q, 2] where it was)], every index checked, and the points as they were given"""
    out, given = [], []
    if not len(blocks):
        raise ValueError('reconstruct_views needs at least one block')
    for block in blocks:
        if not isinstance(block, (tuple, list)) or len(block) != 3 or not hasattr(block[1], '__len__'):
            raise ValueError('a block must be (anchor, neighbours, points [1 + neighbours, Q, 2])')
        a, nbrs, pts = block
        given.append(pts)
        nbrs = [int(b) for b in nbrs]
        t = _args.tensor(pts)
        if t.dim() != 3 or t.shape[2] != 2 or t.shape[0] != 1 + len(nbrs) or not nbrs:
            raise ValueError(f'the points of a block must be [1 + neighbours, Q, 2], got shape {tuple(t.shape)} with {len(nbrs)} neighbours')
        if t.shape[1] < 5:
            raise ValueError(f'a block needs at least 5 queries, got {t.shape[1]}')
        if not 0 <= int(a) < V or any(not 0 <= b < V or b == int(a) for b in nbrs) or len(set(nbrs)) != len(nbrs):
            raise ValueError(f'a block names its anchor and distinct other views in [0, {V}), got anchor {a} and neighbours {nbrs}')
        out.append((int(a), nbrs, t.to(dtype=torch.float64)))
    if sum(len(n) for _, n, _ in out) > V * (V - 1):
        raise ValueError(f'at most V (V - 1) = {V * (V - 1)} view pairs, got {sum(len(n) for _, n, _ in out)}')
    return out, given


def reconstruct_views_tensors(blocks, cameras, V, root=0, pose_kw=None, rotation_kw=None, position_kw=None, bundle_rounds=2, device=None,
                              **kw):
    """The poses of ``V`` views (2 to 32) and the points they see from matched query sets alone, as one device sequence with
    no host wait.  ``blocks``: a list of (anchor view a, neighbour views b_1 .. b_k, points [1 + k, Q, 2] in
    the layout of ``stack_views``: the anchor's queries, then what each neighbour sees of them); ``cameras`` [V,3,3], one [3,3]
    or [V,5] rows, host.  Per (anchor, neighbour) ``relative_pose_tensors`` (``pose_kw``; refine_rounds 4 unless given) gives the
    edge (a, b) its rotation, its inlier count as weight and its found flag; ``average_rotations`` (``rotation_kw``) turns the
    edges into rotations, ``solve_positions`` (``position_kw``) places the centres on the tracks - a block's queries are the
    tracks, visible where the two-view inlier masks say - ``triangulate_views`` (``kw``: threshold, min_angle,
    distance_thresh, refine_iters, robust) fits the points on the resulting poses, and with ``bundle_rounds`` > 0
    ``bundle_adjust_tensors(rounds=bundle_rounds, fixed_views=(root,))`` refines both.  Every found flag is chained on the
    device.  -> dict of device tensors: poses float64 [V,3,4] world-to-camera (the root at [I | 0]; NaN translation for a view
    that was not placed), c2w float64 [V,4,4] (what ``fuse_images`` takes), X float64 [N,3] and mask bool [N] over the N = sum Q
    tracks in block order, located int32 [V], points float64 [V,N,2] and visible bool [V,N] (the tracks as they were solved),
    edges int32 [E,2], and the dicts of the steps: pairs (one per edge), rotations, positions, triangulation, bundle."""
    from .essential import relative_pose_tensors
    _args.check_int_range('V', V, 2, MAX_VIEWS)
    blocks, given = _check_blocks(blocks, V)
    rows = _args.cam_rows(cameras, V)
    if rows.is_cuda:
        raise ValueError('cameras must be host arrays (the two-view estimators read them on the host)')
    if int(bundle_rounds) != bundle_rounds or bundle_rounds < 0:
        raise ValueError(f'bundle_rounds must be an integer >= 0, got {bundle_rounds}')
    _args.check_int_range('root', root, 0, V - 1)
    _args.no_cpu_tensors(_SUBJECT, *given)
    rows = rows.numpy()
    Ks = [_k3(r) for r in rows]
    device = _args.device(device)
    N = sum(int(p.shape[1]) for _, _, p in blocks)
    points = torch.full((V, N, 2), float('nan'), dtype=torch.float64, device=device)
    visible = torch.zeros((V, N), dtype=torch.bool, device=device)
    edges, pairs, at = [], [], 0
    with torch.cuda.device(device):
        for a, nbrs, pts in blocks:
            pts = pts.to(device)
            Q = int(pts.shape[1])
            points[a, at:at + Q] = pts[0]
            for i, b in enumerate(nbrs):
                pose = relative_pose_tensors(pts[0].contiguous(), pts[1 + i].contiguous(), Ks[a], Ks[b], device=device,
                                             **dict(dict(refine_rounds=4), **(pose_kw or {})))
                points[b, at:at + Q] = pts[1 + i]
                visible[b, at:at + Q] = pose['mask']
                visible[a, at:at + Q] |= pose['mask']
                edges.append((a, b))
                pairs.append(pose)
            at += Q
        return _enqueue_view_poses(points, visible, rows, edges, pairs, V, root, rotation_kw, position_kw, bundle_rounds, kw, device)


def _enqueue_view_poses(points, visible, rows, edges, pairs, V, root, rotation_kw, position_kw, bundle_rounds, kw, device):
    """What follows the two-view poses, whoever made the tracks (``reconstruct_views_tensors``, ``tracks.reconstruct_tracks_tensors``):
    points [V,N,2] and visible bool [V,N] on ``device``, ``rows`` the host camera rows, ``edges`` the (i, j) of ``pairs`` (the dicts
    of ``relative_pose_tensors``), every argument checked, inside ``torch.cuda.device(device)`` -> the dict of
    ``reconstruct_views_tensors``"""
    from .bundle import bundle_adjust_tensors
    from .global_pose import average_rotations, solve_positions
    e = torch.tensor(edges, dtype=torch.int32, device=device)
    R_rel = torch.stack([p['R'] for p in pairs])
    weights = torch.stack([p['mask'].sum() for p in pairs]).to(torch.float64)
    found = torch.stack([p['info'][0] for p in pairs])
    rot = average_rotations(R_rel, e, V, weights=weights, found=found, root=root, device=device, **(rotation_kw or {}))
    pos = solve_positions(points, rows, rot['R'], visible=visible, located=rot['located'], found=rot['info'], root=root, device=device,
                          **(position_kw or {}))
    tri = triangulate_views(points, rows, pos['poses'], visible=pos['used'], found=pos['info'], device=device, **kw)
    r = dict(poses=pos['poses'], X=tri['X'], mask=tri['mask'], located=rot['located'], points=points, visible=visible, edges=e, pairs=pairs,
             rotations=rot, positions=pos, triangulation=tri)
    if bundle_rounds > 0:
        ba = bundle_adjust_tensors(points, rows, pos['poses'], tri['X'], visible=tri['used'] & tri['mask'][None], fixed_views=(root,),
                                   rounds=int(bundle_rounds), found=tri['info'], device=device,
                                   **{k: v for k, v in kw.items() if k in ('threshold', 'distance_thresh')})
        r['poses'], r['X'], r['bundle'] = ba['poses'], ba['X'], ba
    Rt = r['poses'][:, :, :3].transpose(1, 2)
    c2w = torch.zeros((V, 4, 4), dtype=torch.float64, device=device)
    c2w[:, :3, :3] = Rt
    c2w[:, :3, 3] = -(Rt @ r['poses'][:, :, 3:])[:, :, 0]
    c2w[:, 3, 3] = 1.0
    r['c2w'] = c2w
    return r
