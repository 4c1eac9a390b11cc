"""Registration of 3D-3D correspondences on the device: 3-point RANSAC on Horn's closed form for a rigid motion or a
similarity, with a closed-form refit on the inliers (robust absolute orientation: Kabsch / Horn / Umeyama).

``ransac_rigid3d`` is one call of cotr_amd/csrc/rigid3d.hip (``cotr_ransac_rigid3d``) with device tensors, ``register_points``
the same with host results, and ``register_captures`` enqueues two ``cotr_lift_pixels`` calls and the registration back to
back: correspondences between two RGB-D captures (image, metric depth, K; the first with its pose) give the second capture's
camera-to-world pose in the first one's world frame, from both depth maps - where ``localize`` uses only the first.  With
``with_scale=True`` the model is a similarity, which puts a reconstruction at unit baseline into a metric frame.  The model
is y = s R x + t; the rules are the library's own.  No CPU fallback."""
import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args, _ransac, icp
from .icp import _enqueue_icp
from .pnp import _enqueue_lift

MAX_ROUNDS = 8
_TOO_FEW = 'a registration needs at least 3 correspondences'
_SUBJECT = 'the 3D registration runs'


def _check(threshold, confidence, max_iters, with_scale, rounds):
    _ransac.check_ransac(threshold, confidence, max_iters)
    _args.check_sq_float32(threshold, ransac=True)
    if with_scale not in (False, True, 0, 1):
        raise ValueError(f'with_scale must be a bool, got {with_scale}')
    _args.check_int_range('rounds', rounds, 0, MAX_ROUNDS)


def _enqueue_rigid3d(lib, src, dst, n, threshold, confidence, max_iters, seed, with_scale, rounds, hypotheses, device):
    scratch, R, mask, out = _ransac.outputs(lib, 'cotr_ransac_rigid3d_scratch_bytes', n, max_iters, 3, 1, 8, 'hyp_model', hypotheses, device)
    t, scale = _args.empty(device, (3, _args.F64), (1, _args.F64))
    check_op(lib.cotr_ransac_rigid3d(ptr(src), ptr(dst), n, float(threshold), float(confidence), int(max_iters), _ransac.seed64(seed),
                                     int(bool(with_scale)), int(rounds), ptr(R), ptr(t), ptr(scale), ptr(mask), ptr(out['info']),
                                     ptr(out.get('hyp_model')), ptr(out.get('hyp_count')), ptr(out.get('samples')), ptr(scratch),
                                     scratch.numel(), _lib.current_stream_ptr()), 'cotr_ransac_rigid3d')
    out['R'] = R.view(3, 3)
    out['t'] = t
    out['scale'] = scale
    out['mask'] = mask.bool()
    return out


def ransac_rigid3d(src, dst, threshold, confidence=0.99, max_iters=100, seed=0, with_scale=False, rounds=2, hypotheses=False, device=None):
    """One ``cotr_ransac_rigid3d`` call on the current stream: src, dst [n,3] corresponding points, taken as float64 -> dict
    of device tensors: R float64 [3,3], t float64 [3], scale float64 [1] (dst = scale R src + t; scale is 1 exactly unless
    ``with_scale``), mask bool [n] (the mask the last executed refit round fitted on; with ``rounds=0`` the RANSAC inliers
    of the chosen candidate), info int32 [8] = (found, best count, iterations run, chosen slot, refit rounds run, points in
    mask, 0, 0); with hypotheses=True also samples int32 [max_iters, 3], hyp_model float64 [max_iters, 9] (rows 1 and 2 of
    scale R, then t) and hyp_count int32 [max_iters] (the tables tests check).  ``threshold``: a distance in dst's units.  A
    pair with a NaN is never an inlier.  Nothing found: R = 0, t = 0, scale = 0, mask = 0, info[0] = 0."""
    s, d = _args.points(src, 'src', 3), _args.points(dst, 'dst', 3)
    n = s.shape[0]
    _args.count_pairs(n, d.shape[0], 3, _TOO_FEW, 'src', 'dst')
    _check(threshold, confidence, max_iters, with_scale, rounds)
    _args.no_cpu_tensors(_SUBJECT, src, dst)
    device = _args.device(device)
    s, d = on(s, device), on(d, device)
    with torch.cuda.device(device):
        return _enqueue_rigid3d(_lib.load_library(), s, d, n, threshold, confidence, max_iters, seed, with_scale, rounds, hypotheses, device)


def register_points(src, dst, threshold, confidence=0.99, max_iters=100, seed=0, with_scale=False, rounds=2):
    """``ransac_rigid3d`` with host results -> (True, T float64 [3,4] = [scale R | t] with dst = T (src, 1), scale float,
    inliers uint8 [n,1]), or (False, None, None, None) when no model is found."""
    r = ransac_rigid3d(src, dst, threshold, confidence, max_iters, seed, with_scale, rounds)
    if not _args.found_flag(r):
        return False, None, None, None
    scale = float(r['scale'].cpu().numpy()[0])
    T = np.concatenate([scale * r['R'].cpu().numpy(), r['t'].cpu().numpy().reshape(3, 1)], axis=1)
    return True, T, scale, _args.mask_column(r['mask'])


def register_captures_tensors(points_a, points_b, depth_a, K_a, c2w_a, depth_b, K_b, threshold=0.05, confidence=0.99, max_iters=100, seed=0,
                              with_scale=False, rounds=2, icp_iters=0, icp_max_dist=None, device=None):
    """Two ``cotr_lift_pixels`` calls (A's pixels through ``c2w_a`` into the world frame, B's into B's camera frame) and
    ``cotr_ransac_rigid3d`` with src = B's points, enqueued back to back on the current stream with no host round trip
    between them -> the dict of ``ransac_rigid3d`` (world = scale R x_b + t) with points_world [n,3] and points_cam_b [n,3]
    besides.  A point without depth on either side is NaN and never an inlier.  ``icp_iters`` > 0: ``cotr_icp_depth`` on both
    depth maps is the next call of the same sequence, started from the sparse result and gated by its info[0]
    (``icp_max_dist``: the association distance, the RANSAC ``threshold`` unless given; the other arguments at the defaults
    of ``icp_depth``): R and t are then the refined pose, R_sparse and t_sparse the sparse one, icp the dict of ``icp_depth``
    (all 0 when no model was found).  Not with ``with_scale``."""
    pa, pb = _args.points(points_a, 'points_a', cv2=True), _args.points(points_b, 'points_b', cv2=True)
    n = pa.shape[0]
    _args.count_pairs(n, pb.shape[0], 3, _TOO_FEW, 'points_a', 'points_b')
    _args.check_depth(depth_a)
    _args.check_depth(depth_b)
    ka, kb = _args.camera(K_a, 'K_a'), _args.camera(K_b, 'K_b')
    m = _args.pose_matrix(c2w_a)
    _check(threshold, confidence, max_iters, with_scale, rounds)
    _args.check_int_range('icp_iters', icp_iters, 0, icp.MAX_ITERS)
    if icp_iters > 0:
        if with_scale:
            raise ValueError('icp_iters > 0 refines a rigid motion: not together with with_scale')
        icp_max_dist = threshold if icp_max_dist is None else icp_max_dist
        _args.check_map(depth_a, 'depth_a')
        _args.check_map(depth_b, 'depth_b')
        icp.check(icp_max_dist, iters=icp_iters)
    _args.no_cpu_tensors(_SUBJECT, points_a, points_b, depth_a, depth_b)
    device = _args.device(device)
    pa, pb, depth_a, depth_b, m = on(pa, device), on(pb, device), on(depth_a, device), on(depth_b, device), _args.pose_on(m, device)
    lib = _lib.load_library()
    with torch.cuda.device(device):
        world = _enqueue_lift(lib, pa, n, depth_a, ka, m, device)
        cam_b = _enqueue_lift(lib, pb, n, depth_b, kb, None, device)
        r = _enqueue_rigid3d(lib, cam_b, world, n, threshold, confidence, max_iters, seed, with_scale, rounds, False, device)
        if icp_iters > 0:
            d = _enqueue_icp(lib, depth_a, ka, depth_b, kb, r['R'], r['t'], m, r['info'], None, icp_max_dist, icp.NORMAL_COS, icp.EDGE,
                             icp.COND_TOL, icp_iters, 1, False, device)
            r['R_sparse'], r['t_sparse'], r['icp'] = r['R'], r['t'], d
            r['R'], r['t'] = d['R'], d['t']
    r['points_world'] = world
    r['points_cam_b'] = cam_b
    return r


def register_captures(points_a, points_b, cap_a, cap_b, **ransac_kw):
    """The metric pose of the RGB-D capture B from its correspondences with the posed RGB-D capture A: ``points_a`` [n,2]
    pixels of ``cap_a`` (a ``cotr_amd.data.Capture``: image, depth, K, c2w) are lifted through its depth map and pose to
    world points, ``points_b`` [n,2] through the depth map of ``cap_b`` to points in B's camera frame (its c2w is not
    read), and the rigid motion between the two clouds is estimated, as one device sequence -> (c2w_b float64 [4,4] in the
    world frame of ``cap_a``; mask uint8 [n,1]), or (None, None) when no model is found.  ``ransac_kw``: threshold (0.05, in
    the depth maps' units), confidence (0.99), max_iters (100), seed (0), with_scale (False; True keeps the scaled rotation
    in c2w_b), rounds (2), icp_iters (0; above 0 the pose is refined on both depth maps by that many point-to-plane steps of
    ``icp_depth`` within the same device sequence), icp_max_dist (the threshold)."""
    r = register_captures_tensors(points_a, points_b, cap_a.depth, cap_a.K, cap_a.c2w, cap_b.depth, cap_b.K, **ransac_kw)
    if not _args.found_flag(r):
        return None, None
    return _args.c2w_from(r['R'], r['t'], float(r['scale'].cpu().numpy()[0])), _args.mask_column(r['mask'])
