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
from . import _ransac
from . import icp as _icp
from ._ransac import _device
from .essential import _camera
from .pnp import _check_depth, _enqueue_lift, _image_points, _pose_matrix

MAX_ROUNDS = 8


def _no_cpu_tensors(*xs):
    if any(torch.is_tensor(x) and not x.is_cuda for x in xs):
        raise _lib.CotrHipError('the 3D registration runs on an MI355X only (HIP kernels, no CPU fallback): got a CPU tensor; '
                                'pass a numpy array or move the tensor with .cuda()')


def _points3(p, what):
    """[N,3] float64 tensor, where it was"""
    t = p if torch.is_tensor(p) else torch.from_numpy(np.ascontiguousarray(np.asarray(p, dtype=np.float64)))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f'{what} must be [N, 3], got shape {tuple(t.shape)}')
    return t.to(dtype=torch.float64)


def _count(n, m, a='src', b='dst'):
    if m != n:
        raise ValueError(f'{a} and {b} must have the same length, got {n} and {m}')
    if n < 3:
        raise ValueError(f'a registration needs at least 3 correspondences, got {n}')
    if n > _ransac.MAX_POINTS:
        raise ValueError(f'at most 2^24 correspondences, got {n}')


def _check(threshold, confidence, max_iters, with_scale, rounds):
    _ransac.check_ransac(threshold, confidence, max_iters)
    with np.errstate(over='ignore', under='ignore'):
        sq = np.float32(float(threshold) * float(threshold))
    if not (sq > 0 and np.isfinite(sq)):
        raise ValueError(f'the squared RANSAC threshold must be a finite float32 that is not 0, got threshold {threshold}')
    if with_scale not in (False, True, 0, 1):
        raise ValueError(f'with_scale must be a bool, got {with_scale}')
    if not 0 <= int(rounds) <= MAX_ROUNDS or int(rounds) != rounds:
        raise ValueError(f'rounds must be an integer in [0, {MAX_ROUNDS}], got {rounds}')


def _enqueue_rigid3d(lib, src, dst, n, threshold, confidence, max_iters, seed, with_scale, rounds, hypotheses, device):
    scratch, R, mask, out = _ransac.outputs(lib.cotr_ransac_rigid3d_scratch_bytes, 'cotr_ransac_rigid3d_scratch_bytes', n, max_iters, 3, 1, 8,
                                            'hyp_model', hypotheses, device)
    t = torch.empty(3, dtype=torch.float64, device=device)
    scale = torch.empty(1, dtype=torch.float64, device=device)
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
    s, d = _points3(src, 'src'), _points3(dst, 'dst')
    n = s.shape[0]
    _count(n, d.shape[0])
    _check(threshold, confidence, max_iters, with_scale, rounds)
    _no_cpu_tensors(src, dst)
    device = _device(device)
    s, d = on(s, device), on(d, device)
    with torch.cuda.device(device):
        return _enqueue_rigid3d(_lib.load_library(), s, d, n, threshold, confidence, max_iters, seed, with_scale, rounds, hypotheses, device)


def register_points(src, dst, threshold, confidence=0.99, max_iters=100, seed=0, with_scale=False, rounds=2):
    """``ransac_rigid3d`` with host results -> (True, T float64 [3,4] = [scale R | t] with dst = T (src, 1), scale float,
    inliers uint8 [n,1]), or (False, None, None, None) when no model is found."""
    r = ransac_rigid3d(src, dst, threshold, confidence, max_iters, seed, with_scale, rounds)
    if not r['info'].cpu().numpy()[0]:
        return False, None, None, None
    scale = float(r['scale'].cpu().numpy()[0])
    T = np.concatenate([scale * r['R'].cpu().numpy(), r['t'].cpu().numpy().reshape(3, 1)], axis=1)
    return True, T, scale, r['mask'].cpu().numpy().astype(np.uint8).reshape(-1, 1)


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
    pa, pb = _image_points(points_a, 'points_a'), _image_points(points_b, 'points_b')
    n = pa.shape[0]
    _count(n, pb.shape[0], 'points_a', 'points_b')
    _check_depth(depth_a)
    _check_depth(depth_b)
    ka, kb = _camera(K_a, 'K_a'), _camera(K_b, 'K_b')
    m = _pose_matrix(c2w_a)
    _check(threshold, confidence, max_iters, with_scale, rounds)
    if not 0 <= icp_iters <= _icp.MAX_ITERS or int(icp_iters) != icp_iters:
        raise ValueError(f'icp_iters must be an integer in [0, {_icp.MAX_ITERS}], got {icp_iters}')
    if icp_iters > 0:
        if with_scale:
            raise ValueError('icp_iters > 0 refines a rigid motion: not together with with_scale')
        icp_max_dist = threshold if icp_max_dist is None else icp_max_dist
        _icp._check_map(depth_a, 'depth_a')
        _icp._check_map(depth_b, 'depth_b')
        _icp._check(icp_max_dist, 0.5, 0.05, 1e-6, icp_iters, 1)
    _no_cpu_tensors(points_a, points_b, depth_a, depth_b)
    device = _device(device)
    pa, pb, depth_a, depth_b = on(pa, device), on(pb, device), on(depth_a, device), on(depth_b, device)
    m = None if m is None else on(m.reshape(16), device)
    lib = _lib.load_library()
    with torch.cuda.device(device):
        world = _enqueue_lift(lib, pa, n, depth_a, ka, m, device)
        cam_b = _enqueue_lift(lib, pb, n, depth_b, kb, None, device)
        r = _enqueue_rigid3d(lib, cam_b, world, n, threshold, confidence, max_iters, seed, with_scale, rounds, False, device)
        if icp_iters > 0:
            d = _icp._enqueue_icp(lib, depth_a, ka, depth_b, kb, r['R'], r['t'], m, r['info'], None, icp_max_dist, 0.5, 0.05, 1e-6,
                                  icp_iters, 1, False, device)
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
    if not r['info'].cpu().numpy()[0]:
        return None, None
    c2w = np.eye(4)
    c2w[:3, :3] = float(r['scale'].cpu().numpy()[0]) * r['R'].cpu().numpy()
    c2w[:3, 3] = r['t'].cpu().numpy()
    return c2w, r['mask'].cpu().numpy().astype(np.uint8).reshape(-1, 1)
