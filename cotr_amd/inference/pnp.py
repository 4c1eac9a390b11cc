"""Absolute camera pose from 3D-2D correspondences on the device: P3P RANSAC with a Gauss-Newton refit on the inliers, and
the lift of pixels of a posed RGB-D capture to the 3D points that feed it.

``solve_pnp_ransac`` has the signature and defaults of ``cv2.solvePnPRansac(objectPoints, imagePoints, cameraMatrix,
distCoeffs, iterationsCount=100, reprojectionError=8.0, confidence=0.99, flags=cv2.SOLVEPNP_P3P)``; ``ransac_pnp`` is the
same call with device tensors, ``lift_pixels`` reads a depth map at pixel positions and un-projects them, and ``localize``
enqueues both back to back: correspondences from a ``Capture`` (image, metric depth, K, c2w) into a new image give the new
image's metric camera-to-world pose in the capture's world frame - the inverse of what ``depth_corrs`` does.  Each is one
call of cotr_amd/csrc/pnp.hip (``cotr_lift_pixels``, ``cotr_ransac_pnp``) on the current device and stream.  The rules are
the library's own: they follow the structure of OpenCV's estimator - 4-point samples, P3P on the first
three, the fourth chooses, reprojection error, adaptive iteration count, a refit on the inliers, the mask not re-evaluated -
with the F path's counter-based sampler, and claim no bit-compatibility with it.  ``rodrigues`` is ``cv2.Rodrigues`` on the
host.  No CPU fallback."""
import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args, _ransac

MAX_REFINE = 64
_TOO_FEW = 'an absolute pose needs at least 4 correspondences'
_SUBJECT = 'the absolute-pose estimator runs'


def _check(threshold, confidence, max_iters, refine_iters):
    _ransac.check_ransac(threshold, confidence, max_iters)
    _args.check_sq_float32(threshold, ransac=True)
    _args.check_int_range('refine_iters', refine_iters, 0, MAX_REFINE)


def _enqueue_lift(lib, pts, n, depth, k, c2w, device):
    out = torch.empty((n, 3), dtype=torch.float64, device=device)
    check_op(lib.cotr_lift_pixels(ptr(depth), int(depth.shape[0]), int(depth.shape[1]), k, ptr(c2w), ptr(pts), n, ptr(out),
                                  _lib.current_stream_ptr()), 'cotr_lift_pixels')
    return out


def _enqueue_pnp(lib, obj, img, n, k, threshold, confidence, max_iters, seed, refine_iters, hypotheses, device):
    scratch, R, mask, out = _ransac.outputs(lib, 'cotr_ransac_pnp_scratch_bytes', n, max_iters, 4, 1, 8, 'hyp_pose', hypotheses, device)
    t = torch.empty(3, dtype=torch.float64, device=device)
    check_op(lib.cotr_ransac_pnp(ptr(obj), ptr(img), n, k, float(threshold), float(confidence), int(max_iters), _ransac.seed64(seed),
                                 int(refine_iters), ptr(R), ptr(t), ptr(mask), ptr(out['info']), ptr(out.get('hyp_pose')),
                                 ptr(out.get('hyp_count')), ptr(out.get('samples')), ptr(scratch), scratch.numel(),
                                 _lib.current_stream_ptr()), 'cotr_ransac_pnp')
    out['R'] = R.view(3, 3)
    out['t'] = t
    out['mask'] = mask.bool()
    return out


def lift_pixels(points, depth, K, c2w=None, device=None):
    """One ``cotr_lift_pixels`` call on the current stream: points [n,2] (x, y) in pixels of the depth map ``depth`` [H,W]
    float32 with the camera matrix ``K`` -> device tensor float64 [n,3]: the depth read at the pixel the point falls in
    (``np.round``: ties to even), X = z K^-1 (x, y, 1) of the unrounded point, in world coordinates when the camera-to-world
    pose ``c2w`` [4,4] is given.  Three NaN for a point outside the map or without a finite depth > 0."""
    pts = _args.points(points, 'points', cv2=True)
    n = pts.shape[0]
    if n < 1 or n > _ransac.MAX_POINTS:
        raise ValueError(f'points: between 1 and 2^24 of them, got {n}')
    _args.check_depth(depth)
    k = _args.camera(K, 'K')
    m = _args.pose_matrix(c2w)
    _args.no_cpu_tensors(_SUBJECT, points, depth)
    device = _args.device(device)
    pts, depth, m = on(pts, device), on(depth, device), _args.pose_on(m, device)
    with torch.cuda.device(device):
        return _enqueue_lift(_lib.load_library(), pts, n, depth, k, m, device)


def ransac_pnp(object_points, image_points, K, threshold=8.0, confidence=0.99, max_iters=100, seed=0, refine_iters=10, hypotheses=False,
               device=None):
    """One ``cotr_ransac_pnp`` call on the current stream -> dict of device tensors: R float64 [3,3], t float64 [3]
    (x_cam = R X + t; the chosen P3P candidate after up to ``refine_iters`` Gauss-Newton steps on its inliers), mask bool [n]
    (the candidate's RANSAC inliers, not re-evaluated after the refit), info int32 [8] = (found, best count, iterations run,
    chosen slot, refit steps kept, 0, 0, 0); with hypotheses=True also samples int32 [max_iters, 4], hyp_pose float64
    [max_iters, 9] (rows 1 and 2 of R, then t) and hyp_count int32 [max_iters] (the tables tests check).  K [3,3]
    upper-triangular; threshold in pixels.  An object point with a NaN is never an inlier.  Nothing found: R = 0, t = 0,
    mask = 0, info[0] = 0."""
    img, obj = _args.points(image_points, 'image_points', cv2=True), _args.points(object_points, 'object_points', 3, cv2=True)
    n = img.shape[0]
    _args.count_pairs(obj.shape[0], n, 4, _TOO_FEW, 'object_points', 'image_points')
    k = _args.camera(K, 'K')
    _check(threshold, confidence, max_iters, refine_iters)
    _args.no_cpu_tensors(_SUBJECT, object_points, image_points)
    device = _args.device(device)
    obj, img = on(obj, device), on(img, device)
    with torch.cuda.device(device):
        return _enqueue_pnp(_lib.load_library(), obj, img, n, k, threshold, confidence, max_iters, seed, refine_iters, hypotheses, device)


def rodrigues(x):
    """``cv2.Rodrigues`` without the Jacobian, on the host in float64: a rotation vector ([3], [3,1] or [1,3]) -> R [3,3], or
    a rotation matrix [3,3] -> rotation vector [3,1]."""
    a = np.asarray(x, dtype=np.float64)
    if a.shape == (3, 3):
        U, _, Vt = np.linalg.svd(a)
        R = U @ Vt
        r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        s = np.sqrt((r * r).sum() * 0.25)
        c = min(max((R[0, 0] + R[1, 1] + R[2, 2] - 1.0) * 0.5, -1.0), 1.0)
        theta = np.arccos(c)
        if s < 1e-5:
            if c > 0:
                return np.zeros((3, 1))
            # an angle near pi: the axis from the diagonal of R, its signs from the off-diagonal sums
            r = np.sqrt(np.maximum((np.diag(R) + 1.0) * 0.5, 0.0))
            if R[0, 1] < 0:
                r[1] = -r[1]
            if R[0, 2] < 0:
                r[2] = -r[2]
            if abs(r[0]) < abs(r[1]) and abs(r[0]) < abs(r[2]) and (R[1, 2] > 0) != (r[1] * r[2] > 0):
                r[2] = -r[2]
            return (r * (theta / np.linalg.norm(r))).reshape(3, 1)
        return (r * (theta / (2.0 * s))).reshape(3, 1)
    if a.size != 3:
        raise ValueError(f'rodrigues takes a rotation vector of 3 entries or a [3, 3] matrix, got shape {a.shape}')
    r = a.reshape(3)
    theta = np.linalg.norm(r)
    if theta < np.finfo(np.float64).eps:
        return np.eye(3)
    k = r / theta
    c, s = np.cos(theta), np.sin(theta)
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return c * np.eye(3) + (1.0 - c) * np.outer(k, k) + s * Kx


def solve_pnp_ransac(object_points, image_points, camera_matrix, dist_coeffs=None, iterations_count=100, reprojection_error=8.0,
                     confidence=0.99, seed=0, refine_iters=10):
    """``cv2.solvePnPRansac(objectPoints, imagePoints, cameraMatrix, distCoeffs, iterationsCount=100, reprojectionError=8.0,
    confidence=0.99, flags=cv2.SOLVEPNP_P3P)`` by the rules of DESIGN.md 3h-4 -> (True, rvec float64 [3,1], tvec float64
    [3,1], inliers int32 [k,1]: the indices of the inliers) as cv2 shapes them, or (False, None, None, None) when no pose is
    found.  Lens distortion is not modelled: ``dist_coeffs`` must be None or all zero."""
    if dist_coeffs is not None and np.any(np.asarray(dist_coeffs, dtype=np.float64) != 0):
        raise ValueError('dist_coeffs must be None or zero: lens distortion is not modelled')
    r = ransac_pnp(object_points, image_points, camera_matrix, reprojection_error, confidence, iterations_count, seed, refine_iters)
    if not _args.found_flag(r):
        return False, None, None, None
    inl = np.flatnonzero(r['mask'].cpu().numpy()).astype(np.int32).reshape(-1, 1)
    return True, rodrigues(r['R'].cpu().numpy()), r['t'].cpu().numpy().reshape(3, 1), inl


def localize_tensors(points_a, points_b, depth_a, K_a, c2w_a, K_b, threshold=8.0, confidence=0.99, max_iters=100, seed=0,
                     refine_iters=10, device=None):
    """``cotr_lift_pixels`` then ``cotr_ransac_pnp`` enqueued back to back on the current stream: the second reads the
    first's points on the device, so no host round trip lies between them -> the dict of ``ransac_pnp`` with
    object_points [n,3] besides."""
    pa, pb = _args.points(points_a, 'points_a', cv2=True), _args.points(points_b, 'points_b', cv2=True)
    n = pa.shape[0]
    _args.count_pairs(n, pb.shape[0], 4, _TOO_FEW, 'points_a', 'points_b')
    _args.check_depth(depth_a)
    ka, kb = _args.camera(K_a, 'K_a'), _args.camera(K_b, 'K_b')
    m = _args.pose_matrix(c2w_a)
    _check(threshold, confidence, max_iters, refine_iters)
    _args.no_cpu_tensors(_SUBJECT, points_a, points_b, depth_a)
    device = _args.device(device)
    pa, pb, depth_a, m = on(pa, device), on(pb, device), on(depth_a, device), _args.pose_on(m, device)
    lib = _lib.load_library()
    with torch.cuda.device(device):
        obj = _enqueue_lift(lib, pa, n, depth_a, ka, m, device)
        r = _enqueue_pnp(lib, obj, pb, n, kb, threshold, confidence, max_iters, seed, refine_iters, False, device)
    r['object_points'] = obj
    return r


def localize(points_a, points_b, cap_a, K_b, **ransac_kw):
    """The metric pose of a new image B from its correspondences with a posed RGB-D capture A: ``points_a`` [n,2] pixels of
    ``cap_a`` (a ``cotr_amd.data.Capture``: image, depth, K, c2w) are lifted through its depth map and pose to world points,
    and ``ransac_pnp`` estimates B's pose from them and ``points_b`` [n,2] with the camera matrix ``K_b``, as one device
    sequence -> (c2w_b float64 [4,4]: the inverse of [R|t], in the world frame of ``cap_a``; mask uint8 [n,1]), or (None,
    None) when no pose is found.  ``ransac_kw``: threshold (8.0), confidence (0.99), max_iters (100), seed (0), refine_iters
    (10)."""
    r = localize_tensors(points_a, points_b, cap_a.depth, cap_a.K, cap_a.c2w, K_b, **ransac_kw)
    if not _args.found_flag(r):
        return None, None
    return _args.c2w_from(r['R'], r['t'], invert=True), _args.mask_column(r['mask'])
