"""Relative camera pose of a wide-baseline pair on the device: essential-matrix RANSAC (five-point minimal solver), then
the pose of the essential matrix by the cheirality count.

``find_essential_mat`` and ``recover_pose`` have the signatures and defaults of ``cv2.findEssentialMat(points1, points2,
cameraMatrix1, None, cameraMatrix2, None, cv2.RANSAC, prob, threshold)`` and ``cv2.recoverPose(E, points1, points2,
cameraMatrix, distanceThresh=50)``, which demo_wbs.py's evaluation calls on the correspondences; each is one call of
cotr_amd/csrc/essential.hip (``cotr_ransac_essential``, ``cotr_recover_pose``) on the current device and stream.
``relative_pose`` enqueues both back to back with no host round trip between them.  The rules are the library's own
(DESIGN.md 3h-3): they follow the structure of OpenCV's estimator - 5-point samples, up to 10 candidates per sample, Sampson
error, adaptive iteration count, no refit, the four (R, t) in its order - with the F path's counter-based sampler, and claim
no bit-compatibility with it.  ``refine_relative_pose`` / ``refine_pose_tensors`` (``cotr_refine_pose``) refit a
pose on its inliers, which cv2's pair does not do: Gauss-Newton on the Sampson error over (R, unit t), the inliers re-counted
between rounds; ``relative_pose(..., refine_rounds=4)`` enqueues it third.  No CPU fallback."""
import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args, _ransac
from ._args import F64, I32, U8

MAX_ITERS = 6553


def _views(points1, points2, K1, K2):
    """-> (points1, points2, n, k1, k2): the pair of point sets and the two cameras (K2 = K1 when None)"""
    p1, p2, n = _ransac.pairs(points1, points2, 5, 'an essential matrix needs at least 5 correspondences')
    k1 = _args.camera(K1, 'K1')
    return p1, p2, n, k1, k1 if K2 is None else _args.camera(K2, 'K2')


def _check_ransac(K1, K2, threshold, confidence, max_iters):
    _ransac.check_ransac(threshold, confidence, max_iters, MAX_ITERS)
    _check_threshold(K1, K2, threshold)


def _check_threshold(K1, K2, threshold):
    _args.check_positive('the RANSAC threshold', threshold)
    thr = threshold / ((K1[0] + K1[4] + K2[0] + K2[4]) / 4.0) if (K1[0] + K1[4] + K2[0] + K2[4]) != 0 else np.inf
    if not (thr * thr > 0 and np.isfinite(thr * thr)):
        raise ValueError('the RANSAC threshold over the mean focal length must be finite and not 0')


def _mask(mask, n):
    m = None if mask is None else _args.tensor(mask, None)
    if m is not None and m.numel() != n:
        raise ValueError(f'mask must have one entry per correspondence, got {m.numel()} for {n}')
    return m


def _enqueue_essential(lib, p1, p2, n, k1, k2, threshold, confidence, max_iters, seed, hypotheses, device):
    scratch, E, mask, out = _ransac.outputs(lib, 'cotr_ransac_essential_scratch_bytes', n, max_iters, 5, 10, 8, 'hyp_E', hypotheses, device)
    check_op(lib.cotr_ransac_essential(ptr(p1), ptr(p2), n, k1, k2, float(threshold), float(confidence), int(max_iters),
                                       _ransac.seed64(seed), ptr(E), ptr(mask), ptr(out['info']), ptr(out.get('hyp_E')),
                                       ptr(out.get('hyp_count')), ptr(out.get('samples')), ptr(scratch), scratch.numel(),
                                       _lib.current_stream_ptr()), 'cotr_ransac_essential')
    out['E'] = E.view(3, 3)
    out['mask_u8'] = mask
    return out


def _enqueue_pose(lib, E, p1, p2, n, k1, k2, distance_thresh, mask, found, device):
    scratch, nbytes = _args.scratch(lib, 'cotr_recover_pose_scratch_bytes', n, device=device)
    R, t, mask_out, info = _args.empty(device, (9, F64), (3, F64), (n, U8), (8, I32))
    check_op(lib.cotr_recover_pose(ptr(E), ptr(p1), ptr(p2), n, k1, k2, float(distance_thresh), ptr(mask), ptr(found), ptr(R), ptr(t),
                                   ptr(mask_out), ptr(info), ptr(scratch), nbytes, _lib.current_stream_ptr()), 'cotr_recover_pose')
    return dict(R=R.view(3, 3), t=t, mask=mask_out.bool(), info=info)


def ransac_essential(points1, points2, K1, K2=None, threshold=1.0, confidence=0.999, max_iters=1000, seed=0, hypotheses=False,
                     device=None):
    """One ``cotr_ransac_essential`` call on the current stream -> dict of device tensors: E float64 [3,3] (the chosen
    five-point candidate at unit Frobenius norm, x2h^T E x1h = 0 on normalised points; no refit), mask bool [n] (its
    inliers), info int32 [8] = (found, best count, iterations run, chosen slot, 0, 0, 0, 0); with hypotheses=True also samples
    int32 [max_iters, 5], hyp_E float64 [10 * max_iters, 9] and hyp_count int32 [10 * max_iters] (the tables tests check).
    K1, K2 [3,3] upper-triangular camera matrices (K2 = K1 when None); threshold in pixels.  Nothing found: E = 0, mask = 0,
    info[0] = 0."""
    p1, p2, n, k1, k2 = _views(points1, points2, K1, K2)
    _check_ransac(k1, k2, threshold, confidence, max_iters)
    device = _args.device(device)
    p1, p2 = on(p1, device), on(p2, device)
    with torch.cuda.device(device):
        out = _enqueue_essential(_lib.load_library(), p1, p2, n, k1, k2, threshold, confidence, max_iters, seed, hypotheses, device)
    out['mask'] = out.pop('mask_u8').bool()
    return out


def find_essential_mat(points1, points2, camera_matrix1, camera_matrix2=None, prob=0.999, threshold=1.0, max_iters=1000, seed=0):
    """``cv2.findEssentialMat(points1, points2, cameraMatrix1, None, cameraMatrix2, None, cv2.RANSAC, prob, threshold)`` by
    the rules of DESIGN.md 3h-3 -> (E float64 [3,3], mask uint8 [n,1]) as cv2 shapes them, or (None, None) when no model is
    found."""
    r = ransac_essential(points1, points2, camera_matrix1, camera_matrix2, threshold, prob, max_iters, seed)
    if not _args.found_flag(r):
        return None, None
    return r['E'].cpu().numpy(), _args.mask_column(r['mask'])


def pose_of_essential(E, points1, points2, K1, K2=None, mask=None, distance_thresh=50.0, device=None):
    """One ``cotr_recover_pose`` call on the current stream -> dict of device tensors: R float64 [3,3], t float64 [3] (unit
    length; x2 ~ R x1 + t), mask bool [n] (``mask`` and in front of both cameras), info int32 [8] = (points in front, chosen
    candidate, the four counts, 0, 0)."""
    p1, p2, n, k1, k2 = _views(points1, points2, K1, K2)
    _args.check_distance(distance_thresh)
    e = _args.flat(E, 'E', 9)
    m = _mask(mask, n)
    device = _args.device(device)
    e, p1, p2, m = on(e, device), on(p1, device), on(p2, device), _args.mask_u8(m, n, device)
    with torch.cuda.device(device):
        return _enqueue_pose(_lib.load_library(), e, p1, p2, n, k1, k2, distance_thresh, m, None, device)


def recover_pose(E, points1, points2, camera_matrix1, camera_matrix2=None, mask=None, distance_thresh=50.0):
    """``cv2.recoverPose(E, points1, points2, cameraMatrix, distanceThresh=50, mask=mask)`` by the rules of DESIGN.md 3h-3
    (with a second camera matrix when the two views differ) -> (n_good, R float64 [3,3], t float64 [3,1], mask uint8 [n,1])
    as cv2 shapes them."""
    r = pose_of_essential(E, points1, points2, camera_matrix1, camera_matrix2, mask, distance_thresh)
    return int(_args.found_flag(r)), r['R'].cpu().numpy(), r['t'].cpu().numpy().reshape(3, 1), _args.mask_column(r['mask'])


MAX_ROUNDS = 8
MAX_REFINE = 64


def _check_refine(rounds, refine_iters, what='rounds'):
    _args.check_int_range(what, rounds, 1, MAX_ROUNDS, integer=False)
    _args.check_int_range('refine_iters', refine_iters, 0, MAX_REFINE, integer=False)


def _enqueue_refine(lib, R, t, p1, p2, n, k1, k2, threshold, distance_thresh, rounds, refine_iters, mask, found, device):
    scratch, nbytes = _args.scratch(lib, 'cotr_refine_pose_scratch_bytes', n, device=device)
    R_out, t_out, E_out, mask_out, info = _args.empty(device, (9, F64), (3, F64), (9, F64), (n, U8), (8, I32))
    check_op(lib.cotr_refine_pose(ptr(R), ptr(t), ptr(p1), ptr(p2), n, k1, k2, float(threshold), float(distance_thresh), int(rounds),
                                  int(refine_iters), ptr(mask), ptr(found), ptr(R_out), ptr(t_out), ptr(E_out), ptr(mask_out), ptr(info),
                                  ptr(scratch), nbytes, _lib.current_stream_ptr()), 'cotr_refine_pose')
    return dict(R=R_out.view(3, 3), t=t_out, E=E_out.view(3, 3), mask=mask_out.bool(), info=info)


def refine_pose_tensors(R, t, points1, points2, K1, K2=None, mask=None, threshold=1.0, distance_thresh=50.0, rounds=4, refine_iters=10,
                        found=None, device=None):
    """One ``cotr_refine_pose`` call on the current stream: the pose (R [3,3], t [3]) refitted on the
    correspondences by undamped Gauss-Newton on the Sampson error over (R, unit t); round 1 fits on ``mask`` (None: every
    point), each later round on the Sampson inliers of the current pose (``threshold`` in pixels) that lie in front of both
    cameras within ``distance_thresh`` -> dict of device tensors: R float64 [3,3], t float64 [3] (unit length), E float64
    [3,3] (= [t]x R at unit Frobenius norm), mask bool [n] (what the last round fitted on), info int32 [8] = (found, points in
    mask, rounds run, steps kept in total, steps kept in the last round, points skipped, 0, 0).  ``found``: a device int32
    tensor whose first entry 0 means there is no pose to refine (every output 0), as do a non-finite pose and t = 0."""
    p1, p2, n, k1, k2 = _views(points1, points2, K1, K2)
    _check_threshold(k1, k2, threshold)
    _args.check_distance(distance_thresh)
    _check_refine(rounds, refine_iters)
    r, tt = _args.flat(R, 'R', 9), _args.flat(t, 't', 3, 'have 3 entries')
    m = _mask(mask, n)
    _args.no_cpu_tensors('the pose refit runs', R, t, points1, points2, mask, found)
    device = _args.device(device)
    r, tt, p1, p2 = on(r, device), on(tt, device), on(p1, device), on(p2, device)
    m, found = _args.mask_u8(m, n, device), _args.found_i32(found, device)
    with torch.cuda.device(device):
        return _enqueue_refine(_lib.load_library(), r, tt, p1, p2, n, k1, k2, threshold, distance_thresh, rounds, refine_iters, m, found, device)


def refine_relative_pose(R, t, points1, points2, K1, K2=None, mask=None, **kw):
    """A relative pose refitted on its correspondences (``refine_pose_tensors``; ``kw``: threshold (1.0), distance_thresh (50),
    rounds (4), refine_iters (10)) -> (R float64 [3,3], t float64 [3,1] of unit length, mask uint8 [n,1]: the points the last
    round fitted on), x2 ~ R x1 + t."""
    r = refine_pose_tensors(R, t, points1, points2, K1, K2, mask, **kw)
    return r['R'].cpu().numpy(), r['t'].cpu().numpy().reshape(3, 1), _args.mask_column(r['mask'])


def relative_pose_tensors(points1, points2, K1, K2=None, threshold=1.0, confidence=0.999, max_iters=1000, seed=0,
                          distance_thresh=50.0, device=None, refine_rounds=0, refine_iters=10):
    """``cotr_ransac_essential`` then ``cotr_recover_pose`` enqueued back to back on the current stream: the second reads the
    first's E, mask and found flag on the device, so no host round trip lies between them -> dict of device tensors: E,
    R, t, mask (the inliers in front of both cameras), info (the RANSAC's), pose_info.  With ``refine_rounds`` > 0
    ``cotr_refine_pose`` follows third in the same sequence, reading R, t, the pose mask and the found flag on the device: R,
    t, E and mask are then the refit's, with refine_info beside them and the unrefined ones as R_ransac, t_ransac, E_ransac,
    mask_ransac."""
    p1, p2, n, k1, k2 = _views(points1, points2, K1, K2)
    _check_ransac(k1, k2, threshold, confidence, max_iters)
    _args.check_distance(distance_thresh)
    if refine_rounds != 0:
        _check_refine(refine_rounds, refine_iters, 'refine_rounds')
    device = _args.device(device)
    p1, p2 = on(p1, device), on(p2, device)
    lib = _lib.load_library()
    with torch.cuda.device(device):
        r = _enqueue_essential(lib, p1, p2, n, k1, k2, threshold, confidence, max_iters, seed, False, device)
        q = _enqueue_pose(lib, r['E'], p1, p2, n, k1, k2, distance_thresh, r['mask_u8'], r['info'], device)
        if refine_rounds != 0:
            f = _enqueue_refine(lib, q['R'], q['t'], p1, p2, n, k1, k2, threshold, distance_thresh, refine_rounds, refine_iters,
                                q['mask'].to(torch.uint8), r['info'], device)
            return dict(E=f['E'], R=f['R'], t=f['t'], mask=f['mask'], info=r['info'], pose_info=q['info'], refine_info=f['info'],
                        E_ransac=r['E'], R_ransac=q['R'], t_ransac=q['t'], mask_ransac=q['mask'])
    return dict(E=r['E'], R=q['R'], t=q['t'], mask=q['mask'], info=r['info'], pose_info=q['info'])


def relative_pose(points1, points2, K1, K2=None, **kw):
    """The relative pose of two calibrated views from their correspondences: ``find_essential_mat`` then ``recover_pose``
    with its mask, as one device sequence -> (R float64 [3,3], t float64 [3,1] of unit length, mask uint8 [n,1]: the
    inliers in front of both cameras), x2 ~ R x1 + t, or (None, None, None) when no model is found.  ``kw``: threshold (1.0),
    confidence (0.999), max_iters (1000), seed (0), distance_thresh (50), refine_rounds (0; above 0: that many rounds of the
    refit of ``refine_pose_tensors`` follow in the same sequence, and the mask is what the last round fitted on),
    refine_iters (10)."""
    r = relative_pose_tensors(points1, points2, K1, K2, **kw)
    if not _args.found_flag(r):
        return None, None, None
    return r['R'].cpu().numpy(), r['t'].cpu().numpy().reshape(3, 1), _args.mask_column(r['mask'])
