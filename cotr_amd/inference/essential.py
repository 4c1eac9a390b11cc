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
import ctypes

import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _ransac
from ._ransac import _device

MAX_ITERS = 6553
_K9 = ctypes.c_double * 9


def _camera(K, what):
    """[3,3] upper-triangular camera matrix -> 9 host doubles; finite, focal lengths not 0"""
    k = np.asarray(K.cpu() if torch.is_tensor(K) else K, dtype=np.float64)
    if k.shape != (3, 3):
        raise ValueError(f'{what} must be [3, 3], got shape {k.shape}')
    if not np.isfinite(k[[0, 0, 0, 1, 1], [0, 1, 2, 1, 2]]).all() or k[0, 0] == 0 or k[1, 1] == 0:
        raise ValueError(f'{what} must be finite with focal lengths that are not 0')
    return _K9(*k.reshape(9))


def _pairs(points1, points2):
    return _ransac.pairs(points1, points2, 5, 'an essential matrix needs at least 5 correspondences')


def _check_ransac(K1, K2, threshold, confidence, max_iters):
    _ransac.check_ransac(threshold, confidence, max_iters, MAX_ITERS)
    _check_threshold(K1, K2, threshold)


def _check_threshold(K1, K2, threshold):
    if not (threshold > 0 and np.isfinite(threshold)):
        raise ValueError(f'the RANSAC threshold must be finite and > 0, got {threshold}')
    thr = threshold / ((K1[0] + K1[4] + K2[0] + K2[4]) / 4.0) if (K1[0] + K1[4] + K2[0] + K2[4]) != 0 else np.inf
    if not (thr * thr > 0 and np.isfinite(thr * thr)):
        raise ValueError('the RANSAC threshold over the mean focal length must be finite and not 0')


def _enqueue_essential(lib, p1, p2, n, k1, k2, threshold, confidence, max_iters, seed, hypotheses, device):
    scratch, E, mask, out = _ransac.outputs(lib.cotr_ransac_essential_scratch_bytes, 'cotr_ransac_essential_scratch_bytes', n,
                                            max_iters, 5, 10, 8, 'hyp_E', hypotheses, device)
    check_op(lib.cotr_ransac_essential(ptr(p1), ptr(p2), n, k1, k2, float(threshold), float(confidence), int(max_iters),
                                       _ransac.seed64(seed), ptr(E), ptr(mask), ptr(out['info']), ptr(out.get('hyp_E')),
                                       ptr(out.get('hyp_count')), ptr(out.get('samples')), ptr(scratch), scratch.numel(),
                                       _lib.current_stream_ptr()), 'cotr_ransac_essential')
    out['E'] = E.view(3, 3)
    out['mask_u8'] = mask
    return out


def _enqueue_pose(lib, E, p1, p2, n, k1, k2, distance_thresh, mask, found, device):
    nbytes = ctypes.c_size_t()
    check_op(lib.cotr_recover_pose_scratch_bytes(n, ctypes.byref(nbytes)), 'cotr_recover_pose_scratch_bytes')
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
    R = torch.empty(9, dtype=torch.float64, device=device)
    t = torch.empty(3, dtype=torch.float64, device=device)
    mask_out = torch.empty(n, dtype=torch.uint8, device=device)
    info = torch.empty(8, dtype=torch.int32, device=device)
    check_op(lib.cotr_recover_pose(ptr(E), ptr(p1), ptr(p2), n, k1, k2, float(distance_thresh), ptr(mask), ptr(found), ptr(R), ptr(t),
                                   ptr(mask_out), ptr(info), ptr(scratch), nbytes.value, _lib.current_stream_ptr()), 'cotr_recover_pose')
    return dict(R=R.view(3, 3), t=t, mask=mask_out.bool(), info=info)


def ransac_essential(points1, points2, K1, K2=None, threshold=1.0, confidence=0.999, max_iters=1000, seed=0, hypotheses=False,
                     device=None):
    """One ``cotr_ransac_essential`` call on the current stream -> dict of device tensors: E float64 [3,3] (the chosen
    five-point candidate at unit Frobenius norm, x2h^T E x1h = 0 on normalised points; no refit), mask bool [n] (its
    inliers), info int32 [8] = (found, best count, iterations run, chosen slot, 0, 0, 0, 0); with hypotheses=True also samples
    int32 [max_iters, 5], hyp_E float64 [10 * max_iters, 9] and hyp_count int32 [10 * max_iters] (the tables tests check).
    K1, K2 [3,3] upper-triangular camera matrices (K2 = K1 when None); threshold in pixels.  Nothing found: E = 0, mask = 0,
    info[0] = 0."""
    p1, p2, n = _pairs(points1, points2)
    k1 = _camera(K1, 'K1')
    k2 = k1 if K2 is None else _camera(K2, 'K2')
    _check_ransac(k1, k2, threshold, confidence, max_iters)
    device = _device(device)
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
    if not r['info'].cpu().numpy()[0]:
        return None, None
    return r['E'].cpu().numpy(), r['mask'].cpu().numpy().astype(np.uint8).reshape(-1, 1)


def _check_distance(distance_thresh):
    if not (distance_thresh > 0 and np.isfinite(distance_thresh)):
        raise ValueError(f'distance_thresh must be finite and > 0, got {distance_thresh}')


def pose_of_essential(E, points1, points2, K1, K2=None, mask=None, distance_thresh=50.0, device=None):
    """One ``cotr_recover_pose`` call on the current stream -> dict of device tensors: R float64 [3,3], t float64 [3] (unit
    length; x2 ~ R x1 + t), mask bool [n] (``mask`` and in front of both cameras), info int32 [8] = (points in front, chosen
    candidate, the four counts, 0, 0)."""
    p1, p2, n = _pairs(points1, points2)
    k1 = _camera(K1, 'K1')
    k2 = k1 if K2 is None else _camera(K2, 'K2')
    _check_distance(distance_thresh)
    e = E if torch.is_tensor(E) else torch.from_numpy(np.ascontiguousarray(np.asarray(E, dtype=np.float64)))
    if e.numel() != 9:
        raise ValueError(f'E must be [3, 3], got shape {tuple(e.shape)}')
    m = None
    if mask is not None:
        m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask)))
        if m.numel() != n:
            raise ValueError(f'mask must have one entry per correspondence, got {m.numel()} for {n}')
    device = _device(device)
    e = on(e.to(dtype=torch.float64).reshape(9), device)
    p1, p2 = on(p1, device), on(p2, device)
    if m is not None:
        m = (on(m, device).reshape(n) != 0).to(torch.uint8)
    with torch.cuda.device(device):
        return _enqueue_pose(_lib.load_library(), e, p1, p2, n, k1, k2, distance_thresh, m, None, device)


def recover_pose(E, points1, points2, camera_matrix1, camera_matrix2=None, mask=None, distance_thresh=50.0):
    """``cv2.recoverPose(E, points1, points2, cameraMatrix, distanceThresh=50, mask=mask)`` by the rules of DESIGN.md 3h-3
    (with a second camera matrix when the two views differ) -> (n_good, R float64 [3,3], t float64 [3,1], mask uint8 [n,1])
    as cv2 shapes them."""
    r = pose_of_essential(E, points1, points2, camera_matrix1, camera_matrix2, mask, distance_thresh)
    info = r['info'].cpu().numpy()
    return int(info[0]), r['R'].cpu().numpy(), r['t'].cpu().numpy().reshape(3, 1), r['mask'].cpu().numpy().astype(np.uint8).reshape(-1, 1)


MAX_ROUNDS = 8
MAX_REFINE = 64


def _no_cpu_tensors(*xs):
    if any(torch.is_tensor(x) and not x.is_cuda for x in xs):
        raise _lib.CotrHipError('the pose refit runs on an MI355X only (HIP kernels, no CPU fallback): got a CPU tensor; '
                                'pass a numpy array or move the tensor with .cuda()')


def _check_refine(rounds, refine_iters, what='rounds'):
    if not 1 <= rounds <= MAX_ROUNDS:
        raise ValueError(f'{what} must be in [1, {MAX_ROUNDS}], got {rounds}')
    if not 0 <= refine_iters <= MAX_REFINE:
        raise ValueError(f'refine_iters must be in [0, {MAX_REFINE}], got {refine_iters}')


def _enqueue_refine(lib, R, t, p1, p2, n, k1, k2, threshold, distance_thresh, rounds, refine_iters, mask, found, device):
    nbytes = ctypes.c_size_t()
    check_op(lib.cotr_refine_pose_scratch_bytes(n, ctypes.byref(nbytes)), 'cotr_refine_pose_scratch_bytes')
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
    R_out = torch.empty(9, dtype=torch.float64, device=device)
    t_out = torch.empty(3, dtype=torch.float64, device=device)
    E_out = torch.empty(9, dtype=torch.float64, device=device)
    mask_out = torch.empty(n, dtype=torch.uint8, device=device)
    info = torch.empty(8, dtype=torch.int32, device=device)
    check_op(lib.cotr_refine_pose(ptr(R), ptr(t), ptr(p1), ptr(p2), n, k1, k2, float(threshold), float(distance_thresh), int(rounds),
                                  int(refine_iters), ptr(mask), ptr(found), ptr(R_out), ptr(t_out), ptr(E_out), ptr(mask_out), ptr(info),
                                  ptr(scratch), nbytes.value, _lib.current_stream_ptr()), 'cotr_refine_pose')
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
    p1, p2, n = _pairs(points1, points2)
    k1 = _camera(K1, 'K1')
    k2 = k1 if K2 is None else _camera(K2, 'K2')
    _check_threshold(k1, k2, threshold)
    _check_distance(distance_thresh)
    _check_refine(rounds, refine_iters)
    r = R if torch.is_tensor(R) else torch.from_numpy(np.ascontiguousarray(np.asarray(R, dtype=np.float64)))
    tt = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float64)))
    if r.numel() != 9:
        raise ValueError(f'R must be [3, 3], got shape {tuple(r.shape)}')
    if tt.numel() != 3:
        raise ValueError(f't must have 3 entries, got shape {tuple(tt.shape)}')
    m = None
    if mask is not None:
        m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask)))
        if m.numel() != n:
            raise ValueError(f'mask must have one entry per correspondence, got {m.numel()} for {n}')
    _no_cpu_tensors(R, t, points1, points2, mask, found)
    device = _device(device)
    r, tt = on(r.to(dtype=torch.float64).reshape(9), device), on(tt.to(dtype=torch.float64).reshape(3), device)
    p1, p2 = on(p1, device), on(p2, device)
    if m is not None:
        m = (on(m, device).reshape(n) != 0).to(torch.uint8)
    if found is not None:
        found = on(found, device).to(torch.int32).reshape(-1)
    with torch.cuda.device(device):
        return _enqueue_refine(_lib.load_library(), r, tt, p1, p2, n, k1, k2, threshold, distance_thresh, rounds, refine_iters, m, found, device)


def refine_relative_pose(R, t, points1, points2, K1, K2=None, mask=None, **kw):
    """A relative pose refitted on its correspondences (``refine_pose_tensors``; ``kw``: threshold (1.0), distance_thresh (50),
    rounds (4), refine_iters (10)) -> (R float64 [3,3], t float64 [3,1] of unit length, mask uint8 [n,1]: the points the last
    round fitted on), x2 ~ R x1 + t."""
    r = refine_pose_tensors(R, t, points1, points2, K1, K2, mask, **kw)
    return r['R'].cpu().numpy(), r['t'].cpu().numpy().reshape(3, 1), r['mask'].cpu().numpy().astype(np.uint8).reshape(-1, 1)


def relative_pose_tensors(points1, points2, K1, K2=None, threshold=1.0, confidence=0.999, max_iters=1000, seed=0,
                          distance_thresh=50.0, device=None, refine_rounds=0, refine_iters=10):
    """``cotr_ransac_essential`` then ``cotr_recover_pose`` enqueued back to back on the current stream: the second reads the
    first's E, mask and found flag on the device, so no host round trip lies between them -> dict of device tensors: E,
    R, t, mask (the inliers in front of both cameras), info (the RANSAC's), pose_info.  With ``refine_rounds`` > 0
    ``cotr_refine_pose`` follows third in the same sequence, reading R, t, the pose mask and the found flag on the device: R,
    t, E and mask are then the refit's, with refine_info beside them and the unrefined ones as R_ransac, t_ransac, E_ransac,
    mask_ransac."""
    p1, p2, n = _pairs(points1, points2)
    k1 = _camera(K1, 'K1')
    k2 = k1 if K2 is None else _camera(K2, 'K2')
    _check_ransac(k1, k2, threshold, confidence, max_iters)
    _check_distance(distance_thresh)
    if refine_rounds != 0:
        _check_refine(refine_rounds, refine_iters, 'refine_rounds')
    device = _device(device)
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
    if not r['info'].cpu().numpy()[0]:
        return None, None, None
    return r['R'].cpu().numpy(), r['t'].cpu().numpy().reshape(3, 1), r['mask'].cpu().numpy().astype(np.uint8).reshape(-1, 1)
