"""Robust homography of planar correspondences on the device: RANSAC, then a least-squares refit on the inliers.

``find_homography`` has the signature and defaults of ``cv2.findHomography(src, dst, cv2.RANSAC, ...)``; it is one
``cotr_ransac_homography`` call on the current device and stream (cotr_amd/csrc/homography.hip).  The rules are the
library's own: they follow the structure of OpenCV's estimator - 4-point samples with its degeneracy
check, adaptive iteration count, a refit on the inliers of the best sample, the mask staying the RANSAC mask - with the
F path's counter-based sampler, and claim no bit-compatibility with it.  ``paste_by_homography`` is the robust form of
``paste_by_corners`` (demo_homography.py from any number of correspondences).  No CPU fallback."""
import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args, _ransac

MAX_REFINE = 64


def ransac_homography(points1, points2, threshold=3.0, confidence=0.995, max_iters=2000, seed=0, refine_iters=10, hypotheses=False,
                      device=None):
    """One ``cotr_ransac_homography`` call on the current stream -> dict of device tensors: H float64 [3,3] (the refit on the
    inliers; maps points1 to points2), H_ransac float64 [3,3] (the chosen 4-point candidate), mask bool [n] (its inliers),
    info int32 [8] = (found, best count, iterations run, chosen slot, Gauss-Newton steps kept, refit status: 0 DLT +
    refinement, 1 DLT only, 2 none, 0, 0); with hypotheses=True also samples int32 [max_iters, 4], hyp_H float64
    [max_iters, 9] and hyp_count int32 [max_iters] (the tables tests check).  Nothing found: H = 0, mask = 0, info[0] = 0."""
    p1, p2, n = _ransac.pairs(points1, points2, 4, 'a homography needs at least 4 correspondences')
    _ransac.check_ransac(threshold, confidence, max_iters)
    _args.check_int_range('refine_iters', refine_iters, 0, MAX_REFINE, integer=False)
    device = _args.device(device)
    p1, p2 = on(p1, device), on(p2, device)
    lib = _lib.load_library()
    scratch, H, mask, out = _ransac.outputs(lib, 'cotr_ransac_homography_scratch_bytes', n, max_iters, 4, 1, 8, 'hyp_H', hypotheses, device)
    H_ransac = torch.empty(9, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        check_op(lib.cotr_ransac_homography(ptr(p1), ptr(p2), n, float(threshold), float(confidence), int(max_iters), int(refine_iters),
                                            _ransac.seed64(seed), ptr(H), ptr(mask), ptr(out['info']), ptr(H_ransac),
                                            ptr(out.get('hyp_H')), ptr(out.get('hyp_count')), ptr(out.get('samples')), ptr(scratch),
                                            scratch.numel(), _lib.current_stream_ptr()), 'cotr_ransac_homography')
    out['H'] = H.view(3, 3)
    out['H_ransac'] = H_ransac.view(3, 3)
    out['mask'] = mask.bool()
    return out


def _check_ransac_kw(ransac_reproj_threshold=3.0, max_iters=2000, confidence=0.995, seed=0):
    """``find_homography``'s keywords, checked as ``ransac_homography`` checks them (an unknown one: TypeError)"""
    _ransac.check_ransac(ransac_reproj_threshold, confidence, max_iters)
    int(seed)


def find_homography(src, dst, ransac_reproj_threshold=3.0, max_iters=2000, confidence=0.995, seed=0):
    """``cv2.findHomography(src, dst, cv2.RANSAC, ransac_reproj_threshold, maxIters=max_iters, confidence=confidence)`` by the
    rules of DESIGN.md 3h-2 -> (H float64 [3,3] mapping src to dst, mask uint8 [n,1]) as cv2 shapes them, or (None, None)
    when no model is found."""
    r = ransac_homography(src, dst, ransac_reproj_threshold, confidence, max_iters, seed)
    if not _args.found_flag(r):
        return None, None
    return r['H'].cpu().numpy(), _args.mask_column(r['mask'])


def paste_by_homography(picture, pts_picture, pts_b, img_b, as_tensor=False, **ransac_kw):
    """Paste ``picture`` into ``img_b`` through the homography fitted to any number >= 4 of correspondences: pts_picture
    [N, 2] positions in the picture, pts_b [N, 2] where they land in ``img_b`` (both rounded to float32, as
    ``paste_by_corners`` rounds its corners).  The fit is ``find_homography`` (``ransac_kw``: ransac_reproj_threshold,
    max_iters, confidence, seed); exactly four correspondences determine it: ``get_perspective_transform`` of them on the
    host, with no estimator call (``ransac_kw`` is checked as ``find_homography`` checks it and then has no effect), so the
    picture's four corners give what ``paste_by_corners`` gives.  Then the one ``cotr_warp_perspective`` launch of
    ``paste_by_corners``, ``img_b`` as the background.  No model found: ValueError."""
    from .warp import check_image, get_perspective_transform, warp_perspective
    check_image(picture, 'picture')
    Hb, Wb, _ = check_image(img_b, 'img_b')
    pp = np.asarray(pts_picture.cpu() if torch.is_tensor(pts_picture) else pts_picture)
    pb = np.asarray(pts_b.cpu() if torch.is_tensor(pts_b) else pts_b)
    if pp.ndim != 2 or pp.shape[1] != 2 or pb.shape != pp.shape:
        raise ValueError(f'pts_picture and pts_b must both be [N, 2], got {pp.shape} and {pb.shape}')
    if pp.shape[0] < 4:
        raise ValueError(f'a homography needs at least 4 correspondences, got {pp.shape[0]}')
    pp, pb = pp.astype(np.float32), pb.astype(np.float32)
    if pp.shape[0] == 4:
        _check_ransac_kw(**ransac_kw)
        T = get_perspective_transform(pp, pb)
    else:
        T, _ = find_homography(pp, pb, **ransac_kw)
        if T is None:
            raise ValueError('no homography found for the correspondences')
    return warp_perspective(picture, T, (Wb, Hb), background=img_b, as_tensor=as_tensor)
