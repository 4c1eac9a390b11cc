"""Guided matching of keypoints (demo_guided_matching.py:48-63) on the device.

After its two ``cotr_corr_multiscale`` calls the reference demo matches every predicted position to its nearest keypoint
(scipy ``distance_matrix`` + ``np.argmin``), keeps the mutual pairs with a Python double loop, and prunes them with
``cv2.findFundamentalMat(..., cv2.FM_RANSAC, ...)``.  Here the first two steps are one ``cotr_nearest_mutual`` call and the
third one ``cotr_ransac_fundamental`` call (cotr_amd/csrc/guided.hip; rules in DESIGN.md 3h), on the current device and
stream.  The RANSAC follows the structure of OpenCV 3.4's FM_RANSAC with a counter-based sampler of its own: same
distribution of samples, different draws.  cv2's 7-point LMedS fallback below 15 points is not provided.  No CPU fallback."""
import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args, _ransac


def nearest_mutual(pred_ab, kp_b, pred_ba, kp_a, device=None):
    """idx_ab [Na] (nearest kp_b of every pred_ab row), idx_ba [Nb] (nearest kp_a of every pred_ba row), int32, and the
    mutual flags [Na] bool (idx_ba[idx_ab[i]] == i), as device tensors; one ``cotr_nearest_mutual`` call on the current
    stream.  pred_ab and kp_a are [Na, 2], pred_ba and kp_b [Nb, 2]."""
    pred_ab, kp_b, pred_ba, kp_a = (_args.points(p, w) for p, w in ((pred_ab, 'pred_ab'), (kp_b, 'kp_b'), (pred_ba, 'pred_ba'),
                                                                     (kp_a, 'kp_a')))
    na, nb = kp_a.shape[0], kp_b.shape[0]
    if pred_ab.shape[0] != na or pred_ba.shape[0] != nb:
        raise ValueError(f'pred_ab must have one row per kp_a ({na}) and pred_ba one per kp_b ({nb}), got '
                         f'{pred_ab.shape[0]} and {pred_ba.shape[0]}')
    if na == 0 or nb == 0:
        raise ValueError('nearest keypoints need at least one keypoint on each side')
    device = _args.device(device)
    pred_ab, kp_b, pred_ba, kp_a = (on(t, device) for t in (pred_ab, kp_b, pred_ba, kp_a))
    lib = _lib.load_library()
    scratch, nbytes = _args.scratch(lib, 'cotr_nearest_mutual_scratch_bytes', na, nb, device=device)
    idx_ab, idx_ba, mutual = _args.empty(device, (na, _args.I32), (nb, _args.I32), (na, _args.U8))
    with torch.cuda.device(device):
        check_op(lib.cotr_nearest_mutual(ptr(pred_ab), ptr(kp_b), ptr(pred_ba), ptr(kp_a), na, nb, ptr(idx_ab), ptr(idx_ba),
                                         ptr(mutual), ptr(scratch), nbytes, _lib.current_stream_ptr()), 'cotr_nearest_mutual')
    return idx_ab, idx_ba, mutual.bool()


def mutual_matches(corrs_a_b, corrs_b_a, kp_a, kp_b):
    """``final_matches`` of demo_guided_matching.py:48-62: int64 [K, 2] rows (i, j) with kp_b[j] the nearest keypoint of
    corrs_a_b[i, 2:] and kp_a[i] the nearest of corrs_b_a[j, 2:], in the double loop's order (ascending i).
    corrs_a_b [Na, 4] and corrs_b_a [Nb, 4] are ``cotr_corr_multiscale`` results, one row per keypoint."""
    corrs_a_b, corrs_b_a = np.asarray(corrs_a_b), np.asarray(corrs_b_a)
    for name, c in (('corrs_a_b', corrs_a_b), ('corrs_b_a', corrs_b_a)):
        if c.ndim != 2 or c.shape[1] != 4:
            raise ValueError(f'{name} must be [N, 4] (x_a, y_a, x_b, y_b), got shape {c.shape}')
    idx_ab, _, mutual = nearest_mutual(corrs_a_b[:, 2:], kp_b, corrs_b_a[:, 2:], kp_a)
    i = torch.nonzero(mutual).flatten()
    return torch.stack([i, idx_ab[i].long()], dim=1).cpu().numpy().astype(np.int64).reshape(-1, 2)


def ransac_fundamental(points1, points2, threshold=3.0, confidence=0.99, max_iters=1000, seed=0, hypotheses=False, device=None):
    """One ``cotr_ransac_fundamental`` call on the current stream -> dict of device tensors: F float64 [3,3], mask bool [n],
    info int32 [4] = (found, best count, iterations run, chosen slot); with hypotheses=True also samples int32
    [max_iters, 7], hyp_F float64 [3*max_iters, 9] and hyp_count int32 [3*max_iters] (the tables tests check)."""
    p1, p2, n = _ransac.pairs(points1, points2, 15, 'find_fundamental_mat needs at least 15 correspondences for RANSAC '
                              '(cv2\'s 7-point / LMedS fallback below 15 points is not provided)')
    _ransac.check_ransac(threshold, confidence, max_iters)
    device = _args.device(device)
    p1, p2 = on(p1, device), on(p2, device)
    lib = _lib.load_library()
    scratch, F, mask, out = _ransac.outputs(lib, 'cotr_ransac_fundamental_scratch_bytes', n, max_iters, 7, 3, 4, 'hyp_F', hypotheses, device)
    with torch.cuda.device(device):
        check_op(lib.cotr_ransac_fundamental(ptr(p1), ptr(p2), n, float(threshold), float(confidence), int(max_iters),
                                             _ransac.seed64(seed), ptr(F), ptr(mask), ptr(out['info']), ptr(out.get('hyp_F')),
                                             ptr(out.get('hyp_count')), ptr(out.get('samples')), ptr(scratch), scratch.numel(),
                                             _lib.current_stream_ptr()), 'cotr_ransac_fundamental')
    out['F'] = F.view(3, 3)
    out['mask'] = mask.bool()
    return out


def find_fundamental_mat(points1, points2, ransac_reproj_threshold=3.0, confidence=0.99, max_iters=1000, seed=0):
    """``cv2.findFundamentalMat(points1, points2, cv2.FM_RANSAC, ransac_reproj_threshold, confidence, max_iters)`` by the
    rule of DESIGN.md 3h -> (F float64 [3,3], mask uint8 [n,1]) as cv2 shapes them, or (None, None) when no model is
    found.  Fewer than 15 points: ValueError (cv2 would switch to its 7-point / LMedS fallback, not provided here)."""
    r = ransac_fundamental(points1, points2, ransac_reproj_threshold, confidence, max_iters, seed)
    if not _args.found_flag(r):
        return None, None
    return r['F'].cpu().numpy(), _args.mask_column(r['mask'])


def filter_guided_matches(corrs_a_b, corrs_b_a, kp_a, kp_b, ransac_threshold=5.0, confidence=0.999999, seed=0):
    """demo_guided_matching.py:48-65 after the two ``cotr_corr_multiscale`` calls: mutual nearest keypoints, then the
    fundamental-matrix RANSAC -> ``final_corrs[np.where(mask[:, 0])]``, rows concat(kp_a[i], kp_b[j]) (numpy's dtype
    promotion of the two keypoint arrays).  Fewer than 15 mutual matches: ValueError, as from find_fundamental_mat."""
    kp_a, kp_b = np.asarray(kp_a), np.asarray(kp_b)
    final_matches = mutual_matches(corrs_a_b, corrs_b_a, kp_a, kp_b)
    final_corrs = np.concatenate([kp_a[final_matches[:, 0]], kp_b[final_matches[:, 1]]], axis=1)
    _, mask = find_fundamental_mat(final_corrs[:, :2], final_corrs[:, 2:], ransac_threshold, confidence, seed=seed)
    if mask is None:
        return final_corrs[:0]
    return final_corrs[np.where(mask[:, 0])]
