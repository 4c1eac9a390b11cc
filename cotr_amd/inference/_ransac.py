"""What the wrappers of the RANSAC estimators share (guided.py, homography.py, essential.py): the point and argument
checks and the allocation of a call's outputs.  The messages keep one wording for all three."""
import ctypes

import numpy as np
import torch

from .._lib import check_op

MAX_POINTS = 1 << 24
MAX_ITERS = 1 << 16


def _device(device):
    return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


def _points(p, what):
    """[N,2] float64 tensor, where it was (float32 input is widened exactly)"""
    t = p if torch.is_tensor(p) else torch.from_numpy(np.ascontiguousarray(np.asarray(p, dtype=np.float64)))
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError(f'{what} must be [N, 2], got shape {tuple(t.shape)}')
    return t.to(dtype=torch.float64)


def pairs(points1, points2, least, too_few):
    """-> (points1, points2, n) as [n, 2] float64 tensors; ``too_few``: the message below ``least`` correspondences, the
    model's own"""
    p1, p2 = _points(points1, 'points1'), _points(points2, 'points2')
    n = p1.shape[0]
    if p2.shape[0] != n:
        raise ValueError(f'points1 and points2 must have the same length, got {n} and {p2.shape[0]}')
    if n < least:
        raise ValueError(f'{too_few}, got {n}')
    if n > MAX_POINTS:
        raise ValueError(f'at most 2^24 correspondences, got {n}')
    return p1, p2, n


def check_ransac(threshold, confidence, max_iters, most_iters=MAX_ITERS):
    if not 1 <= max_iters <= most_iters:
        raise ValueError(f'max_iters must be in [1, {most_iters}], got {max_iters}')
    if not (threshold > 0 and np.isfinite(threshold)):
        raise ValueError(f'the RANSAC threshold must be finite and > 0, got {threshold}')
    if not 0 < confidence < 1:
        raise ValueError(f'confidence must be in (0, 1), got {confidence}')


def seed64(seed):
    return int(seed) & ((1 << 64) - 1)


def outputs(scratch_bytes, what, n, max_iters, model, slots, info_len, hyp_key, hypotheses, device):
    """the tensors of one estimator call -> (scratch uint8, result float64 [9], mask uint8 [n], dict(info int32 [info_len]) with,
    when ``hypotheses``, samples int32 [max_iters, model], ``hyp_key`` float64 [slots * max_iters, 9] and hyp_count int32
    [slots * max_iters]).  scratch_bytes: the library's ``*_scratch_bytes`` function, ``what`` its name."""
    nbytes = ctypes.c_size_t()
    check_op(scratch_bytes(n, max_iters, ctypes.byref(nbytes)), what)
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
    result = torch.empty(9, dtype=torch.float64, device=device)
    mask = torch.empty(n, dtype=torch.uint8, device=device)
    out = dict(info=torch.empty(info_len, dtype=torch.int32, device=device))
    if hypotheses:
        out['samples'] = torch.empty((max_iters, model), dtype=torch.int32, device=device)
        out[hyp_key] = torch.empty((slots * max_iters, 9), dtype=torch.float64, device=device)
        out['hyp_count'] = torch.empty(slots * max_iters, dtype=torch.int32, device=device)
    return scratch, result, mask, out
