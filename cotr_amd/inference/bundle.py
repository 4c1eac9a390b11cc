"""Bundle adjustment on the device: the poses of 2 to 32 views and the points they see, refined together.

``bundle_adjust_tensors`` is one ``cotr_bundle_adjust`` call (cotr_amd/csrc/bundle.hip, rules in DESIGN.md 3h-7) on the current
device and stream: Levenberg-Marquardt on the summed squared pixel error, the points eliminated by the Schur complement, the
observation set re-selected between rounds.  It follows ``triangulate_views`` (its ``X`` and ``used`` are the natural ``X`` and
``visible`` here) as one more call of the same device sequence; ``bundle_adjust`` is the same with host arrays back.  No CPU
fallback."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from ._ransac import _device
from .essential import _check_distance
from .structure import _cam_rows, _no_cpu_tensors, _pose_rows, _tensor, _view_points

MAX_POINTS = 1 << 20
MAX_ROUNDS = 8
MAX_ITERS = 64


def _fixed(fixed_views, V):
    """indices of the views whose pose is held, or a [V] mask -> uint8 [V] host array"""
    f = np.asarray(fixed_views.cpu() if torch.is_tensor(fixed_views) else fixed_views)
    if f.dtype == bool:
        if f.shape != (V,):
            raise ValueError(f'a fixed_views mask must be [V] = [{V}], got shape {f.shape}')
        m = f.astype(np.uint8)
    else:
        idx = f.astype(np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= V):
            raise ValueError(f'fixed_views must name views in [0, {V}), got {list(idx)}')
        m = np.zeros(V, np.uint8)
        m[idx] = 1
    if not m.any():
        raise ValueError('at least one view must be fixed')
    if m.all():
        raise ValueError('at least one view must not be fixed')
    return np.ascontiguousarray(m)


def _check(threshold, distance_thresh, rounds, iters, lambda0):
    if not (threshold > 0 and np.isfinite(threshold)):
        raise ValueError(f'threshold must be finite and > 0, got {threshold}')
    with np.errstate(over='ignore', under='ignore'):
        sq = np.float32(float(threshold) * float(threshold))
    if not (sq > 0 and np.isfinite(sq)):
        raise ValueError(f'the squared threshold must be a finite float32 that is not 0, got threshold {threshold}')
    _check_distance(distance_thresh)
    if int(rounds) != rounds or not 1 <= int(rounds) <= MAX_ROUNDS:
        raise ValueError(f'rounds must be an integer in [1, {MAX_ROUNDS}], got {rounds}')
    if int(iters) != iters or not 0 <= int(iters) <= MAX_ITERS:
        raise ValueError(f'iters must be an integer in [0, {MAX_ITERS}], got {iters}')
    if not 1e-12 <= lambda0 <= 1e12:
        raise ValueError(f'lambda0 must be in [1e-12, 1e12], got {lambda0}')


def _enqueue(lib, pts, vis, cams, rows, X, fixed, V, N, found, threshold, distance_thresh, rounds, iters, lambda0, device):
    nbytes = ctypes.c_size_t()
    check_op(lib.cotr_bundle_adjust_scratch_bytes(V, N, ctypes.byref(nbytes)), 'cotr_bundle_adjust_scratch_bytes')
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
    poses = torch.empty((V, 12), dtype=torch.float64, device=device)
    Xo = torch.empty((N, 3), dtype=torch.float64, device=device)
    used = torch.empty((V, N), dtype=torch.uint8, device=device)
    stats = torch.empty(4, dtype=torch.float64, device=device)
    info = torch.empty(8, dtype=torch.int32, device=device)
    check_op(lib.cotr_bundle_adjust(ptr(pts), ptr(vis), ptr(cams), ptr(rows), ptr(X), fixed.ctypes.data, V, N, ptr(found), float(threshold),
                                    float(distance_thresh), int(rounds), int(iters), float(lambda0), ptr(poses), ptr(Xo), ptr(used),
                                    ptr(stats), ptr(info), ptr(scratch), nbytes.value, _lib.current_stream_ptr()), 'cotr_bundle_adjust')
    return dict(poses=poses.reshape(V, 3, 4), X=Xo, used=used.bool(), stats=stats, info=info)


def bundle_adjust_tensors(points, cameras, poses, X, visible=None, fixed_views=(0,), threshold=4.0, distance_thresh=50.0, rounds=1,
                          iters=10, lambda0=1e-3, found=None, device=None):
    """One ``cotr_bundle_adjust`` call on the current stream: points [V,N,2], cameras and poses as for
    ``triangulate_views`` (the poses to start from), X [N,3] the points to start from, visible [V,N] the observations to
    trust (None: every view sees every point; ``used`` of ``triangulate_views`` is the natural choice), fixed_views the
    indices (or a bool [V] mask) of the views whose pose is held -> dict of device tensors: poses float64 [V,3,4], X float64
    [N,3] (a view or a point that never moved carries its input bit for bit), used bool [V,N] (the observations of the last
    round), stats float64 [4] = (cost of round 1's observations at the input, cost of the last round's at the output, the
    last damping, 0), info int32 [8] = (found, observations in the last round, views optimised, views frozen (fewer than 4
    observations), landmarks (points with fewer than 2), steps kept, steps rejected, rounds run).  Round 1 takes the visible
    observations in front of their camera; each later round re-selects those within ``threshold`` px and ``distance_thresh``
    at the current state.  ``iters`` Levenberg-Marquardt iterations per round from damping ``lambda0``.  The intrinsics are
    not optimised.  ``found``: a device int32 tensor whose first entry 0 zeroes every output."""
    pts, V, N = _view_points(points)
    if N > MAX_POINTS:
        raise ValueError(f'between 1 and 2^20 points, got {N}')
    cams = _cam_rows(cameras, V)
    rows = _pose_rows(poses, V)
    Xt = _tensor(X).to(dtype=torch.float64)
    if tuple(Xt.shape) != (N, 3):
        raise ValueError(f'X must be [N, 3] = [{N}, 3], got shape {tuple(Xt.shape)}')
    vis = None
    if visible is not None:
        vis = _tensor(visible, None)
        if tuple(vis.shape) != (V, N):
            raise ValueError(f'visible must be [V, N] = [{V}, {N}], got shape {tuple(vis.shape)}')
    fixed = _fixed(fixed_views, V)
    _check(threshold, distance_thresh, rounds, iters, lambda0)
    _no_cpu_tensors(points, cameras, poses, X, visible, found)
    device = _device(device)
    pts, cams, rows, Xt = on(pts, device, 16), on(cams, device), on(rows, device), on(Xt, device)
    if vis is not None:
        vis = (on(vis, device) != 0).to(torch.uint8)
    if found is not None:
        found = on(found, device).to(torch.int32).reshape(-1)
    with torch.cuda.device(device):
        return _enqueue(_lib.load_library(), pts, vis, cams, rows, Xt, fixed, V, N, found, threshold, distance_thresh, rounds, iters, lambda0,
                        device)


def bundle_adjust(points, cameras, poses, X, **kw):
    """``bundle_adjust_tensors`` with host arrays back -> dict(poses [V,3,4], X [N,3], used uint8 [V,N], stats [4], info [8])."""
    r = bundle_adjust_tensors(points, cameras, poses, X, **kw)
    out = {k: v.cpu().numpy() for k, v in r.items()}
    out['used'] = out['used'].astype(np.uint8)
    return out
