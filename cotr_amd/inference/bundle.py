"""Bundle adjustment on the device: the poses of 2 to 32 views and the points they see, refined together.

``bundle_adjust_tensors`` is one ``cotr_bundle_adjust`` call (cotr_amd/csrc/bundle.hip, rules in DESIGN.md 3h-7) on the current
device and stream: Levenberg-Marquardt on the summed squared pixel error, the points eliminated by the Schur complement, the
observation set re-selected between rounds.  It follows ``triangulate_views`` (its ``X`` and ``used`` are the natural ``X`` and
``visible`` here) as one more call of the same device sequence; ``bundle_adjust`` is the same with host arrays back.  No CPU
fallback."""
import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args
from ._args import F64, I32, U8

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
    _args.check_positive('threshold', threshold)
    _args.check_sq_float32(threshold)
    _args.check_distance(distance_thresh)
    _args.check_int_range('rounds', rounds, 1, MAX_ROUNDS)
    _args.check_int_range('iters', iters, 0, MAX_ITERS)
    if not 1e-12 <= lambda0 <= 1e12:
        raise ValueError(f'lambda0 must be in [1e-12, 1e12], got {lambda0}')


def _enqueue(lib, pts, vis, cams, rows, X, fixed, V, N, found, threshold, distance_thresh, rounds, iters, lambda0, device):
    scratch, nbytes = _args.scratch(lib, 'cotr_bundle_adjust_scratch_bytes', V, N, device=device)
    poses, Xo, used, stats, info = _args.empty(device, ((V, 12), F64), ((N, 3), F64), ((V, N), U8), (4, F64), (8, I32))
    check_op(lib.cotr_bundle_adjust(ptr(pts), ptr(vis), ptr(cams), ptr(rows), ptr(X), fixed.ctypes.data, V, N, ptr(found), float(threshold),
                                    float(distance_thresh), int(rounds), int(iters), float(lambda0), ptr(poses), ptr(Xo), ptr(used),
                                    ptr(stats), ptr(info), ptr(scratch), nbytes, _lib.current_stream_ptr()), 'cotr_bundle_adjust')
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
    pts, V, N = _args.view_points(points)
    if N > MAX_POINTS:
        raise ValueError(f'between 1 and 2^20 points, got {N}')
    cams, rows = _args.cam_rows(cameras, V), _args.pose_rows(poses, V)
    Xt = _args.tensor(X).to(dtype=torch.float64)
    if tuple(Xt.shape) != (N, 3):
        raise ValueError(f'X must be [N, 3] = [{N}, 3], got shape {tuple(Xt.shape)}')
    vis = _args.visible(visible, V, N)
    fixed = _fixed(fixed_views, V)
    _check(threshold, distance_thresh, rounds, iters, lambda0)
    _args.no_cpu_tensors('the triangulation runs', points, cameras, poses, X, visible, found)   # (the wording of structure.py, whose call this follows)
    device = _args.device(device)
    pts, cams, rows, Xt = on(pts, device, 16), on(cams, device), on(rows, device), on(Xt, device)
    vis, found = _args.mask_u8(vis, (V, N), device), _args.found_i32(found, device)
    with torch.cuda.device(device):
        return _enqueue(_lib.load_library(), pts, vis, cams, rows, Xt, fixed, V, N, found, threshold, distance_thresh, rounds, iters, lambda0,
                        device)


def bundle_adjust(points, cameras, poses, X, **kw):
    """``bundle_adjust_tensors`` with host arrays back -> dict(poses [V,3,4], X [N,3], used uint8 [V,N], stats [4], info [8])."""
    r = bundle_adjust_tensors(points, cameras, poses, X, **kw)
    out = {k: v.cpu().numpy() for k, v in r.items()}
    out['used'] = out['used'].astype(np.uint8)
    return out
