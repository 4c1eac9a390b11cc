"""The poses of 2 to 32 views from pairwise results, on the device: the global step between ``relative_pose_tensors`` and
``bundle_adjust``.

``average_rotations`` is one ``cotr_average_rotations`` call (cotr_amd/csrc/global_pose.hip, rules in DESIGN.md 3h-19) on the
current device and stream: the absolute rotations of the views from relative ones over a graph of view pairs, started on a
greedy tree and refined by annealed robust Gauss-Newton steps, with every edge's residual and inlier flag.
``solve_positions`` is one ``cotr_solve_positions`` call: the camera centres and the points from the tracks with the rotations
known, a linear problem whose points are eliminated by the Schur complement and whose solution is the eigenvector of the
smallest eigenvalue of the reduced matrix.  ``*_host`` are the same with host arrays back.
``structure.reconstruct_views_tensors`` chains them between the two-view poses and the bundle adjustment.  No CPU fallback."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args
from ._args import F64, I32, MAX_VIEWS, U8

MAX_POINTS = 1 << 20
MAX_ITERS = 64
MAX_ROUNDS = 8
MAX_POWER = 64
DEG = np.pi / 180.0
STOP_REASONS = ('ran all', 'no view to solve for', 'singular')
_SUBJECT = 'the global poses run'


def _check_rotations(n, E, root, iters, sigma0, sigma_end, edge_thresh):
    _args.check_int_range('n', n, 2, MAX_VIEWS)
    if not 1 <= E <= n * (n - 1):
        raise ValueError(f'between 1 and n (n - 1) = {n * (n - 1)} edges, got {E}')
    _args.check_int_range('root', root, 0, n - 1)
    _args.check_int_range('iters', iters, 0, MAX_ITERS)
    _args.check_positive('sigma_end', sigma_end)
    _args.check_positive('sigma0', sigma0)
    if sigma0 < sigma_end:
        raise ValueError(f'sigma0 must not be below sigma_end, got {sigma0} and {sigma_end}')
    _args.check_positive('edge_thresh', edge_thresh)


def _enqueue_rotations(lib, R_rel, edges, weights, found, n, E, root, iters, sigma0, sigma_end, edge_thresh, device):
    """every tensor on ``device`` already, every argument checked -> the dict of ``average_rotations``"""
    R, edge, view_info, info, stats = _args.empty(device, ((n, 3, 3), F64), ((E, 4), F64), ((n, 4), I32), (8, I32), (2, F64))
    check_op(lib.cotr_average_rotations(ptr(R_rel), ptr(edges), ptr(weights), ptr(found), n, E, int(root), int(iters), float(sigma0),
                                        float(sigma_end), float(edge_thresh), ptr(R), ptr(edge), ptr(view_info), ptr(info), ptr(stats),
                                        _lib.current_stream_ptr()), 'cotr_average_rotations')
    return dict(R=R, edge=edge, live=edge[:, 2] != 0, inlier=edge[:, 3] != 0, view_info=view_info, located=view_info[:, 0].contiguous(),
                info=info, stats=stats)


def average_rotations(R_rel, edges, n, weights=None, found=None, root=0, iters=12, sigma0=32 * DEG, sigma_end=1 * DEG, edge_thresh=3 * DEG,
                      device=None):
    """One ``cotr_average_rotations`` call on the current stream: R_rel [E,3,3] float64, edges [E,2] int =
    (i, j) with x_j ~ R_ij x_i + t_ij (what ``relative_pose_tensors`` returns with i as view 1), so R_j = R_ij R_i; weights [E]
    (None: 1; inlier counts are the natural weight), found [E] int (0: the edge is dead, as is one with a bad index, i = j, a
    weight that is not positive and finite or a matrix that is not finite) -> dict of device tensors: R float64 [n,3,3]
    (world-to-camera, R[root] = I, NaN for a view no live edge reaches), edge float64 [E,4] = (|r_e| at the output in radians,
    the last robust weight, live, inlier), live and inlier bool [E], view_info int32 [n,4] = (located, the round of the greedy
    tree it was located in, live edges, inlier edges), located int32 [n], info int32 [8] = (ok, located views, live edges,
    inlier edges, steps taken, stop reason (an index of STOP_REASONS), 0, 0), stats float64 [2] = (sum w r^2, the largest
    inlier residual).  The start is the greedy tree of the heaviest edges; step k weighs an edge by
    weight / (1 + (|r| / sigma_k)^2)^2 with sigma_k = max(sigma_end, sigma0 / 2^k); an edge is an inlier when its residual at the
    output is at most ``edge_thresh``.  The angles are radians."""
    Rt = _args.tensor(R_rel).to(dtype=F64)
    if Rt.dim() == 3 and tuple(Rt.shape[1:]) == (3, 3):
        Rt = Rt.reshape(-1, 9)
    if Rt.dim() != 2 or Rt.shape[1] != 9:
        raise ValueError(f'R_rel must be [E, 3, 3] or [E, 9], got shape {tuple(Rt.shape)}')
    E = int(Rt.shape[0])
    e = _args.tensor(edges, np.int32)
    if tuple(e.shape) != (E, 2) or e.dtype not in (torch.int32, torch.int64):
        raise ValueError(f'edges must be int [E, 2] = [{E}, 2], got {e.dtype} {tuple(e.shape)}')
    w = None if weights is None else _args.tensor(weights).to(dtype=F64).reshape(-1)
    if w is not None and w.numel() != E:
        raise ValueError(f'weights must be [E] = [{E}], got shape {tuple(np.shape(weights))}')
    f = None if found is None else _args.tensor(found, np.int32)
    if f is not None and f.numel() != E:
        raise ValueError(f'found must be [E] = [{E}], got shape {tuple(f.shape)}')
    _check_rotations(n, E, root, iters, sigma0, sigma_end, edge_thresh)
    _args.no_cpu_tensors(_SUBJECT, R_rel, edges, weights, found)
    device = _args.device(device)
    Rt, e, w = on(Rt, device).contiguous(), on(e.to(dtype=I32), device).contiguous(), None if w is None else on(w, device).contiguous()
    with torch.cuda.device(device):
        return _enqueue_rotations(_lib.load_library(), Rt, e, w, _args.found_i32(f, device), int(n), E, root, iters, sigma0, sigma_end,
                                  edge_thresh, device)


def _check_positions(V, N, root, threshold, rounds, min_obs, power_iters):
    if N > MAX_POINTS:
        raise ValueError(f'between 1 and 2^20 points, got {N}')
    _args.check_int_range('root', root, 0, V - 1)
    _args.check_positive('threshold', threshold)
    _args.check_int_range('rounds', rounds, 1, MAX_ROUNDS)
    _args.check_int_range('min_obs', min_obs, 1, MAX_POINTS)
    _args.check_int_range('power_iters', power_iters, 1, MAX_POWER)


def _enqueue_positions(lib, pts, vis, cams, R, located, V, N, found, root, threshold, rounds, min_obs, power_iters, device):
    """every tensor on ``device`` already, every argument checked -> the dict of ``solve_positions``"""
    count = ctypes.c_size_t()
    check_op(lib.cotr_solve_positions_work_doubles(V, N, ctypes.byref(count)), 'cotr_solve_positions_work_doubles')
    C, poses, X, used, stats, info, work = _args.empty(device, ((V, 3), F64), ((V, 12), F64), ((N, 3), F64), ((V, N), U8), (4, F64), (8, I32),
                                                       (count.value, F64))
    check_op(lib.cotr_solve_positions(ptr(pts), ptr(vis), ptr(cams), ptr(R), ptr(located), V, N, ptr(found), int(root), float(threshold),
                                      int(rounds), int(min_obs), int(power_iters), ptr(C), ptr(poses), ptr(X), ptr(used), ptr(stats), ptr(info),
                                      ptr(work), _lib.current_stream_ptr()), 'cotr_solve_positions')
    poses = poses.reshape(V, 3, 4)
    # camera-to-world [R^T | C], the form fuse_images takes (torch ops on the device: no host wait)
    c2w = torch.zeros((V, 4, 4), dtype=F64, device=device)
    c2w[:, :3, :3] = poses[:, :, :3].transpose(1, 2)
    c2w[:, :3, 3] = C
    c2w[:, 3, 3] = 1.0
    return dict(C=C, poses=poses, c2w=c2w, X=X, used=used.bool(), stats=stats, info=info)


def solve_positions(points, cameras, R, visible=None, located=None, found=None, root=0, threshold=4.0, rounds=3, min_obs=8, power_iters=16,
                    device=None):
    """One ``cotr_solve_positions`` call on the current stream: points [V,N,2], cameras and visible as for
    ``triangulate_views``, R [V,3,3] the world-to-camera rotations (``average_rotations``' R), located [V] int (its located;
    None: every view) -> dict of device tensors: C float64 [V,3] the camera centres (the root at the origin, the
    root-mean-square distance of the others from it 1, NaN for a view not placed), poses float64 [V,3,4] = [R | -R C], c2w
    float64 [V,4,4], X float64 [N,3] (NaN for a point that is not solved), used bool [V,N] (the observations of the last
    round), stats float64 [4] = (lambda0, lambda1, the cost of the last round, 0), info int32 [8] = (ok, observations in the
    last round, views placed, views dropped (fewer than ``min_obs`` observations), points solved, positive depths, negative
    depths, rounds run).  Round 1 trusts ``visible`` (feed it the two-view inlier masks); each later round keeps the
    observations whose ray passes the point within ``threshold`` px, in front of the camera.  lambda0 and lambda1 are the two
    smallest eigenvalues of the reduced matrix (``power_iters`` steps of inverse iteration each): the solution is ambiguous,
    with ok still 1, when lambda1 is as small as lambda0 - the tracks leave a group of views untied to the root.  ``found``:
    a device int32 tensor whose first entry 0 zeroes every output."""
    pts, V, N = _args.view_points(points)
    cams, vis = _args.cam_rows(cameras, V), _args.visible(visible, V, N)
    Rt = _args.tensor(R).to(dtype=F64)
    if Rt.numel() != V * 9:
        raise ValueError(f'R must be [V, 3, 3] = [{V}, 3, 3], got shape {tuple(Rt.shape)}')
    loc = None if located is None else _args.tensor(located, np.int32)
    if loc is not None and loc.numel() != V:
        raise ValueError(f'located must be [V] = [{V}], got shape {tuple(loc.shape)}')
    _check_positions(V, N, root, threshold, rounds, min_obs, power_iters)
    _args.no_cpu_tensors(_SUBJECT, points, cameras, R, visible, located, found)
    device = _args.device(device)
    pts, cams, Rt = on(pts, device, 16), on(cams, device), on(Rt.reshape(V, 9), device).contiguous()
    vis, found, located = _args.mask_u8(vis, (V, N), device), _args.found_i32(found, device), _args.found_i32(loc, device)
    with torch.cuda.device(device):
        return _enqueue_positions(_lib.load_library(), pts, vis, cams, Rt, located, V, N, found, root, threshold, rounds, min_obs, power_iters,
                                  device)


def _host(r):
    out = {k: v.cpu().numpy() for k, v in r.items()}
    for k in ('used', 'live', 'inlier'):
        if k in out:
            out[k] = out[k].astype(np.uint8)
    return out


def average_rotations_host(R_rel, edges, n, **kw):
    """``average_rotations`` with host arrays back (live, inlier as uint8)."""
    return _host(average_rotations(R_rel, edges, n, **kw))


def solve_positions_host(points, cameras, R, **kw):
    """``solve_positions`` with host arrays back (used as uint8)."""
    return _host(solve_positions(points, cameras, R, **kw))
