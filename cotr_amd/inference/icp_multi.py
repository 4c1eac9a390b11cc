"""Joint registration of N depth maps on the device: multi-way point-to-plane ICP.  Where ``register_captures`` and
``icp_depth`` place one capture against another, ``icp_multiview`` refines all free camera-to-world poses together, on every
pixel of every ordered pair (edge) of a graph of views, with one normal system per step - the dense counterpart of
``bundle_adjust``.

``vertex_normal_maps`` is one call of cotr_amd/csrc/icp_multi.hip (``cotr_icp_maps``), ``icp_multiview`` one of
``cotr_icp_multiview`` with device tensors, ``refine_poses`` the same on ``cotr_amd.data.Capture`` with host results, and
``ZoomEngine.fuse(..., joint_iters=4)`` runs it between the pairwise registration and the fusion.  The rules are the library's
own.  No CPU fallback."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args
from ._args import F64, I32
from .icp import EDGE, MAX_ITERS, MAX_STRIDE, NORMAL_COS

MAX_VIEWS = _args.MAX_VIEWS
PIVOT_TOL = 1e-9
BANDS, ROW = 8, 32   # edge_sums [E, BANDS, ROW]: 29 sums, the usable source pixels, 0, 0 of every band of source rows
STOP_REASONS = ('ran all', 'too few pairs', 'singular', 'not finite')
D3 = ctypes.c_double * 3


def check(max_dist, normal_cos=NORMAL_COS, pivot_tol=PIVOT_TOL, iters=10, stride=1):
    _args.check_positive('max_dist', max_dist)
    if not -1 <= normal_cos <= 1:
        raise ValueError(f'normal_cos must be in [-1, 1], got {normal_cos}')
    if not 0 < pivot_tol < 1:
        raise ValueError(f'pivot_tol must be in (0, 1), got {pivot_tol}')
    _args.check_int_range('iters', iters, 0, MAX_ITERS)
    _args.check_int_range('stride', stride, 1, MAX_STRIDE)


def _check_stack(shape, what, least):
    """the size rules of a stack of n maps of H x W pixels -> n"""
    n, H, W = (int(v) for v in shape)
    if not least <= n <= MAX_VIEWS:
        raise ValueError(f'between {least} and {MAX_VIEWS} {what}, got {n}')
    if H < 3 or W < 3:
        raise ValueError(f'{what}: maps of at least 3 x 3 pixels, got {H} x {W}')
    if n * H * W > 1 << 28:
        raise ValueError(f'{what}: at most 2^28 pixels in all, got {n} x {H} x {W}')
    return n


def _check_depths(depths, least=1):
    if len(depths.shape) != 3 or depths.shape[0] < 1:
        raise ValueError(f'depths must be [n, H, W], got shape {tuple(depths.shape)}')
    _args.check_depth(depths[0])
    return _check_stack(depths.shape, 'depth maps', least)


def _enqueue_maps(lib, depths, K, edge):
    """depths on its device, every argument checked -> (maps float64 [n,H,W,6], info int32 [n,4])"""
    n, H, W = (int(v) for v in depths.shape)
    maps, info = _args.empty(depths.device, ((n, H, W, 6), F64), ((n, 4), I32))
    check_op(lib.cotr_icp_maps(ptr(depths), n, H, W, K, float(edge), ptr(maps), ptr(info), _lib.current_stream_ptr()), 'cotr_icp_maps')
    return maps, info


def vertex_normal_maps(depths, Ks, edge=EDGE, device=None):
    """``cotr_icp_maps`` on the current stream: the depth maps ``depths`` float32 [n,H,W] (1 <= n <= 32) with the cameras ``Ks``
    [n,3,3] (host; one [3,3] serves every map) -> (maps float64 [n,H,W,6]: the vertex and the unit normal of every pixel by the
    rule of ``icp_depth``, NaN where there is none, info int32 [n,4] = (pixels with a vertex, pixels with a normal, 0, 0)), both
    on the device.  ``edge``: the relative depth step across which no normal is taken."""
    if not torch.is_tensor(depths):
        depths = np.asarray(depths)
    n = _check_depths(depths)
    _, K = _args.cameras(Ks, n)
    _args.check_positive('edge', edge)
    _args.no_cpu_tensors('the joint registration runs', depths)
    device = _args.device(device)
    depths = on(_args.tensor(depths, np.float32), device).contiguous()
    with torch.cuda.device(device):
        return _enqueue_maps(_lib.load_library(), depths, K, edge)


def all_pairs(n):
    """every ordered pair of n views -> int32 [n (n - 1), 2]"""
    return np.array([(a, b) for a in range(n) for b in range(n) if a != b], dtype=np.int32)


def _edges(edges, n):
    if edges is None:
        return torch.from_numpy(all_pairs(n))
    e = _args.tensor(edges, np.int32)
    if e.dim() != 2 or e.shape[1] != 2 or not 1 <= e.shape[0] <= n * (n - 1):
        raise ValueError(f'edges must be [E, 2] with 1 <= E <= n (n - 1) = {n * (n - 1)}, got shape {tuple(e.shape)}')
    if e.dtype not in (torch.int32, torch.int64):
        raise ValueError(f'edges must be int32 or int64, got {e.dtype}')
    return e.to(dtype=I32)


def _fixed_mask(fixed, n):
    fixed = [int(v) for v in np.asarray(fixed).reshape(-1)]
    if not fixed or any(not 0 <= v < n for v in fixed):
        raise ValueError(f'fixed must name at least one of the {n} views, got {fixed}')
    mask = 0
    for v in fixed:
        mask |= 1 << v
    return mask


def _enqueue_multiview(lib, maps, K, rows, edges, fixed_mask, centre, found, max_dist, normal_cos, pivot_tol, iters, stride, tables):
    """every tensor on the device of ``maps`` already, every argument checked -> the dict of ``icp_multiview`` without maps"""
    n, H, W = (int(v) for v in maps.shape[:3])
    E, iters, stride = int(edges.shape[0]), int(iters), int(stride)
    device = maps.device
    c2w, info, view_info, stats, sums = _args.empty(device, ((n, 4, 4), F64), (8, I32), ((n, 4), I32), (2, F64), ((E, BANDS, ROW), F64))
    out = dict(c2w=c2w, info=info, view_info=view_info, stats=stats, edge_sums=sums, edges=edges)
    if tables:
        n_src = -(-H // stride) * -(-W // stride)
        out['hist'], out['assoc'] = _args.empty(device, ((iters + 1, 4), F64), ((E, n_src), I32))
    check_op(lib.cotr_icp_multiview(ptr(maps), n, H, W, K, ptr(rows), ptr(edges), E, fixed_mask, D3(*centre), ptr(found), float(max_dist),
                                    float(normal_cos), float(pivot_tol), iters, stride, ptr(c2w), ptr(info), ptr(view_info), ptr(stats), ptr(sums),
                                    ptr(out.get('hist')), ptr(out.get('assoc')), _lib.current_stream_ptr()), 'cotr_icp_multiview')
    return out


def icp_multiview(maps_or_depths, Ks, c2ws, edges=None, fixed=(0,), centre=None, max_dist=0.05, normal_cos=NORMAL_COS, pivot_tol=PIVOT_TOL,
                  iters=10, stride=1, found=None, tables=False, edge=EDGE, device=None):
    """One ``cotr_icp_multiview`` call on the current stream: the camera-to-world poses ``c2ws`` [n,4,4] (float64; a device
    tensor is read in place) of n depth maps of one size (2 <= n <= 32), refined together by up to ``iters`` Gauss-Newton steps
    on the point-to-plane residuals of every edge.  ``maps_or_depths``: float64 [n,H,W,6] as ``vertex_normal_maps`` returns, or
    float32 depth maps [n,H,W], whose maps are taken first (``edge``).  ``Ks`` [n,3,3] or one [3,3], host.  ``edges`` [E,2] int =
    (a, b): view b's pixels are paired with the pixels of view a they project to, by the gates of ``icp_depth`` (``max_dist``,
    ``normal_cos``, every ``stride``-th pixel); None: every ordered pair; a device tensor is read in place, and an entry that
    names no pair of views, or names one again, is skipped.  ``fixed``: the views that do not move.  ``centre`` [3]: the point
    the pose twists turn about; None: the mean of the start camera centres, which a device ``c2ws`` cannot give without a
    host trip, so it is required then.  ``found`` int [n]: a view whose entry is 0 takes no part.
    -> dict of device tensors: c2w float64 [n,4,4], info int32 [8] = (ok, steps taken, pairs, stop reason (0 ran all, 1 no
    free view or fewer than 6 pairs, 2 the system is singular: a Cholesky pivot <= ``pivot_tol`` times its diagonal entry,
    3 not finite), live edges, kept edges, free views, 0), view_info int32 [n,4] = (free, pairs, kept edges, 0), stats
    float64 [2] = (sum r^2, rmse), edge_sums float64 [E,8,32] (the 29 sums and the usable pixels of every band of every edge),
    edges int32 [E,2]; with ``tables=True`` also hist float64 [iters + 1, 4], assoc int32 [E, n_src] and maps.  A stop leaves
    the poses of the evaluation it happened at: at the first one, the start."""
    if not torch.is_tensor(maps_or_depths):
        maps_or_depths = np.asarray(maps_or_depths)
    m = maps_or_depths
    is_maps = len(m.shape) == 4
    if is_maps:
        if m.dtype not in (torch.float64, np.float64) or m.shape[3] != 6:
            raise ValueError(f'maps must be float64 [n, H, W, 6], got {m.dtype} {tuple(m.shape)}')
        n = _check_stack(m.shape[:3], 'maps', 2)
    else:
        n = _check_depths(m, least=2)
    _, K = _args.cameras(Ks, n)
    rows = _args.c2w_rows(c2ws, n)
    e = _edges(edges, n)
    mask = _fixed_mask(fixed, n)
    check(max_dist, normal_cos, pivot_tol, iters, stride)
    _args.check_positive('edge', edge)
    if centre is None:
        if rows.is_cuda:
            raise ValueError('centre must be given with poses on the device (its default is the mean of the start camera centres)')
        centre = rows.view(n, 4, 4)[:, :3, 3].mean(dim=0).numpy()
    centre = [float(v) for v in np.asarray(centre, dtype=np.float64).reshape(-1)]
    if len(centre) != 3 or not np.isfinite(centre).all():
        raise ValueError(f'centre must be 3 finite numbers, got {centre}')
    if found is not None and not torch.is_tensor(found):
        found = np.asarray(found)
    if found is not None and int(np.prod(tuple(found.shape))) != n:
        raise ValueError(f'found must be [{n}], got shape {tuple(found.shape)}')
    _args.no_cpu_tensors('the joint registration runs', m, c2ws, edges, found)
    device = _args.device(device)
    with torch.cuda.device(device):
        lib = _lib.load_library()
        if is_maps:
            maps = on(_args.tensor(m), device).contiguous()
        else:
            maps, _ = _enqueue_maps(lib, on(_args.tensor(m, np.float32), device).contiguous(), K, edge)
        out = _enqueue_multiview(lib, maps, K, on(rows, device).contiguous(), on(e, device).contiguous(), mask, centre,
                                 _args.found_i32(found, device), max_dist, normal_cos, pivot_tol, iters, stride, tables)
    if tables:
        out['maps'] = maps
    return out


def host_result(r):
    """the dict of ``icp_multiview`` -> (poses: list of c2w float64 [4,4], info dict) on the host, as ``refine_poses`` returns"""
    info, view, stats = r['info'].cpu().numpy(), r['view_info'].cpu().numpy(), r['stats'].cpu().numpy()
    poses = list(r['c2w'].cpu().numpy())
    return poses, dict(ok=bool(info[0]), steps=int(info[1]), pairs=int(info[2]), stop=STOP_REASONS[int(info[3])], live_edges=int(info[4]),
                       kept_edges=int(info[5]), free_views=int(info[6]), sum_r2=float(stats[0]), rmse=float(stats[1]),
                       view_free=[bool(v) for v in view[:, 0]], view_pairs=[int(v) for v in view[:, 1]], view_edges=[int(v) for v in view[:, 2]])


def overlap_edges(dist, min_overlap):
    """overlap matrix float32 [n,n] on the device (``cotr_amd.scene.overlap_matrix``: [i, j] = the share of capture i's depth
    support that capture j's points fall on) -> int32 [n (n - 1), 2] on the device: every ordered pair (a, b), a the target and b
    the source, whose cell [a, b] is above ``min_overlap``; the others are (-1, -1), which the call skips.  No host trip."""
    n = int(dist.shape[0])
    pairs = torch.from_numpy(all_pairs(n)).to(dist.device)
    keep = dist[pairs[:, 0].long(), pairs[:, 1].long()] > float(min_overlap)
    return torch.where(keep[:, None], pairs, torch.full_like(pairs, -1))


def refine_poses(caps, c2ws=None, edges=None, min_overlap=None, **kw):
    """The poses of the RGB-D captures ``caps`` (``cotr_amd.data.Capture`` of one depth-map size; ``c2ws``: their start poses,
    None: the captures' own) refined together by ``icp_multiview`` -> (poses: one c2w float64 [4,4] per capture, info:
    dict(ok, steps, pairs, stop (one of STOP_REASONS), live_edges, kept_edges, free_views, sum_r2, rmse, view_free, view_pairs,
    view_edges)).  ``edges`` [E,2]: the pairs to use; with ``min_overlap`` instead, the cells of ``overlap_matrix`` of the
    captures at their start poses above it, chosen on the device; neither: every ordered pair.  ``kw``: fixed, centre,
    max_dist, normal_cos, pivot_tol, iters, stride, found, edge."""
    caps = list(caps)
    if len(caps) < 2:
        raise ValueError(f'refine_poses needs at least two captures, got {len(caps)}')
    shapes = {tuple(cap.depth.shape) for cap in caps}
    if len(shapes) != 1:
        raise ValueError(f'the captures must share one depth-map size, got {sorted(shapes)}')
    if edges is not None and min_overlap is not None:
        raise ValueError('give edges or min_overlap, not both')
    start = [cap.c2w for cap in caps] if c2ws is None else list(c2ws)
    if len(start) != len(caps):
        raise ValueError(f'c2ws must hold one [4, 4] matrix for each of the {len(caps)} captures, got {len(start)}')
    start = [_args.pose_matrix(m) for m in start]
    if any(m is None for m in start):
        raise ValueError('c2w must be a finite [4, 4] matrix, got None')
    for cap in caps:
        _args.check_map(cap.depth, 'depth')
    check(kw.get('max_dist', 0.05), kw.get('normal_cos', NORMAL_COS), kw.get('pivot_tol', PIVOT_TOL), kw.get('iters', 10), kw.get('stride', 1))
    _fixed_mask(kw.get('fixed', (0,)), len(caps))
    _args.no_cpu_tensors('the joint registration runs', *[cap.depth for cap in caps])
    if min_overlap is not None:
        from ..scene import overlap_matrix
        edges = overlap_edges(overlap_matrix([cap._replace(c2w=m) for cap, m in zip(caps, start)]), min_overlap)
        kw.setdefault('device', edges.device)
    if any(torch.is_tensor(cap.depth) for cap in caps):
        device = _args.device(kw.get('device'))
        depths = torch.stack([on(_args.tensor(cap.depth, np.float32), device) for cap in caps])
    else:
        depths = np.stack([np.asarray(cap.depth) for cap in caps])
    Ks = np.stack([np.asarray(cap.K.cpu() if torch.is_tensor(cap.K) else cap.K, dtype=np.float64) for cap in caps])
    return host_result(icp_multiview(depths, Ks, start, edges=edges, **kw))
