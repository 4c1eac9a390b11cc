"""Dense registration of two depth maps on the device: projective data association with a point-to-plane Gauss-Newton
step (the ICP of KinectFusion), which uses every pixel of both captures where ``register_captures`` fits a few hundred
sparse correspondences.

``icp_depth`` is one call of cotr_amd/csrc/icp.hip (``cotr_icp_depth``) with device tensors, ``refine_registration`` the same
on two ``cotr_amd.data.Capture`` with host results, and ``register_captures(..., icp_iters=10)`` (rigid3d.py) enqueues it behind
the sparse registration as one device sequence.  The model is x_a = R x_b + t; the rules are the library's own (DESIGN.md
3h-9).  No CPU fallback."""
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args
from ._args import F64, I32

MAX_ITERS = 64
MAX_STRIDE = 64
NORMAL_COS, EDGE, COND_TOL = 0.5, 0.05, 1e-6   # the defaults of icp_depth, and what register_captures(icp_iters=...) runs it with
STOP_REASONS = ('ran all', 'too few pairs', 'ill-conditioned', 'not finite')


def check(max_dist, normal_cos=NORMAL_COS, edge=EDGE, cond_tol=COND_TOL, iters=10, stride=1):
    _args.check_positive('max_dist', max_dist)
    if not -1 <= normal_cos <= 1:
        raise ValueError(f'normal_cos must be in [-1, 1], got {normal_cos}')
    _args.check_positive('edge', edge)
    if not 0 < cond_tol < 1:
        raise ValueError(f'cond_tol must be in (0, 1), got {cond_tol}')
    _args.check_int_range('iters', iters, 0, MAX_ITERS)
    _args.check_int_range('stride', stride, 1, MAX_STRIDE)


def _pose(R0, t0):
    """-> R [9], t [3] float64 tensors, where they were"""
    def take(x, shape, what):
        t = _args.tensor(x)
        if tuple(t.shape) not in shape:
            raise ValueError(f'{what} must have shape {" or ".join(str(list(s)) for s in shape)}, got {list(t.shape)}')
        return t.to(dtype=torch.float64).reshape(-1)
    return take(R0, ((3, 3), (9,)), 'R0'), take(t0, ((3,), (3, 1)), 't0')


def _source_mask(src_mask, depth_b):
    if src_mask is None:
        return None
    m = _args.tensor(src_mask, None)
    if tuple(m.shape) != tuple(depth_b.shape):
        raise ValueError(f'src_mask must have the shape of depth_b {list(depth_b.shape)}, got {list(m.shape)}')
    if m.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f'src_mask must be bool or uint8, got {m.dtype}')
    return m.to(dtype=torch.uint8)


def _enqueue_icp(lib, depth_a, ka, depth_b, kb, R0, t0, c2w_a, found, src_mask, max_dist, normal_cos, edge, cond_tol, iters, stride, tables,
                 device):
    """every tensor on ``device`` already, every argument checked -> the dict of ``icp_depth``"""
    (Ha, Wa), (Hb, Wb) = (int(v) for v in depth_a.shape), (int(v) for v in depth_b.shape)
    iters, stride = int(iters), int(stride)
    scratch, nbytes = _args.scratch(lib, 'cotr_icp_depth_scratch_bytes', Ha, Wa, Hb, Wb, stride, device=device)
    R, t, info, stats = _args.empty(device, (9, F64), (3, F64), (8, I32), (2, F64))
    out = dict(t=t, info=info, stats=stats)
    if tables:
        n_src = -(-Hb // stride) * -(-Wb // stride)
        out['hist'], out['assoc'], out['maps_a'], out['maps_b'] = _args.empty(device, ((iters + 1, 32), F64), (n_src, I32), ((Ha, Wa, 6), F64),
                                                                              ((Hb, Wb, 6), F64))
    check_op(lib.cotr_icp_depth(ptr(depth_a), Ha, Wa, ka, ptr(depth_b), Hb, Wb, kb, ptr(R0), ptr(t0), ptr(c2w_a), ptr(found), ptr(src_mask),
                                float(max_dist), float(normal_cos), float(edge), float(cond_tol), iters, stride, ptr(R), ptr(out['t']),
                                ptr(out['info']), ptr(out['stats']), ptr(out.get('hist')), ptr(out.get('assoc')), ptr(out.get('maps_a')),
                                ptr(out.get('maps_b')), ptr(scratch), nbytes, _lib.current_stream_ptr()), 'cotr_icp_depth')
    out['R'] = R.view(3, 3)
    return out


def icp_depth(depth_a, K_a, depth_b, K_b, R0, t0, max_dist, normal_cos=NORMAL_COS, edge=EDGE, cond_tol=COND_TOL, iters=10, stride=1,
              c2w_a=None, src_mask=None, tables=False, device=None):
    """One ``cotr_icp_depth`` call on the current stream: the rigid motion x_a = R x_b + t between the depth maps ``depth_a``
    [Ha,Wa] and ``depth_b`` [Hb,Wb] (float32, cameras ``K_a``, ``K_b``), refined from the start (``R0`` [3,3], ``t0`` [3]; device
    tensors are read in place) by up to ``iters`` point-to-plane steps on the pairs that projective association finds: a source
    pixel of B (every ``stride``-th in x and y, where ``src_mask`` [Hb,Wb] is not 0) is paired with the pixel of A it projects
    to when their points lie within ``max_dist`` and their normals within ``normal_cos``; ``edge``: the relative depth step
    across which no normal is taken.  With ``c2w_a`` [4,4] the start and the result map B's camera frame to the world frame.
    -> dict of device tensors: R float64 [3,3], t float64 [3], info int32 [8] = (ok, steps taken, pairs, stop reason (0 ran
    all, 1 fewer than 6 pairs, 2 ill-conditioned: the smallest eigenvalue of the normal matrix <= ``cond_tol`` times the
    largest, 3 not finite), usable source pixels, pixels of A with a normal, 0, 0), stats float64 [2] = (sum r^2, rmse); with
    ``tables=True`` also hist float64 [iters + 1, 32], assoc int32 [n_src], maps_a [Ha,Wa,6] and maps_b [Hb,Wb,6] (the
    tables tests check).  A stop leaves the pose of the evaluation it happened at: at the first one, the start."""
    _args.check_map(depth_a, 'depth_a')
    _args.check_map(depth_b, 'depth_b')
    ka, kb = _args.camera(K_a, 'K_a'), _args.camera(K_b, 'K_b')
    raw = (depth_a, depth_b, R0, t0, src_mask)
    R0, t0 = _pose(R0, t0)
    m = _args.pose_matrix(c2w_a)
    sm = _source_mask(src_mask, depth_b)
    check(max_dist, normal_cos, edge, cond_tol, iters, stride)
    _args.no_cpu_tensors('the dense registration runs', *raw)
    device = _args.device(device)
    depth_a, depth_b, R0, t0, m = on(depth_a, device), on(depth_b, device), on(R0, device), on(t0, device), _args.pose_on(m, device)
    sm = None if sm is None else on(sm, device)
    with torch.cuda.device(device):
        return _enqueue_icp(_lib.load_library(), depth_a, ka, depth_b, kb, R0, t0, m, None, sm, max_dist, normal_cos, edge, cond_tol, iters,
                            stride, tables, device)


def host_result(r):
    """the dict of ``icp_depth`` -> (c2w float64 [4,4], info dict) on the host, as ``refine_registration`` returns them"""
    info, stats = r['info'].cpu().numpy(), r['stats'].cpu().numpy()
    c2w = _args.c2w_from(r['R'], r['t'])
    return c2w, dict(ok=bool(info[0]), steps=int(info[1]), pairs=int(info[2]), stop=STOP_REASONS[int(info[3])], source_pixels=int(info[4]),
                     target_pixels=int(info[5]), sum_r2=float(stats[0]), rmse=float(stats[1]))


def refine_registration(cap_a, cap_b, c2w_b, max_dist=0.05, **kw):
    """The pose ``c2w_b`` [4,4] of the RGB-D capture ``cap_b`` in the world frame of the posed capture ``cap_a`` (both
    ``cotr_amd.data.Capture``; the c2w of ``cap_b`` is not read), refined on both depth maps by ``icp_depth`` -> (c2w_b float64
    [4,4], info: dict(ok, steps, pairs, stop (one of STOP_REASONS), source_pixels, target_pixels, sum_r2, rmse)).  ``kw``:
    normal_cos, edge, cond_tol, iters, stride, src_mask.  A stop at the first evaluation returns the pose given."""
    start = _args.pose_matrix(c2w_b)
    if start is None:
        raise ValueError('c2w_b must be a finite [4, 4] matrix, got None')
    return host_result(icp_depth(cap_a.depth, cap_a.K, cap_b.depth, cap_b.K, start[:3, :3], start[:3, 3], max_dist, c2w_a=cap_a.c2w, **kw))
