"""The argument rules and allocations every geometry wrapper of this package shares (guided, homography, essential, pnp,
structure, bundle, rigid3d, icp, icp_multi, tsdf, depth, tracks; triangulate and warp for the scratch query and the CPU-tensor refusal): each rule is stated
here once, and a caller passes the words its own message differs by, so every message reads as that wrapper's.

The import rule (tests/test_wrapper_imports_cpu.py): a module of this package imports names that start with an underscore
only from here and from ``_ransac`` (what only the RANSAC estimators share, itself built on this module, never the other way) -
except the ``_enqueue_*`` functions, which one wrapper takes from another to chain device calls.  A rule two wrappers need
moves here; it is not imported from whichever wrapper had it first."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on

MAX_POINTS = 1 << 24
MAX_VIEWS = 32
K9 = ctypes.c_double * 9
F64, I32, U8 = torch.float64, torch.int32, torch.uint8


def device(device):
    return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


def no_cpu_tensors(subject, *xs):
    """``subject``: who runs, with its verb ('the warps run')"""
    if any(torch.is_tensor(x) and not x.is_cuda for x in xs):
        raise _lib.CotrHipError(f'{subject} on an MI355X only (HIP kernels, no CPU fallback): got a CPU tensor; '
                                'pass a numpy array or move the tensor with .cuda()')


# ---- arrays and tensors ---------------------------------------------------------------------------------------------------
def tensor(x, dtype=np.float64):
    """array (taken as ``dtype``; None: as it is) or tensor -> tensor, where it was"""
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype)))


def points(p, what, d=2, cv2=False):
    """[N,d] float64 tensor, where it was (float32 input is widened exactly); ``cv2``: its [N,1,d] is taken too"""
    t = tensor(p)
    if cv2 and t.dim() == 3 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 2 or t.shape[1] != d:
        raise ValueError(f'{what} must be [N, {d}], got shape {tuple(t.shape)}')
    return t.to(dtype=F64)


def flat(x, what, numel, must='be [3, 3]'):
    """a matrix or vector of ``numel`` entries in any shape -> float64 tensor [numel], where it was"""
    t = tensor(x)
    if t.numel() != numel:
        raise ValueError(f'{what} must {must}, got shape {tuple(t.shape)}')
    return t.to(dtype=F64).reshape(numel)


def view_points(points):
    """[V,N,2] -> (float64 tensor where it was, V, N)"""
    t = tensor(points)
    if t.dim() != 3 or t.shape[2] != 2:
        raise ValueError(f'points must be [V, N, 2], got shape {tuple(t.shape)}')
    V, N = int(t.shape[0]), int(t.shape[1])
    if not 2 <= V <= MAX_VIEWS:
        raise ValueError(f'between 2 and {MAX_VIEWS} views, got {V}')
    if not 1 <= N <= MAX_POINTS:
        raise ValueError(f'between 1 and 2^24 points, got {N}')
    return t.to(dtype=F64), V, N


def cam_rows(cameras, V):
    """[V,3,3] camera matrices, one [3,3] for every view, or [V,5] rows (fx, fy, cx, cy, skew) -> [V,5] float64 tensor"""
    if torch.is_tensor(cameras) and cameras.is_cuda:
        c = cameras.to(dtype=F64)
        if c.dim() == 3 and tuple(c.shape[1:]) == (3, 3):
            c = torch.stack([c[:, 0, 0], c[:, 1, 1], c[:, 0, 2], c[:, 1, 2], c[:, 0, 1]], dim=1)
    else:
        k = np.asarray(cameras.cpu() if torch.is_tensor(cameras) else cameras, dtype=np.float64)
        if k.shape == (3, 3):
            k = np.broadcast_to(k, (V, 3, 3))
        if k.ndim == 3 and k.shape[1:] == (3, 3):
            k = np.stack([k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2], k[:, 0, 1]], axis=1)
        if k.ndim == 2 and k.shape[1] == 5 and (not np.isfinite(k).all() or (k[:, :2] == 0).any()):
            raise ValueError('cameras must be finite with focal lengths that are not 0')
        c = torch.from_numpy(np.ascontiguousarray(k))
    if c.dim() != 2 or tuple(c.shape) != (V, 5):
        raise ValueError(f'cameras must be [V, 3, 3], [3, 3] or [V, 5] for {V} views, got shape {tuple(np.shape(cameras))}')
    return c


def pose_rows(poses, V):
    """[V,3,4] or [V,4,4] world-to-camera matrices, or [V,12] -> [V,12] float64 tensor"""
    t = tensor(poses).to(dtype=F64)
    if t.dim() == 3 and tuple(t.shape[1:]) == (4, 4):
        t = t[:, :3]
    if t.dim() == 3 and tuple(t.shape[1:]) == (3, 4):
        t = t.reshape(t.shape[0], 12)
    if t.dim() != 2 or tuple(t.shape) != (V, 12):
        raise ValueError(f'poses must be [V, 3, 4], [V, 4, 4] or [V, 12] for {V} views, got shape {tuple(np.shape(poses))}')
    return t


def visible(v, V, N):
    """[V,N] flags as they are (None stays None); ``mask_u8`` takes them to the device"""
    t = None if v is None else tensor(v, None)
    if t is not None and tuple(t.shape) != (V, N):
        raise ValueError(f'visible must be [V, N] = [{V}, {N}], got shape {tuple(t.shape)}')
    return t


def mask_u8(m, shape, device):
    return None if m is None else (on(m, device).reshape(shape) != 0).to(U8)


def found_i32(found, device):
    return None if found is None else on(found, device).to(I32).reshape(-1)


def camera(K, what):
    """[3,3] upper-triangular camera matrix -> 9 host doubles; finite, focal lengths not 0"""
    k = np.asarray(K.cpu() if torch.is_tensor(K) else K, dtype=np.float64)
    if k.shape != (3, 3):
        raise ValueError(f'{what} must be [3, 3], got shape {k.shape}')
    if not np.isfinite(k[[0, 0, 0, 1, 1], [0, 1, 2, 1, 2]]).all() or k[0, 0] == 0 or k[1, 1] == 0:
        raise ValueError(f'{what} must be finite with focal lengths that are not 0')
    return K9(*k.reshape(9))


def pose_matrix(c2w):
    """camera-to-world [4,4] -> contiguous host float64 array (None stays None)"""
    if c2w is None:
        return None
    m = np.asarray(c2w.cpu() if torch.is_tensor(c2w) else c2w, dtype=np.float64)
    if m.shape != (4, 4) or not np.isfinite(m).all():
        raise ValueError(f'c2w must be a finite [4, 4] matrix, got shape {m.shape}')
    return np.ascontiguousarray(m)


def pose_on(m, device):
    """what ``pose_matrix`` returned -> the [16] device tensor the kernels read"""
    return None if m is None else on(m.reshape(16), device)


def c2w_rows(c2ws, n):
    """[n,4,4] camera-to-world: a device tensor as it is, anything else through ``pose_matrix`` -> float64 [n,16], where it was"""
    if torch.is_tensor(c2ws) and c2ws.is_cuda:
        if c2ws.dtype != F64 or c2ws.numel() != n * 16:
            raise ValueError(f'c2ws on the device must be float64 [{n}, 4, 4], got {c2ws.dtype} {list(c2ws.shape)}')
        return c2ws.reshape(n, 16)
    if len(c2ws) != n:
        raise ValueError(f'c2ws must hold one [4, 4] matrix for each of the {n} depth maps, got {len(c2ws)}')
    return torch.from_numpy(np.stack([pose_matrix(m) for m in c2ws]).reshape(n, 16))


def cameras(Ks, n):
    """[n,3,3] camera matrices, or one [3,3] for every map -> (one ``camera`` per map, the [n][9] host doubles a call takes)"""
    k = np.asarray(Ks.cpu() if torch.is_tensor(Ks) else Ks, dtype=np.float64)
    if k.shape == (3, 3):
        k = np.broadcast_to(k, (n, 3, 3))
    if k.shape != (n, 3, 3):
        raise ValueError(f'Ks must be [{n}, 3, 3] or [3, 3], got shape {k.shape}')
    ks = [camera(m, 'Ks') for m in k]
    return ks, (ctypes.c_double * (9 * n))(*[v for m in ks for v in m])


def check_depth(depth):
    if (torch.is_tensor(depth) and depth.dtype != torch.float32) or (not torch.is_tensor(depth) and np.asarray(depth).dtype != np.float32):
        raise ValueError(f'depth must be float32, got {depth.dtype if hasattr(depth, "dtype") else type(depth)}')
    if len(depth.shape) != 2 or depth.shape[0] < 1 or depth.shape[1] < 1:
        raise ValueError(f'depth must be [H, W], got shape {tuple(depth.shape)}')
    if int(depth.shape[0]) * int(depth.shape[1]) > 1 << 28:
        raise ValueError(f'depth: at most 2^28 pixels, got {depth.shape[0]} x {depth.shape[1]}')


def check_map(depth, what):
    """a depth map normals can be taken on"""
    check_depth(depth)
    if depth.shape[0] < 3 or depth.shape[1] < 3:
        raise ValueError(f'{what}: a map of at least 3 x 3 pixels, got {depth.shape[0]} x {depth.shape[1]}')


# ---- scalars --------------------------------------------------------------------------------------------------------------
def check_positive(name, v):
    if not (v > 0 and np.isfinite(v)):
        raise ValueError(f'{name} must be finite and > 0, got {v}')


def check_distance(v):
    check_positive('distance_thresh', v)


def check_sq_float32(threshold, ransac=False):
    """the kernels compare squared float32 errors: the squared threshold must be one they can tell from 0 and from inf"""
    with np.errstate(over='ignore', under='ignore'):
        sq = np.float32(float(threshold) * float(threshold))
    if not (sq > 0 and np.isfinite(sq)):
        raise ValueError(f'the squared {"RANSAC " if ransac else ""}threshold must be a finite float32 that is not 0, got threshold {threshold}')


def check_int_range(name, v, lo, hi, integer=True):
    """``integer=False``: the callers that never insisted on a whole number (they pass ``int(v)`` on) still do not"""
    if not lo <= v <= hi or (integer and int(v) != v):
        raise ValueError(f'{name} must be {"an integer " if integer else ""}in [{lo}, {hi}], got {v}')


def count_pairs(n, m, least, too_few, a, b):
    """``n`` of ``a`` against ``m`` of ``b``; ``too_few``: the message below ``least`` correspondences, the model's own"""
    if m != n:
        raise ValueError(f'{a} and {b} must have the same length, got {n} and {m}')
    if n < least:
        raise ValueError(f'{too_few}, got {n}')
    if n > MAX_POINTS:
        raise ValueError(f'at most 2^24 correspondences, got {n}')


# ---- allocations ----------------------------------------------------------------------------------------------------------
def scratch(lib, name, *dims, device):
    """the library's ``name`` (a ``*_scratch_bytes`` function) asked at ``dims`` -> (uint8 tensor of that size, the size)"""
    nbytes = ctypes.c_size_t()
    check_op(getattr(lib, name)(*dims, ctypes.byref(nbytes)), name)
    return torch.empty(nbytes.value, dtype=U8, device=device), nbytes.value


def empty(device, *specs):
    """(shape, dtype), ... -> that many uninitialised tensors on ``device``"""
    return [torch.empty(shape, dtype=dtype, device=device) for shape, dtype in specs]


# ---- host results ---------------------------------------------------------------------------------------------------------
def found_flag(r):
    return r['info'].cpu().numpy()[0]


def mask_column(t):
    """device mask [n] -> uint8 [n,1], as cv2 shapes it"""
    return t.cpu().numpy().astype(np.uint8).reshape(-1, 1)


def c2w_from(R, t, scale=1.0, invert=False):
    """device R [3,3], t [3] -> host [4,4] = [scale R | t], or with ``invert`` the inverse of the rigid [R | t]"""
    R, t = scale * R.cpu().numpy(), t.cpu().numpy()
    c2w = np.eye(4)
    c2w[:3, :3] = R.T if invert else R
    c2w[:3, 3] = -(R.T @ t) if invert else t
    return c2w
