"""``triangulate_corr`` (COTR/inference/inference_helper.py:293-308): sparse correspondences -> a dense per-pixel map of A.

The reference triangulates the correspondences' A points (normalised by A's size) with scipy's Delaunay and renders the
triangles with vispy/OpenGL, B's normalised coordinates as vertex colours, into a float framebuffer of A's size.  Here the
rasterisation is one ``cotr_raster_mesh`` call on the current device (cotr_amd/csrc/triangulate.hip; semantics and tie rule
in DESIGN.md 3g).  The triangulation is scipy's on the host by default (imported when called); with ``simplices='device'``
it is one ``cotr_delaunay`` call (cotr_amd/csrc/delaunay.hip; an exact rule of its own) and nothing
leaves the device.  No CPU fallback."""
import numpy as np
import torch

from .. import _lib
from .._lib import check_op, ptr
from . import _args


def raster_mesh(verts, attrs, tris, H, W, device=None):
    """Rasterise the triangles ``tris`` [T,3] over ``verts`` [N,2] (normalised A points) carrying ``attrs`` [N,2] into an
    H x W canvas on ``device`` (default: the current one), on the current stream.  Returns (out float32 [H,W,2],
    mask bool [H,W]) device tensors."""
    lib = _lib.load_library()
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    verts = torch.as_tensor(verts, dtype=torch.float32).to(device).contiguous()
    attrs = torch.as_tensor(attrs, dtype=torch.float32).to(device).contiguous()
    tris = torch.as_tensor(np.asarray(tris, dtype=np.int32) if not torch.is_tensor(tris) else tris,
                           dtype=torch.int32).to(device).contiguous()
    n_tris = tris.numel() // 3
    scratch, nbytes = _args.scratch(lib, 'cotr_raster_mesh_scratch_bytes', n_tris, H, W, device=device)
    out = torch.empty((H, W, 2), dtype=torch.float32, device=device)
    mask = torch.empty((H, W), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        check_op(lib.cotr_raster_mesh(ptr(verts), verts.shape[0], ptr(attrs), ptr(tris), n_tris, H, W, ptr(out), ptr(mask), ptr(scratch),
                                      nbytes, _lib.current_stream_ptr()), 'cotr_raster_mesh')
    return out, mask.bool()


MAX_POINTS = 65536


def delaunay(points, device=None, as_tensor=False):
    """The Delaunay triangulation of ``points`` [n, 2] (numpy array or tensor, cast to float32; n <= 65536) by the exact rule
    of DESIGN.md 3g-bis, one ``cotr_delaunay`` call on ``device`` (default: a device tensor's own, else the current one), on
    the current stream -> int32 array [T, 3]: counter-clockwise triangles, lowest index first, ordered by that index.

    as_tensor: return the device tensors (tris int32 [2 n, 3], rows past the count -1; info int32 [2] = count, status)
        without reading the count back: no host wait."""
    shape = tuple(points.shape) if hasattr(points, 'shape') else np.shape(points)
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError(f'points must be [n, 2], got shape {shape}')
    n = shape[0]
    if n > MAX_POINTS:
        raise ValueError(f'delaunay takes at most {MAX_POINTS} points, got {n}')
    lib = _lib.load_library()
    if device is None:
        device = points.device if torch.is_tensor(points) and points.is_cuda else torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    verts = torch.as_tensor(points if torch.is_tensor(points) else np.asarray(points), dtype=torch.float32).to(device).contiguous()
    scratch, nbytes = _args.scratch(lib, 'cotr_delaunay_scratch_bytes', n, device=device)
    tris = torch.empty((lib.cotr_delaunay_max_tris(n), 3), dtype=torch.int32, device=device)
    info = torch.empty(2, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        check_op(lib.cotr_delaunay(ptr(verts), n, ptr(tris), ptr(info), ptr(scratch), nbytes, _lib.current_stream_ptr()),
                 'cotr_delaunay')
    if as_tensor:
        return tris, info
    count, status = info.tolist()
    if status != 0:
        raise _lib.CotrHipError(f'cotr_delaunay: a walk reached its bound (status {status})')
    return tris[:count].cpu().numpy()


def _triangulate_corr_device(corr, from_shape, to_shape, return_mask, as_tensor):
    """triangulate_corr(simplices='device'): corr on the device, normalised there as the host path normalises (float64
    quotients rounded to float32), cotr_delaunay, the whole capacity of triangles to cotr_raster_mesh"""
    if not torch.is_tensor(corr):
        corr = torch.from_numpy(np.array(corr, dtype=np.float64))
    if corr.dim() != 2 or corr.shape[1] != 4:
        raise ValueError(f'corr must be [N, 4] (x_a, y_a, x_b, y_b), got shape {tuple(corr.shape)}')
    if corr.shape[0] > MAX_POINTS:
        raise ValueError(f"simplices='device' takes at most {MAX_POINTS} correspondences, got {corr.shape[0]}")
    (Ha, Wa), (Hb, Wb) = from_shape, to_shape
    device = corr.device if corr.is_cuda else torch.device('cuda', torch.cuda.current_device())
    with torch.cuda.device(device):
        c = corr.to(device).double()
        norm = torch.stack([c[:, 0] / Wa, c[:, 1] / Ha, c[:, 2] / Wb, c[:, 3] / Hb], 1).float()   # (divisors as scalars: no upload)
        verts, attrs = norm[:, :2].contiguous(), norm[:, 2:].contiguous()
        tris, _ = delaunay(verts, as_tensor=True)
        out, mask = raster_mesh(verts, attrs, tris, int(Ha), int(Wa), device=device)
        render = out.double()
        render[..., 0] *= float(Wb)
        render[..., 1] *= float(Hb)
    if not as_tensor:
        render, mask = render.cpu().numpy(), mask.cpu().numpy()
    return (render, mask) if return_mask else render


def triangulate_corr(corr, from_shape, to_shape, simplices=None, return_mask=False, as_tensor=False):
    """``corr`` [N,4] = (x_a, y_a, x_b, y_b) px -> float64 [H_a, W_a, 2]: at every pixel centre of A, B's position by linear
    interpolation over the Delaunay triangle of the normalised A points that covers it, 0 outside their hull (the
    reference's return value).  ``from_shape`` / ``to_shape``: A's and B's image shapes (H, W, ...).

    simplices: triangles [T,3] of indices into ``corr`` to use instead of scipy's Delaunay, or 'device': triangulate with
        ``cotr_delaunay`` (no scipy, no trip through the host; at most 65536 correspondences).  ``corr`` may then be a
        device tensor, and with as_tensor=True the call neither waits for the device nor copies from the host: it can be
        captured into a graph.  Both triangulations are Delaunay; they differ only in the diagonal of cocircular points.
    return_mask: also return the bool [H_a, W_a] coverage mask.
    as_tensor: return device tensors (float64 map, bool mask) instead of numpy arrays: no copy back to the host, for
        callers that warp with ``warp_by_map``."""
    if isinstance(simplices, str):
        if simplices != 'device':
            raise ValueError(f"simplices must be None, 'device' or an integer array [T, 3], got {simplices!r}")
        return _triangulate_corr_device(corr, tuple(from_shape[:2]), tuple(to_shape[:2]), return_mask, as_tensor)
    corr = np.array(corr, dtype=np.float64)
    if corr.ndim != 2 or corr.shape[1] != 4:
        raise ValueError(f'corr must be [N, 4] (x_a, y_a, x_b, y_b), got shape {corr.shape}')
    to_shape, from_shape = tuple(to_shape[:2]), tuple(from_shape[:2])
    corr = corr / np.concatenate([from_shape[::-1], to_shape[::-1]])
    if simplices is None:
        try:
            from scipy.spatial import Delaunay
        except ImportError as e:
            raise ImportError('triangulate_corr needs scipy (scipy.spatial.Delaunay) to triangulate the correspondences; '
                              'install scipy or pass simplices=') from e
        simplices = Delaunay(corr[:, :2]).simplices
    else:
        simplices = np.asarray(simplices)
        if simplices.ndim != 2 or simplices.shape[1] != 3 or not np.issubdtype(simplices.dtype, np.integer):
            raise ValueError(f'simplices must be an integer array [T, 3], got {simplices.dtype} {simplices.shape}')
        if simplices.size and (simplices.min() < 0 or simplices.max() >= len(corr)):
            raise ValueError(f'simplices index outside [0, {len(corr)})')
    out, mask = raster_mesh(corr[:, :2].astype(np.float32), corr[:, 2:].astype(np.float32), simplices.astype(np.int32),
                            int(from_shape[0]), int(from_shape[1]))
    scale = np.array(to_shape[::-1])
    if as_tensor:
        render = out.double() * torch.as_tensor(scale, dtype=torch.float64, device=out.device)
        return (render, mask) if return_mask else render
    render = out.cpu().numpy() * scale          # float32 * int64 -> float64 [H_a, W_a, 2]
    return (render, mask.cpu().numpy()) if return_mask else render
