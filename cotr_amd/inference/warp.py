"""Warps of 8-bit images on the device: the ``cv2`` calls the reference's demos end with.

``warp_by_map`` is ``cv2.remap(img, map[..., 0], map[..., 1], INTER_LINEAR, borderMode=BORDER_CONSTANT)``
(demo_single_pair.py:43), ``warp_perspective`` / ``get_perspective_transform`` are ``cv2.warpPerspective`` /
``cv2.getPerspectiveTransform`` (demo_homography.py:46-48); ``warp_by_corr`` and ``paste_by_corners`` run the demos' last
lines in one call each.  Every warp is one ``cotr_warp_map`` / ``cotr_warp_perspective`` launch on the current stream
(cotr_amd/csrc/warp.hip); the rule - OpenCV's 8-bit bilinear remap: 1/32 px coordinates, integer weights, one rounding -
is stated in DESIGN.md 3i.  Coordinates are pixel indices, as in cv2 (no +0.5, unlike ``grid_sample``).

Images and maps are numpy arrays (uploaded to the current device) or device tensors (used where they are; all on one
device).  A CPU tensor is refused: there is no CPU fallback."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args
from .triangulate import triangulate_corr

MAX_SIDE = 16384


def _pick_device(*xs):
    """the device of the tensors among xs (they must agree), else the current one; every check here runs before an upload"""
    _args.no_cpu_tensors('the warps run', *xs)
    devs = {x.device for x in xs if torch.is_tensor(x)}
    if len(devs) > 1:
        raise ValueError(f'the tensors of one warp must be on one device, got {sorted(str(d) for d in devs)}')
    return devs.pop() if devs else torch.device('cuda', torch.cuda.current_device())


def check_image(img, what):
    """shape and dtype of an image argument -> (H, W, C); ValueError otherwise"""
    dtype = img.dtype
    if dtype not in (np.uint8, torch.uint8):
        raise ValueError(f'{what} must be uint8, got {dtype}')
    shape = tuple(img.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f'{what} must be [H, W] or [H, W, C], got shape {shape}')
    H, W, C = shape if len(shape) == 3 else shape + (1,)
    if C not in (1, 3, 4):
        raise ValueError(f'{what} must have 1, 3 or 4 channels, got {C}')
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f'{what}: H and W must be in [1, {MAX_SIDE}], got {H} x {W}')
    return H, W, C


def _check_map(map_):
    if map_.dtype not in (np.float32, np.float64, torch.float32, torch.float64):
        raise ValueError(f'map must be float32 or float64, got {map_.dtype}')
    shape = tuple(map_.shape)
    if len(shape) != 3 or shape[2] != 2:
        raise ValueError(f'map must be [H, W, 2] holding (x, y), got shape {shape}')
    if not (1 <= shape[0] <= MAX_SIDE and 1 <= shape[1] <= MAX_SIDE):
        raise ValueError(f'map: H and W must be in [1, {MAX_SIDE}], got {shape[0]} x {shape[1]}')
    return shape[0], shape[1]


def _check_background(background, Hd, Wd, C, img_ndim):
    if background is None:
        return
    shape = check_image(background, 'background')
    if shape != (Hd, Wd, C) or len(background.shape) != img_ndim:
        raise ValueError(f'background must have the result\'s shape {(Hd, Wd) + ((C,) if img_ndim == 3 else ())}, '
                         f'got {tuple(background.shape)}')


def _finish(dst, cover, img_ndim, return_cover, as_tensor):
    if img_ndim == 2:
        dst = dst[..., 0]
    if not as_tensor:
        dst = dst.cpu().numpy()
    if not return_cover:
        return dst
    cover = cover.bool()
    return dst, (cover if as_tensor else cover.cpu().numpy())


def warp_by_map(img, map, background=None, return_cover=False, as_tensor=False):   # noqa: A002 (cv2's argument name)
    """``cv2.remap(img, map[..., 0], map[..., 1], cv2.INTER_LINEAR, borderMode=cv2.BORDER_CONSTANT)`` by the rule of
    DESIGN.md 3i.  img: uint8 [H, W] or [H, W, C], C in 1, 3, 4; map: [Hd, Wd, 2] = (x, y) positions in ``img`` (pixel
    indices), float32 or float64 (rounded to float32, as the demo's ``.astype(np.float32)``) -> uint8 [Hd, Wd(, C)].

    background: uint8, the result's shape; where no tap with a non-zero weight lies inside ``img`` the result takes the
        background's pixel instead of the border value 0.
    return_cover: also return the bool [Hd, Wd] cover (``cv2.remap(ones) > 0``).
    as_tensor: return device tensors instead of numpy arrays."""
    Hs, Ws, C = check_image(img, 'img')
    Hd, Wd = _check_map(map)
    _check_background(background, Hd, Wd, C, len(img.shape))
    device = _pick_device(img, map, background)
    is_f64 = map.dtype in (np.float64, torch.float64)
    src, m = on(img, device), on(map, device, 16 if is_f64 else 8)
    bg = None if background is None else on(background, device)
    dst = torch.empty((Hd, Wd, C), dtype=torch.uint8, device=device)
    cover = torch.empty((Hd, Wd), dtype=torch.uint8, device=device) if return_cover else None
    with torch.cuda.device(device):
        check_op(_lib.load_library().cotr_warp_map(ptr(src), Hs, Ws, C, ptr(m), int(is_f64), Hd, Wd, ptr(dst), ptr(cover),
                                                   ptr(bg), _lib.current_stream_ptr()), 'cotr_warp_map')
    return _finish(dst, cover, len(img.shape), return_cover, as_tensor)


def _matrix(M):
    M = np.asarray(M.cpu() if torch.is_tensor(M) else M, dtype=np.float64)
    if M.shape != (3, 3):
        raise ValueError(f'M must be 3 x 3, got shape {M.shape}')
    if not np.isfinite(M).all():
        raise ValueError('M must be finite')
    return M


def invert_perspective(M):
    """the float64 inverse of a 3 x 3 transform (source -> destination becomes destination -> source, what the kernel
    takes); ValueError when M is singular"""
    M = _matrix(M)
    try:
        inv = np.linalg.inv(M)
    except np.linalg.LinAlgError:
        inv = None
    if inv is None or not np.isfinite(inv).all() or np.linalg.matrix_rank(M) < 3:
        raise ValueError('M is singular')
    return inv


def warp_perspective(img, M, dsize, inverse_map=False, background=None, return_cover=False, as_tensor=False):
    """``cv2.warpPerspective(img, M, dsize)`` (INTER_LINEAR, BORDER_CONSTANT 0; ``flags=cv2.WARP_INVERSE_MAP`` with
    inverse_map=True) by the rule of DESIGN.md 3i.  M: 3 x 3, source -> destination as cv2's default; it is inverted on the
    host in float64 (a singular M: ValueError).  dsize = (width, height).  background, return_cover, as_tensor: as in
    ``warp_by_map``."""
    Hs, Ws, C = check_image(img, 'img')
    if len(dsize) != 2 or int(dsize[0]) != dsize[0] or int(dsize[1]) != dsize[1]:
        raise ValueError(f'dsize must be (width, height), got {dsize}')
    Wd, Hd = int(dsize[0]), int(dsize[1])
    if not (1 <= Hd <= MAX_SIDE and 1 <= Wd <= MAX_SIDE):
        raise ValueError(f'dsize: width and height must be in [1, {MAX_SIDE}], got {Wd} x {Hd}')
    _check_background(background, Hd, Wd, C, len(img.shape))
    Minv = np.ascontiguousarray(_matrix(M) if inverse_map else invert_perspective(M))
    device = _pick_device(img, background)
    src = on(img, device)
    bg = None if background is None else on(background, device)
    dst = torch.empty((Hd, Wd, C), dtype=torch.uint8, device=device)
    cover = torch.empty((Hd, Wd), dtype=torch.uint8, device=device) if return_cover else None
    with torch.cuda.device(device):
        check_op(_lib.load_library().cotr_warp_perspective(ptr(src), Hs, Ws, C, Minv.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                           Hd, Wd, ptr(dst), ptr(cover), ptr(bg), _lib.current_stream_ptr()),
                 'cotr_warp_perspective')
    return _finish(dst, cover, len(img.shape), return_cover, as_tensor)


def get_perspective_transform(src, dst):
    """``cv2.getPerspectiveTransform(src, dst)``: the float64 3 x 3 M with M[2, 2] = 1 that maps the four points src [4, 2]
    onto dst [4, 2], from cv2's 8 x 8 linear system solved with ``numpy.linalg.solve`` (cv2 uses its own decomposition: the
    last bits of M may differ).  Degenerate points (three on a line): ValueError."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    if src.shape != (4, 2) or dst.shape != (4, 2):
        raise ValueError(f'src and dst must be [4, 2], got {src.shape} and {dst.shape}')
    if not (np.isfinite(src).all() and np.isfinite(dst).all()):
        raise ValueError('src and dst must be finite')
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        (x, y), (u, v) = src[i], dst[i]
        A[i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        A[i + 4] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[i], b[i + 4] = u, v
    try:
        h = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        h = None
    if h is None or not np.isfinite(h).all():
        raise ValueError('the four point pairs do not determine a perspective transform (singular system)')
    return np.append(h, 1.0).reshape(3, 3)


def picture_corners(picture_shape):
    """``rep_coord`` of demo_homography.py:41: the picture's corners (x, y) in the order left-upper, right-upper,
    left-bottom, right-bottom, at (0, 0), (W, 0), (0, H), (W, H)"""
    H, W = picture_shape[:2]
    return np.array([[0, 0], [W, 0], [0, H], [W, H]], dtype=np.float32)


def paste_by_corners(picture, corners_b, img_b, as_tensor=False):
    """demo_homography.py:41,46-49: paste ``picture`` into ``img_b`` through its four corners.  corners_b [4, 2]: where the
    picture's corners (``picture_corners``: lu, ru, lb, rb) land in ``img_b``, e.g. ``corrs[:, 2:]`` of the demo; rounded to
    float32 as the demo does.  One ``cotr_warp_perspective`` launch with ``img_b`` as the background -> uint8, ``img_b``'s
    shape: the warped picture where it covers, ``img_b`` elsewhere."""
    check_image(picture, 'picture')
    Hb, Wb, _ = check_image(img_b, 'img_b')
    corners_b = np.asarray(corners_b.cpu() if torch.is_tensor(corners_b) else corners_b)
    if corners_b.shape != (4, 2):
        raise ValueError(f'corners_b must be [4, 2], got {corners_b.shape}')
    T = get_perspective_transform(picture_corners(picture.shape), corners_b.astype(np.float32))
    return warp_perspective(picture, T, (Wb, Hb), background=img_b, as_tensor=as_tensor)


def warp_by_corr(img_a, img_b, corrs, alpha=0.5, as_tensor=False, simplices=None):
    """demo_single_pair.py:42-44: ``triangulate_corr`` of the correspondences, ``img_b`` warped by that map onto A, and the
    blend with ``img_a`` -> (overlay float32 [H_a, W_a, 3] = warped / 255 * alpha + img_a / 255 * (1 - alpha), warped uint8
    [H_a, W_a, 3]).  The dense map stays on the device.  Outside the correspondences' hull the map is 0, so ``warped``
    reads ``img_b`` at (0, 0) there, exactly as the demo's cv2 call does.  simplices: as in ``triangulate_corr``; with 'device', device tensors for the images
    and ``corrs`` and as_tensor=True nothing passes through the host, and the call can be captured into a graph."""
    check_image(img_a, 'img_a')
    check_image(img_b, 'img_b')
    device = _pick_device(img_a, img_b)
    with torch.cuda.device(device):
        dense = triangulate_corr(corrs, img_a.shape, img_b.shape, simplices=simplices, as_tensor=True)
        warped = warp_by_map(on(img_b, device), dense, as_tensor=True)
        a = on(img_a, device)
        a = a if a.dim() == 3 else a[..., None]
        w = warped if warped.dim() == 3 else warped[..., None]
        overlay = (w.double() / 255 * alpha + a.double() / 255 * (1 - alpha)).float()   # the demo's float64 expression, rounded once
    if as_tensor:
        return overlay, warped
    return overlay.cpu().numpy(), warped.cpu().numpy()
