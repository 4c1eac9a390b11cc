"""Keypoints of photographs, on the device: the first link of photographs + intrinsics -> keypoints -> mutual matches -> tracks
-> poses (``mutual_matches``, ``build_tracks``, ``ZoomEngine.guided_match`` and ``ZoomEngine.reconstruct_keypoints`` all consume
keypoints).

``detect_keypoints_tensors`` is one ``cotr_detect_keypoints`` call (cotr_amd/csrc/keypoints.hip, rules in DESIGN.md 3h-22) on the
current device and stream: a corner score ('min_eig' or 'harris') on the integer structure tensor of 8-bit grey images,
non-maximum suppression over a (2 nms_radius + 1)^2 window under a total order on (score, pixel index), a quality test against
the image's best score, the best ``max_keypoints`` by rank, and a sub-pixel position per axis.  The result is defined exactly:
the same images give the same bits.  ``detect_keypoints`` is the host form, one [k, 2] array per image.  No CPU fallback."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args
from ._args import F64, I32
from .depth import to_grey

SCORES = ('min_eig', 'harris')
MAX_IMAGES = 64
MAX_WINDOW = 4
MAX_NMS = 8
MAX_KEYPOINTS = 65536
MAX_PIXELS = 1 << 28
MAX_SIDE = 1 << 20
_SUBJECT = 'the keypoints are detected'


def _check_scalars(max_keypoints, score, window_radius, nms_radius, border, quality, min_score):
    if score not in SCORES:
        raise ValueError(f'score must be one of {SCORES}, got {score!r}')
    _args.check_int_range('max_keypoints', max_keypoints, 1, MAX_KEYPOINTS)
    _args.check_int_range('window_radius', window_radius, 1, MAX_WINDOW)
    _args.check_int_range('nms_radius', nms_radius, 1, MAX_NMS)
    _args.check_int_range('border', border, 0, 1 << 20)
    _args.check_int_range('quality', quality, 0.0, 1.0, integer=False)
    if np.isnan(min_score):
        raise ValueError('min_score must not be NaN')


def _check_shape(n, H, W, window_radius, border):
    if not 1 <= n <= MAX_IMAGES:
        raise ValueError(f'between 1 and {MAX_IMAGES} images in one call, got {n}')
    least = 2 * max(int(border), int(window_radius) + 1) + 1
    if H < least or W < least:
        raise ValueError(f'images must be at least 2 max(border, window_radius + 1) + 1 = {least} pixels high and wide, got {H} x {W}')
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f'images must be at most 2^20 pixels high and wide, got {H} x {W}')
    if n * H * W > MAX_PIXELS:
        raise ValueError(f'at most 2^28 pixels in one call, got {n} x {H} x {W}')


def _grey_batch(images):
    """uint8 [n,H,W], [H,W], or RGB [...,3] -> uint8 device tensor [n,H,W] (``to_grey``'s rule, and its refusals)"""
    g = to_grey(images)
    if g.dim() == 2:
        g = g[None]
    if g.dim() != 3:
        raise ValueError(f'images must be uint8 [n, H, W], [H, W], or RGB [..., 3], got shape {tuple(g.shape)} after to_grey')
    return g.contiguous()


def detect_keypoints_tensors(images, mask=None, max_keypoints=2048, score='min_eig', window_radius=2, nms_radius=4, border=0, quality=0.01,
                             min_score=0.0, device=None):
    """One ``cotr_detect_keypoints`` call on the current stream.  ``images``: uint8 [n,H,W], [H,W], or RGB
    [...,3] (through ``to_grey``), arrays or device tensors; ``mask``: [n,H,W] or [H,W], 0 where no keypoint may lie, or None
    -> dict of device tensors: keypoints float64 [n,K,2] (x, y; integer pixel indices are pixel coordinates), scores float64
    [n,K], pixel int32 [n,K] (the raster index y W + x), info int32 [n,4] = (candidates, survivors of the quality test,
    keypoints written, 0), K = ``max_keypoints``.  Rows from info[:,2] on are NaN / NaN / -1.  ``score``: 'min_eig' (twice the
    smaller eigenvalue of the structure tensor over the (2 window_radius + 1)^2 box) or 'harris' (k = 3/64); a keypoint is the
    strict best of its (2 nms_radius + 1)^2 window (ties go to the smaller pixel index), at least max(border, window_radius
    + 1) pixels from every edge, with a score of at least ``min_score`` and ``quality`` times the image's best; the best K are
    written in order of score."""
    _check_scalars(max_keypoints, score, window_radius, nms_radius, border, quality, min_score)
    _args.no_cpu_tensors(_SUBJECT, images, mask)
    if device is None and torch.is_tensor(images):
        device = images.device
    device = _args.device(device)
    with torch.cuda.device(device):
        g = on(_grey_batch(images), device)
        n, H, W = (int(v) for v in g.shape)
        _check_shape(n, H, W, window_radius, border)
        m = None
        if mask is not None:
            m = _args.tensor(mask, None)
            if m.dim() == 2:
                m = m[None]
            if tuple(m.shape) != (n, H, W):
                raise ValueError(f'mask must be [n, H, W] = [{n}, {H}, {W}], got shape {tuple(m.shape)}')
            m = _args.mask_u8(m, (n, H, W), device).contiguous()
        lib, K = _lib.load_library(), int(max_keypoints)
        work, _ = _args.scratch(lib, 'cotr_detect_keypoints_work_bytes', n, H, W, int(nms_radius), device=device)
        xy, scores, pixel, info = _args.empty(device, ((n, K, 2), F64), ((n, K), F64), ((n, K), I32), ((n, 4), I32))
        check_op(lib.cotr_detect_keypoints(ptr(g), ptr(m), n, H, W, SCORES.index(score), int(window_radius), int(nms_radius), int(border),
                                           ctypes.c_double(quality), ctypes.c_double(min_score), K, ptr(xy), ptr(scores), ptr(pixel), ptr(info),
                                           ptr(work), _lib.current_stream_ptr()), 'cotr_detect_keypoints')
    return dict(keypoints=xy, scores=scores, pixel=pixel, info=info)


def _is_image(x):
    """one image ([H,W] or RGB [H,W,3]) rather than a batch or a list"""
    return hasattr(x, 'shape') and (len(x.shape) == 2 or (len(x.shape) == 3 and x.shape[-1] == 3))


def group_by_size(shapes):
    """the shapes of the images ((H, W) or (H, W, 3): grey and RGB are not stacked together) -> {shape: [indices in input
    order]}, the shapes in order of first appearance"""
    groups = {}
    for i, s in enumerate(shapes):
        groups.setdefault(tuple(int(v) for v in s), []).append(i)
    return groups


def detect_keypoints(image_or_list, **kw):
    """The host form: one image ([H,W] or RGB [H,W,3]) -> one float64 [k,2] array of (x, y), trimmed to the keypoints written; a
    list of images, or a batch [n,H,W] / [n,H,W,3] -> a list of such arrays in input order.  Images of a list may differ in size:
    they are grouped by size, one ``detect_keypoints_tensors`` call per size (and per 64 images of it).  ``kw``: its arguments;
    a ``mask`` is one mask for a single image, else a list or batch with one mask per image."""
    single = _is_image(image_or_list)
    imgs = [image_or_list] if single else list(image_or_list)
    if not imgs:
        raise ValueError('detect_keypoints needs at least one image')
    if any(not _is_image(im) for im in imgs):
        raise ValueError('every image must be [H, W] or RGB [H, W, 3]')
    masks = kw.pop('mask', None)
    if masks is not None:
        masks = [masks] if single else list(masks)
        if len(masks) != len(imgs):
            raise ValueError(f'mask must hold one mask per image ({len(imgs)}), got {len(masks)}')
    stack = lambda xs: torch.stack(list(xs)) if torch.is_tensor(xs[0]) else np.stack([np.asarray(x) for x in xs])   # noqa: E731
    out = [None] * len(imgs)
    for idx in group_by_size([im.shape for im in imgs]).values():
        for lo in range(0, len(idx), MAX_IMAGES):
            part = idx[lo:lo + MAX_IMAGES]
            r = detect_keypoints_tensors(stack([imgs[i] for i in part]), mask=None if masks is None else stack([masks[i] for i in part]), **kw)
            xy, count = r['keypoints'].cpu().numpy(), r['info'][:, 2].cpu().numpy()
            for row, i in enumerate(part):
                out[i] = xy[row, :int(count[row])].copy()
    return out[0] if single else out
