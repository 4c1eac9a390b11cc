"""Multi-view depth maps on the device: the step between dense correspondences and the TSDF stack.

``depth_from_corr`` is one ``cotr_corr_depth`` call of cotr_amd/csrc/mvdepth.hip: the correspondence maps of a reference view
into 1 to 31 posed neighbours (``ZoomEngine.flow`` through ``flow_to_corr``, or ``triangulate_corr``) become the reference's
depth map - per pixel one scalar along a known ray, voted on over the neighbours and refitted on the reprojection error.
``filter_depths`` is one ``cotr_depth_consistency`` call: 2 to 32 depth maps of one size are checked against each other (the
geometric-consistency step of multi-view stereo), ``filter_captures`` the same on ``cotr_amd.data.Capture``.
``ZoomEngine.depth_map`` and ``ZoomEngine.fuse_images`` run them behind the engine's correspondences and in front of
``fuse_captures``.  ``refine_depth_photo`` is one ``cotr_photo_depth`` call of cotr_amd/csrc/photodepth.hip: a depth map is
checked against the pixels it describes - a few depth hypotheses around each pixel's depth, the one kept at which the patches of
the posed neighbour images (``to_grey``) look most like the reference's; ``refine_captures_photo`` the same on captures.  The
rules are the library's own.  No CPU fallback."""
import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args
from ._args import I32, U8

MAX_VIEWS = _args.MAX_VIEWS
MAX_PIXELS = 1 << 28
MAX_REFINE = 64
MAX_RADIUS, MAX_STEPS, MAX_SWEEPS = 4, 16, 8
F32 = torch.float32


def _check_depth_args(threshold, min_angle, distance_thresh, min_views, refine_iters, centres):
    _args.check_positive('threshold', threshold)
    _args.check_sq_float32(threshold)
    if not 0 <= min_angle <= 180:
        raise ValueError(f'min_angle must be in [0, 180] degrees, got {min_angle}')
    _args.check_distance(distance_thresh)
    _args.check_int_range('min_views', min_views, 1, MAX_VIEWS - 1)
    _args.check_int_range('refine_iters', refine_iters, 0, MAX_REFINE)
    if not np.isfinite(centres):
        raise ValueError(f'centres must be finite, got {centres}')


def _w2c_rows(c2ws):
    """host camera-to-world [V,4,4] -> world-to-camera rows [V,12]: [R^T | -R^T t] of each rigid pose"""
    rows = []
    for m in c2ws:
        R, t = m[:3, :3], m[:3, 3]
        rows.append(np.concatenate([R.T, -(R.T @ t)[:, None]], axis=1).reshape(12))
    return np.stack(rows)


def reference_camera(K_ref, centres=0.0):
    """The camera under which a map sampled at x + ``centres`` sits at integer pixels: ``K_ref`` with cx and cy moved by -``centres``
    -> float64 [3,3] on the host.  What ``depth_from_corr`` computes with and returns as K."""
    k = np.array(_args.camera(K_ref, 'K_ref'), dtype=np.float64).reshape(3, 3)
    if not np.isfinite(centres):
        raise ValueError(f'centres must be finite, got {centres}')
    k[0, 2] -= float(centres)
    k[1, 2] -= float(centres)
    return k


def _enqueue_corr_depth(lib, corr, valid, cams, poses, found, threshold, max_cos, distance_thresh, min_views, refine_iters):
    """every tensor on the device of ``corr`` already, every argument checked -> the dict of ``depth_from_corr`` without K"""
    K, H, W = (int(v) for v in corr.shape[:3])
    depth, views, err, info = _args.empty(corr.device, ((H, W), F32), ((H, W), U8), ((H, W), F32), (8, I32))
    check_op(lib.cotr_corr_depth(ptr(corr), ptr(valid), ptr(cams), ptr(poses), K + 1, H, W, ptr(found), float(threshold), float(max_cos),
                                 float(distance_thresh), int(min_views), int(refine_iters), ptr(depth), ptr(views), ptr(err), ptr(info),
                                 _lib.current_stream_ptr()), 'cotr_corr_depth')
    return dict(depth=depth, views=views, err=err, mask=depth > 0, info=info)


def depth_from_corr(corr_maps, K_ref, c2w_ref, Ks, c2ws, valid=None, threshold=2.0, min_angle=1.5, distance_thresh=50.0, min_views=1,
                    refine_iters=10, centres=0.0, found=None, device=None):
    """One ``cotr_corr_depth`` call on the current stream: the depth map of a reference view (camera ``K_ref`` [3,3], pose
    ``c2w_ref`` [4,4] camera-to-world, both host) from ``corr_maps`` [K,H,W,2] (float32, or float64 that is rounded to it; a device
    tensor is read in place), whose entry [k, y, x] is the position (u, v) in pixels of neighbour k (``Ks`` [K,3,3] or one [3,3],
    ``c2ws`` [K,4,4], host; 1 <= K <= 31) of what the reference shows at pixel (x, y).  ``valid`` [K,H,W]: entries that are 0 take no
    part.  Per pixel the neighbours whose ray stands at least ``min_angle`` degrees off the reference ray each propose a depth;
    the first proposal that the most neighbours agree with within ``threshold`` pixels wins, is refitted on their summed squared
    reprojection error by up to ``refine_iters`` Gauss-Newton steps, and is kept when it has ``min_views`` agreeing neighbours,
    lies in (0, ``distance_thresh``) and every one of them still agrees.  ``centres``: 0.0 for maps sampled at integer pixels
    (``flow_to_corr``); 0.5 for maps sampled at pixel centres x + 0.5 (``triangulate_corr``): cx and cy of ``K_ref`` are then
    moved by -0.5.  ``found`` int [1]: 0 empties the result.
    -> dict: depth float32 [H,W] (0: none), views uint8 [H,W] (agreeing neighbours), err float32 [H,W] (their mean squared
    reprojection error, NaN: none), mask bool [H,W], info int32 [8] = (found, pixels with a depth, with too few views, without a
    candidate, dropped by depth, dropped by error, 0, steps kept) - device tensors - and K float64 [3,3] on the host: the camera
    under which depth[y, x] sits at the integer pixel (x, y), the convention of ``lift_pixels`` and the TSDF volume."""
    shape = tuple(corr_maps.shape) if hasattr(corr_maps, 'shape') else np.shape(corr_maps)
    if len(shape) != 4 or shape[3] != 2 or shape[1] < 1 or shape[2] < 1:
        raise ValueError(f'corr_maps must be [K, H, W, 2], got shape {shape}')
    K, H, W = (int(v) for v in shape[:3])
    if not 1 <= K <= MAX_VIEWS - 1:
        raise ValueError(f'between 1 and {MAX_VIEWS - 1} neighbour maps, got {K}')
    if H * W > MAX_PIXELS:
        raise ValueError(f'corr_maps: at most 2^28 pixels, got {H} x {W}')
    if not torch.is_tensor(corr_maps):
        corr_maps = np.asarray(corr_maps)
    if corr_maps.dtype not in (torch.float32, torch.float64, np.float32, np.float64):
        raise ValueError(f'corr_maps must be float32 or float64, got {corr_maps.dtype}')
    k_ref = reference_camera(K_ref, centres)
    ks, _ = _args.cameras(Ks, K)
    ref = _args.pose_matrix(c2w_ref)
    if ref is None:
        raise ValueError('c2w_ref must be a finite [4, 4] matrix, got None')
    rows = _args.c2w_rows(c2ws.cpu() if torch.is_tensor(c2ws) else c2ws, K).numpy().reshape(K, 4, 4)
    _check_depth_args(threshold, min_angle, distance_thresh, min_views, refine_iters, centres)
    if valid is not None and tuple(valid.shape) != (K, H, W):
        raise ValueError(f'valid must be [K, H, W] = [{K}, {H}, {W}], got shape {tuple(valid.shape)}')
    if found is not None and int(np.prod(tuple(np.shape(found) if not torch.is_tensor(found) else found.shape))) != 1:
        raise ValueError('found must be [1]')
    _args.no_cpu_tensors('the depth maps run', corr_maps, valid, found)
    all_k = np.stack([k_ref] + [np.array(k, dtype=np.float64).reshape(3, 3) for k in ks])
    cams = np.stack([all_k[:, 0, 0], all_k[:, 1, 1], all_k[:, 0, 2], all_k[:, 1, 2], all_k[:, 0, 1]], axis=1)
    poses = _w2c_rows(np.concatenate([ref[None], rows]))
    device = _args.device(device)
    with torch.cuda.device(device):
        corr = on(_args.tensor(corr_maps, None), device, 8).to(F32).contiguous()
        out = _enqueue_corr_depth(_lib.load_library(), corr, _args.mask_u8(valid, (K, H, W), device), on(cams, device), on(poses, device),
                                  _args.found_i32(found, device), threshold, float(np.cos(np.deg2rad(float(min_angle)))), distance_thresh,
                                  min_views, refine_iters)
    out['K'] = k_ref
    return out


def flow_to_corr(corr, con, shape_b, max_cycle):
    """``ZoomEngine.flow``'s normalised map ``corr`` [H,W,2] (x, y in [-1, 1] over image B, the convention of ``grid_sample`` with
    align_corners=False) and its cycle error ``con`` [H,W] -> (pixel positions float32 [H,W,2]: u = ((g_x + 1) W_b - 1) / 2, v =
    ((g_y + 1) H_b - 1) / 2, validity bool [H,W]: con <= max_cycle), arrays for arrays and tensors for tensors.  ``shape_b``: B's
    image shape (H_b, W_b, ...)."""
    Hb, Wb = int(shape_b[0]), int(shape_b[1])
    if len(corr.shape) != 3 or corr.shape[2] != 2 or tuple(con.shape) != tuple(corr.shape[:2]):
        raise ValueError(f'corr must be [H, W, 2] and con [H, W], got shapes {tuple(corr.shape)} and {tuple(con.shape)}')
    if Hb < 1 or Wb < 1:
        raise ValueError(f'shape_b must be (H, W) of at least 1 x 1, got {tuple(shape_b)}')
    if not max_cycle >= 0:
        raise ValueError(f'max_cycle must be >= 0, got {max_cycle}')
    if torch.is_tensor(corr):
        g = corr.double()
        px = torch.stack([((g[..., 0] + 1.0) * Wb - 1.0) / 2.0, ((g[..., 1] + 1.0) * Hb - 1.0) / 2.0], dim=-1).float()
        return px, torch.as_tensor(con, device=corr.device) <= float(max_cycle)
    g = np.asarray(corr, dtype=np.float64)
    px = np.stack([((g[..., 0] + 1.0) * Wb - 1.0) / 2.0, ((g[..., 1] + 1.0) * Hb - 1.0) / 2.0], axis=-1).astype(np.float32)
    return px, np.asarray(con) <= float(max_cycle)


def _check_filter_args(px_thresh, rel_thresh, min_views, max_violations):
    _args.check_positive('px_thresh', px_thresh)
    if not np.isfinite(float(px_thresh) * float(px_thresh)):
        raise ValueError(f'px_thresh must have a finite square, got {px_thresh}')
    if not 0 < rel_thresh < 1:
        raise ValueError(f'rel_thresh must be in (0, 1), got {rel_thresh}')
    _args.check_int_range('min_views', min_views, 0, MAX_VIEWS - 1)
    _args.check_int_range('max_violations', max_violations, -1, MAX_VIEWS - 1)


def _check_stack(depths):
    """the size rules of a stack of n depth maps -> n"""
    if len(depths.shape) != 3 or depths.shape[0] < 1:
        raise ValueError(f'depths must be [n, H, W], got shape {tuple(depths.shape)}')
    _args.check_depth(depths[0])
    n, H, W = (int(v) for v in depths.shape)
    if not 2 <= n <= MAX_VIEWS:
        raise ValueError(f'between 2 and {MAX_VIEWS} depth maps, got {n}')
    if n * H * W > MAX_PIXELS:
        raise ValueError(f'depth maps: at most 2^28 pixels in all, got {n} x {H} x {W}')
    return n


def _enqueue_consistency(lib, depths, K, rows, found, pairs, px_thresh, rel_thresh, min_views, max_violations):
    """every tensor on the device of ``depths`` already, every argument checked -> the dict of ``filter_depths``"""
    n, H, W = (int(v) for v in depths.shape)
    depth, count, info = _args.empty(depths.device, ((n, H, W), F32), ((n, H, W), U8), ((n, 4), I32))
    check_op(lib.cotr_depth_consistency(ptr(depths), n, H, W, K, ptr(rows), ptr(found), ptr(pairs), float(px_thresh), float(rel_thresh),
                                        int(min_views), int(max_violations), ptr(depth), ptr(count), ptr(info), _lib.current_stream_ptr()),
             'cotr_depth_consistency')
    return dict(depth=depth, count=count, info=info)


def filter_depths(depths, Ks, c2ws, pairs=None, px_thresh=1.0, rel_thresh=0.01, min_views=2, max_violations=-1, found=None, device=None):
    """One ``cotr_depth_consistency`` call on the current stream: the depth maps ``depths`` float32 [n,H,W] (2 <= n <= 32; a device
    tensor is read in place) with the cameras ``Ks`` [n,3,3] or one [3,3] (host) and the camera-to-world poses ``c2ws`` [n,4,4]
    (float64; a device tensor is read in place) checked against each other.  A pixel of view i with a depth is lifted into the
    world and projected into every other view j; the depth j holds there is lifted and projected back.  j is consistent when the
    point returns within ``px_thresh`` pixels and ``rel_thresh`` (relative) of the depth it left with, and a violation when it is
    not and j's depth lies behind the point by more than ``rel_thresh``: j sees through it.  A pixel is kept with at least
    ``min_views`` consistent views and (``max_violations`` >= 0) at most that many violations, and takes the mean of its own and
    the returned depths.  ``pairs`` [n,n]: row i names the views j (entries that are not 0) it is checked against; None: all.
    ``found`` int [n]: a view whose entry is 0 is neither checked nor checked against.
    -> dict of device tensors: depth float32 [n,H,W] (0: dropped), count uint8 [n,H,W] (consistent views), info int32 [n,4] =
    (evaluated, valid pixels in, kept, dropped by violations)."""
    if not torch.is_tensor(depths):
        depths = np.asarray(depths)
    n = _check_stack(depths)
    _, K = _args.cameras(Ks, n)
    rows = _args.c2w_rows(c2ws, n)
    _check_filter_args(px_thresh, rel_thresh, min_views, max_violations)
    if pairs is not None and tuple(pairs.shape) != (n, n):
        raise ValueError(f'pairs must be [n, n] = [{n}, {n}], got shape {tuple(pairs.shape)}')
    if found is not None and not torch.is_tensor(found):
        found = np.asarray(found)
    if found is not None and int(np.prod(tuple(found.shape))) != n:
        raise ValueError(f'found must be [{n}], got shape {tuple(found.shape)}')
    _args.no_cpu_tensors('the depth maps run', depths, c2ws, pairs, found)
    device = _args.device(device)
    with torch.cuda.device(device):
        return _enqueue_consistency(_lib.load_library(), on(_args.tensor(depths, np.float32), device).contiguous(), K, on(rows, device).contiguous(),
                                    _args.found_i32(found, device), _args.mask_u8(pairs, (n, n), device), px_thresh, rel_thresh, min_views,
                                    max_violations)


def filter_captures(caps, pairs=None, min_overlap=None, **kw):
    """``filter_depths`` on the posed captures ``caps`` (``cotr_amd.data.Capture`` of one depth-map size) -> (the captures with
    their depth replaced by the filtered map, a device tensor; the dict of ``filter_depths``).  ``pairs`` [n,n]: which view is
    checked against which; with ``min_overlap`` instead, the cells of ``overlap_matrix`` of the captures above it, chosen on the
    device.  ``kw``: px_thresh, rel_thresh, min_views, max_violations, found, device."""
    caps = list(caps)
    if len(caps) < 2:
        raise ValueError(f'filter_captures needs at least two captures, got {len(caps)}')
    shapes = {tuple(cap.depth.shape) for cap in caps}
    if len(shapes) != 1:
        raise ValueError(f'the captures must share one depth-map size, got {sorted(shapes)}')
    if pairs is not None and min_overlap is not None:
        raise ValueError('give pairs or min_overlap, not both')
    for cap in caps:
        _args.check_depth(cap.depth)
        if _args.pose_matrix(cap.c2w) is None:
            raise ValueError('c2w must be a finite [4, 4] matrix, got None')
    _check_filter_args(kw.get('px_thresh', 1.0), kw.get('rel_thresh', 0.01), kw.get('min_views', 2), kw.get('max_violations', -1))
    _args.no_cpu_tensors('the depth maps run', *[cap.depth for cap in caps])
    if min_overlap is not None:
        from ..scene import overlap_matrix
        dist = overlap_matrix(caps)
        pairs = (dist > float(min_overlap)).to(U8)
        kw.setdefault('device', pairs.device)
    device = _args.device(kw.pop('device', None))
    depths = torch.stack([on(_args.tensor(cap.depth, np.float32), device) for cap in caps])
    Ks = np.stack([np.asarray(cap.K.cpu() if torch.is_tensor(cap.K) else cap.K, dtype=np.float64) for cap in caps])
    r = filter_depths(depths, Ks, [cap.c2w for cap in caps], pairs=pairs, device=device, **kw)
    return [cap._replace(depth=r['depth'][i]) for i, cap in enumerate(caps)], r


# ---- the photometric refinement -------------------------------------------------------------------------------------------------
def to_grey(images):
    """uint8 [..., H, W, 3] (RGB) or uint8 [..., H, W] (grey already: passed through), array or device tensor -> uint8 device tensor
    [..., H, W] by the integer rule (77 R + 150 G + 29 B + 128) >> 8.  A last axis of 3 behind at least two others is the colour."""
    if not torch.is_tensor(images):
        images = np.asarray(images)
    if images.dtype not in (torch.uint8, np.uint8):
        raise ValueError(f'images must be uint8, got {images.dtype}')
    if len(images.shape) < 2:
        raise ValueError(f'images must be [..., H, W, 3] or [..., H, W], got shape {tuple(images.shape)}')
    _args.no_cpu_tensors('the depth maps run', images)
    t = on(images, _args.device(images.device if torch.is_tensor(images) else None))
    return grey_rule(t) if t.dim() >= 3 and t.shape[-1] == 3 else t


def grey_rule(rgb):
    """uint8 tensor [..., 3] -> uint8 [...]: (77 R + 150 G + 29 B + 128) >> 8, where the tensor is"""
    c = rgb.to(I32)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).to(U8)


def _check_photo_args(radius, steps, sweeps, rel_step, min_var, min_score, min_views, distance_thresh, K):
    _args.check_int_range('radius', radius, 1, MAX_RADIUS)
    _args.check_int_range('steps', steps, 1, MAX_STEPS)
    _args.check_int_range('sweeps', sweeps, 1, MAX_SWEEPS)
    _args.check_positive('rel_step', rel_step)
    if not int(steps) * float(rel_step) < 1:
        raise ValueError(f'steps * rel_step must be < 1, got {steps} * {rel_step}')
    _args.check_positive('min_var', min_var)
    if not -1 <= min_score <= 1:
        raise ValueError(f'min_score must be in [-1, 1], got {min_score}')
    _args.check_int_range('min_views', min_views, 1, K)
    _args.check_distance(distance_thresh)


def _enqueue_photo_depth(lib, grey, depth, cams, poses, found, radius, steps, sweeps, rel_step, min_var, min_score, min_views, distance_thresh,
                         keep_input):
    """every tensor on the device of ``grey`` already, every argument checked -> the dict of ``refine_depth_photo``"""
    V, H, W = (int(v) for v in grey.shape)
    out, score, views, info = _args.empty(grey.device, ((H, W), F32), ((H, W), F32), ((H, W), U8), (8, I32))
    check_op(lib.cotr_photo_depth(ptr(grey), ptr(depth), ptr(cams), ptr(poses), V, H, W, ptr(found), int(radius), int(steps), int(sweeps),
                                  float(rel_step), float(min_var), float(min_score), int(min_views), float(distance_thresh),
                                  1 if keep_input else 0, ptr(out), ptr(score), ptr(views), ptr(info), _lib.current_stream_ptr()),
             'cotr_photo_depth')
    return dict(depth=out, score=score, views=views, mask=views > 0, info=info)


def refine_depth_photo(depth, img_ref, imgs, K_ref, c2w_ref, Ks, c2ws, radius=2, steps=4, sweeps=3, rel_step=0.004, min_var=4.0,
                       min_score=0.5, min_views=1, distance_thresh=50.0, keep_input=True, found=None, device=None):
    """One ``cotr_photo_depth`` call on the current stream: the depth map ``depth`` float32 [H,W] of a reference view (image
    ``img_ref``, camera ``K_ref`` [3,3] under which depth[y, x] sits at the integer pixel (x, y) - the K that ``depth_from_corr``
    returns - and pose ``c2w_ref`` [4,4] camera-to-world, both host) refined on the images ``imgs`` of 1 to 31 posed neighbours
    (``Ks`` [K,3,3] or one [3,3], ``c2ws`` [K,4,4], host).  The images, uint8 [H,W,3] or grey [H,W] of the depth map's size, go
    through ``to_grey``; arrays or device tensors.  Per pixel with a depth, ``sweeps`` sweeps of 2 ``steps`` + 1 depths around the
    current one, ``rel_step`` (relative) apart in the first sweep and half as far in each one after: at each depth the
    (2 ``radius`` + 1)^2 patch, fronto-parallel at that depth, is sampled in every neighbour and scored by its zero-mean
    normalised cross-correlation with the reference's; the depth with the best mean score over the neighbours that see the whole
    patch (at least ``min_views`` of them, each with a patch variance of at least ``min_var``) wins, moved by a parabola through
    its two neighbours.  The result is kept when the last sweep's score is at least ``min_score`` and the depth lies in (0,
    ``distance_thresh``).  Pixels on the image's rim of ``radius`` pixels, pixels whose own patch has a variance below ``min_var``
    and pixels not kept hold the depth they came with (``keep_input``) or 0.  ``found`` int [1]: 0 empties the result.
    -> dict of device tensors: depth float32 [H,W], score float32 [H,W] (NaN: not refined), views uint8 [H,W] (scoring
    neighbours, 0: not refined), mask bool [H,W] (refined), info int32 [8] = (found, refined, without an input depth, rim, flat,
    nothing scored, below min_score, dropped by range)."""
    if not torch.is_tensor(depth):
        depth = np.asarray(depth)
    _args.check_depth(depth)
    H, W = (int(v) for v in depth.shape)
    imgs = list(imgs)
    K = len(imgs)
    if not 1 <= K <= MAX_VIEWS - 1:
        raise ValueError(f'between 1 and {MAX_VIEWS - 1} neighbour images, got {K}')
    for name, img in [('img_ref', img_ref)] + [(f'imgs[{k}]', img) for k, img in enumerate(imgs)]:
        shape = tuple(img.shape) if hasattr(img, 'shape') else np.shape(img)
        if shape not in ((H, W), (H, W, 3)):
            raise ValueError(f'{name} must be [{H}, {W}, 3] or [{H}, {W}], the size of the depth map, got shape {shape}')
        if getattr(img, 'dtype', None) not in (torch.uint8, np.uint8):
            raise ValueError(f'{name} must be uint8, got {getattr(img, "dtype", type(img))}')
    k_ref = reference_camera(K_ref)
    ks, _ = _args.cameras(Ks, K)
    ref = _args.pose_matrix(c2w_ref)
    if ref is None:
        raise ValueError('c2w_ref must be a finite [4, 4] matrix, got None')
    rows = _args.c2w_rows(c2ws.cpu() if torch.is_tensor(c2ws) else c2ws, K).numpy().reshape(K, 4, 4)
    _check_photo_args(radius, steps, sweeps, rel_step, min_var, min_score, min_views, distance_thresh, K)
    if found is not None and int(np.prod(tuple(np.shape(found) if not torch.is_tensor(found) else found.shape))) != 1:
        raise ValueError('found must be [1]')
    _args.no_cpu_tensors('the depth maps run', depth, img_ref, found, *imgs)
    all_k = np.stack([k_ref] + [np.array(k, dtype=np.float64).reshape(3, 3) for k in ks])
    cams = np.stack([all_k[:, 0, 0], all_k[:, 1, 1], all_k[:, 0, 2], all_k[:, 1, 2], all_k[:, 0, 1]], axis=1)
    poses = _w2c_rows(np.concatenate([ref[None], rows]))
    device = _args.device(device)
    with torch.cuda.device(device):
        grey = torch.stack([to_grey(on(img, device)) for img in [img_ref] + imgs])
        return _enqueue_photo_depth(_lib.load_library(), grey, on(_args.tensor(depth, np.float32), device), on(cams, device), on(poses, device),
                                    _args.found_i32(found, device), radius, steps, sweeps, rel_step, min_var, min_score, min_views,
                                    distance_thresh, keep_input)


def nearest_views(c2ws, i, neighbours):
    """the ``neighbours`` views whose camera centres are nearest that of view i, the nearer first (the lower index among equals)"""
    centres = np.asarray(c2ws, dtype=np.float64)[:, :3, 3]
    d = np.linalg.norm(centres - centres[i], axis=1)
    d[i] = np.inf
    return [int(j) for j in np.argsort(d, kind='stable')[:int(neighbours)]]


def refine_captures_photo(caps, neighbours=2, **kw):
    """``refine_depth_photo`` on every one of the posed captures ``caps`` (``cotr_amd.data.Capture`` of one size, each with an
    image) against the ``neighbours`` captures whose camera centres are nearest its own, the choice of ``ZoomEngine.fuse_images``
    -> (the captures with their depth replaced by the refined map, a device tensor; the list of ``refine_depth_photo``'s dicts).
    ``kw``: the other arguments of ``refine_depth_photo``."""
    caps = list(caps)
    n = len(caps)
    if n < 2:
        raise ValueError(f'refine_captures_photo needs at least two captures, got {n}')
    _args.check_int_range('neighbours', neighbours, 1, min(n - 1, MAX_VIEWS - 1))
    if any(cap.image is None for cap in caps):
        raise ValueError('every capture needs an image')
    shapes = {tuple(cap.depth.shape) for cap in caps}
    if len(shapes) != 1:
        raise ValueError(f'the captures must share one depth-map size, got {sorted(shapes)}')
    if any(cap.c2w is None for cap in caps):
        raise ValueError('c2w must be a finite [4, 4] matrix, got None')
    poses = np.stack([_args.pose_matrix(cap.c2w) for cap in caps])
    results = []
    for i, cap in enumerate(caps):
        near = nearest_views(poses, i, neighbours)
        results.append(refine_depth_photo(cap.depth, cap.image, [caps[j].image for j in near], cap.K, poses[i], np.stack([np.asarray(
            caps[j].K.cpu() if torch.is_tensor(caps[j].K) else caps[j].K, dtype=np.float64) for j in near]), poses[near], **kw))
    return [cap._replace(depth=r['depth']) for cap, r in zip(caps, results)], results
