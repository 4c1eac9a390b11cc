"""Training batches on the device from RGB-D captures with intrinsics and poses: the ``(image, queries, targets)`` that
``cotr_amd.training.compute_loss`` consumes, which the reference makes in numpy in ``COTR/datasets/cotr_dataset.py``
(``COTRDataset`` / ``COTRZoomDataset.__getitem__``) and ``COTR/projector/pcd_projector.py``.

The geometry runs in ``cotr_amd/csrc/reproject.hip`` (``cotr_depth_corrs``, ``cotr_depth_valid``, ``cotr_crop_depth_nearest``),
the image half in the Pillow-exact ``cotr_crop_resize_pairs``; the rule, the randomness contract and the measured times are
in DESIGN.md 3j.  What is left to torch is plumbing on ``[B]`` and ``[B, num_kp, 4]`` tensors.  No step of the batch
builders reads a count back to the host.

A capture is a ``Capture(image, depth, K, c2w)``: ``image`` uint8 [H, W, 3] and ``depth`` float32 [H, W] (device tensors,
or numpy arrays that get uploaded), ``K`` 3 x 3 and ``c2w`` 4 x 4 float64 on the host.  A CPU tensor is refused: there is
no CPU fallback.

The reference's one augmentation, ``--need_rotation`` (``capture.rotate_capture`` before any reprojection), is
``rotate_captures`` / ``draw_rotations`` and the ``rotations`` keyword of the batch builders: cv2's ``warpAffine`` rule in
``cotr_amd/csrc/rotate.hip`` (``cotr_rotate_captures``), DESIGN.md 3l."""
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import check_op, on, ptr

OUT = 256              # constants.MAX_SIZE of the reference
MAX_TRY = 100          # get_seed_corr's max_try
ROT_MAX = 16384        # the longest side cotr_rotate_captures takes (csrc/rotate.hip)
_RAND_SHAPES = {'seed': lambda b, kp, t: (b, t), 'zoom': lambda b, kp, t: (b,), 'jitter': lambda b, kp, t: (b, 2),
                'trim': lambda b, kp, t: (b, kp), 'flip': lambda b, kp, t: (b,)}


class Capture(NamedTuple):
    image: object      # uint8 [H, W, 3]
    depth: object      # float32 [H, W]
    K: object          # float64 3 x 3 (host)
    c2w: object        # float64 4 x 4 camera-to-world (host)


def _check_capture(cap, what='capture', need_image=True):
    """shapes and dtypes of a capture -> (H, W); every check runs before an upload"""
    if not isinstance(cap, tuple) or len(cap) != 4:
        raise ValueError(f'{what} must be a Capture(image, depth, K, c2w)')
    image, depth, K, c2w = cap
    if image is None and need_image:
        raise ValueError(f'{what}.image is missing')
    for name, x in (('image', image), ('depth', depth)):
        if x is None and name == 'image' and not need_image:
            continue
        if torch.is_tensor(x):
            if not x.is_cuda:
                raise _lib.CotrHipError(f'{what}.{name}: the batch builders run on an MI355X only (HIP kernels, no CPU fallback): '
                                        'got a CPU tensor; pass a numpy array or move the tensor with .cuda()')
        elif not isinstance(x, np.ndarray):
            raise ValueError(f'{what}.{name} must be a numpy array or a device tensor, got {type(x).__name__}')
    if depth.dtype not in (np.float32, torch.float32):
        raise ValueError(f'{what}.depth must be float32, got {depth.dtype}')
    if len(depth.shape) != 2 or depth.shape[0] < 1 or depth.shape[1] < 1:
        raise ValueError(f'{what}.depth must be [H, W], got shape {tuple(depth.shape)}')
    H, W = int(depth.shape[0]), int(depth.shape[1])
    if H * W > 1 << 28:   # MAX_PIXELS of csrc/handleless.h
        raise ValueError(f'{what}.depth: at most 2^28 pixels, got {H} x {W}')
    if image is not None:
        if image.dtype not in (np.uint8, torch.uint8):
            raise ValueError(f'{what}.image must be uint8, got {image.dtype}')
        if tuple(image.shape) != (H, W, 3):
            raise ValueError(f'{what}.image must be [H, W, 3] with the depth\'s H and W, got shape {tuple(image.shape)}')
    for name, m, shape in (('K', K, (3, 3)), ('c2w', c2w, (4, 4))):
        if torch.is_tensor(m) or np.asarray(m).shape != shape or np.asarray(m).dtype != np.float64:
            raise ValueError(f'{what}.{name} must be a float64 {shape[0]} x {shape[1]} host array')
        if not np.isfinite(np.asarray(m)).all():
            raise ValueError(f'{what}.{name} must be finite')
    return H, W


def _device_of(caps):
    devs = {x.device for cap in caps for x in cap[:2] if torch.is_tensor(x)}
    if len(devs) > 1:
        raise ValueError(f'the tensors of one call must be on one device, got {sorted(str(d) for d in devs)}')
    return devs.pop() if devs else torch.device('cuda', torch.cuda.current_device())


def _cam_rows(from_cap, to_cap):
    """Kinv_from | c2w_from | P_to = K_to . w2c_to[0:3] as 37 float64, formed in numpy where the reference forms them
    (pcd_projector.py:74, :143)"""
    kinv = np.linalg.inv(np.asarray(from_cap.K))
    p_to = np.matmul(np.asarray(to_cap.K), np.linalg.inv(np.asarray(to_cap.c2w))[0:3, :])
    return np.concatenate([kinv.ravel(), np.asarray(from_cap.c2w).ravel(), p_to.ravel()])


def _compact(valid_only, ptrs, shapes, cams, n, max_src, cap, device, zero=True):
    """one cotr_depth_corrs / cotr_depth_valid call -> (rows [n, cap, 4] float64 or indices [n, cap] int32, counts [n] int32);
    what the kernel does not write stays 0, or with zero=False is left uninitialised (the caller masks by the counts)"""
    lib = _lib.load_library()
    out = (torch.zeros if zero else torch.empty)((n, cap) if valid_only else (n, cap, 4), dtype=torch.int32 if valid_only else torch.float64, device=device)
    counts = torch.zeros(n, dtype=torch.int32, device=device)
    nbytes = lib.cotr_depth_corrs_scratch(n, max_src)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        if valid_only:
            check_op(lib.cotr_depth_valid(ptr(ptrs), ptr(shapes), n, max_src, ptr(out), cap, ptr(counts), ptr(scratch), nbytes,
                                          _lib.current_stream_ptr()), 'cotr_depth_valid')
        else:
            check_op(lib.cotr_depth_corrs(ptr(ptrs), ptr(shapes), ptr(cams), n, max_src, ptr(out), cap, ptr(counts), ptr(scratch),
                                          nbytes, _lib.current_stream_ptr()), 'cotr_depth_corrs')
    return out, counts


def _tables(from_depths, to_depths, subsets, device):
    """ptrs [n, 3] int64 and shapes [n, 5] int32 of the items, uploaded"""
    ptrs, shapes = [], []
    for f, t, s in zip(from_depths, to_depths, subsets):
        ptrs.append((f.data_ptr(), t.data_ptr() if t is not None else 0, s.data_ptr() if s is not None else 0))
        shapes.append((f.shape[0], f.shape[1], t.shape[0] if t is not None else 0, t.shape[1] if t is not None else 0,
                       s.numel() if s is not None else f.shape[0] * f.shape[1]))
    return (torch.tensor(ptrs, dtype=torch.int64).to(device), torch.tensor(shapes, dtype=torch.int32).to(device),
            max(max(s[4] for s in shapes), 1))


def _subset_tensor(subset, n_px, device):
    if torch.is_tensor(subset):
        if not subset.is_cuda:
            raise _lib.CotrHipError('subset: got a CPU tensor; pass a numpy array or move the tensor with .cuda()')
        if subset.dtype not in (torch.int32, torch.int64) or subset.dim() != 1:
            raise ValueError('subset must be a 1-d integer list of source pixel indices y * W + x')
        return subset.to(device=device, dtype=torch.int32).contiguous()
    s = np.asarray(subset)
    if s.ndim != 1 or not np.issubdtype(s.dtype, np.integer):
        raise ValueError('subset must be a 1-d integer list of source pixel indices y * W + x')
    if s.size and (s.min() < 0 or s.max() >= n_px):
        raise ValueError(f'subset: indices must be in [0, {n_px})')
    return torch.from_numpy(s.astype(np.int32)).to(device)


def depth_corrs(from_cap, to_cap, subset=None, cap=None):
    """``COTRZoomDataset.get_corrs(from_cap, to_cap)``: every pixel of ``from_cap`` with depth > 0 un-projected, projected
    into ``to_cap`` and kept where the two depths agree within 0.5 -> float64 [n, 4] rows (x, y, u, v) on the device, in
    row-major order of (y, x).  The rule is in DESIGN.md 3j (``cotr_depth_corrs``).

    subset: int list of source pixel indices ``y * W + x``; only those are evaluated and the rows come in list order
        (repeats allowed) - the reference's ``reduced_size`` path with the choice made by the caller.
    Batched form: lists of captures (and a list of subsets or None) -> ``(rows [B, cap, 4], counts [B] int32)`` on the
    device, with no read-back; rows past an item's count are 0, rows past ``cap`` (default: the largest number of source
    pixels) are counted but not written.  The single form reads its count back to size the result."""
    single = isinstance(from_cap, Capture) or (isinstance(from_cap, tuple) and len(from_cap) == 4 and not isinstance(from_cap[0], tuple))
    froms, tos = ([from_cap], [to_cap]) if single else (list(from_cap), list(to_cap))
    subsets = [subset] if single else (list(subset) if subset is not None else [None] * len(froms))
    if not (len(froms) == len(tos) == len(subsets)) or not froms:
        raise ValueError('from_cap, to_cap and subset must be lists of one non-zero length')
    for i, (f, t) in enumerate(zip(froms, tos)):
        _check_capture(f, f'from_cap[{i}]', need_image=False)
        _check_capture(t, f'to_cap[{i}]', need_image=False)
    device = _device_of(froms + tos)
    fd, td = [on(f.depth, device) for f in froms], [on(t.depth, device) for t in tos]
    sub = [None if s is None else _subset_tensor(s, d.numel(), device) for s, d in zip(subsets, fd)]
    if any(s is not None and s.numel() == 0 for s in sub):
        raise ValueError('an empty subset')
    ptrs, shapes, max_src = _tables(fd, td, sub, device)
    cams = torch.from_numpy(np.stack([_cam_rows(f, t) for f, t in zip(froms, tos)])).to(device)
    cap = max_src if cap is None else int(cap)
    if cap < 0:
        raise ValueError('cap must be >= 0')
    rows, counts = _compact(False, ptrs, shapes, cams, len(froms), max_src, max(cap, 0), device)
    if single:
        return rows[0, :min(int(counts[0]), cap)]
    return rows, counts


def valid_pixels(depths):
    """indices ``y * W + x`` of the pixels with depth > 0 of each device depth map, in row-major order ->
    ``(indices [B, max H*W] int32, counts [B] int32)``: ``np.where(depth > 0)`` by the compaction of ``cotr_depth_valid``"""
    device = depths[0].device
    ptrs, shapes, max_src = _tables(depths, [None] * len(depths), [None] * len(depths), device)
    return _compact(True, ptrs, shapes, None, len(depths), max_src, max_src, device)


def _crop_depths(depths, boxes, out):
    """cotr_crop_depth_nearest: depths list of device [H, W] float32, boxes int32 [n, 3] on the device -> [n, out, out]"""
    device = depths[0].device
    n = len(depths)
    srcs = torch.tensor([d.data_ptr() for d in depths], dtype=torch.int64).to(device)
    shapes = torch.tensor([tuple(d.shape) for d in depths], dtype=torch.int32).to(device)
    dst = torch.empty((n, out, out), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        check_op(_lib.load_library().cotr_crop_depth_nearest(ptr(srcs), ptr(shapes), ptr(boxes), n, ptr(dst), out,
                                                             _lib.current_stream_ptr()), 'cotr_crop_depth_nearest')
    return dst


def _crop_images(img_a, img_b, boxes6, out_slot, max_size):
    """cotr_crop_resize_pairs for ONE pair: boxes6 int32 [1, 6] on the device -> out_slot [1, 3, 256, 512] (normalised)"""
    with torch.cuda.device(img_a.device):
        rc = _lib.load_library().cotr_crop_resize_pairs(ptr(img_a), img_a.shape[0], img_a.shape[1], ptr(img_b), img_b.shape[0],
                                                        img_b.shape[1], ptr(boxes6), 1, ptr(out_slot), max_size,
                                                        _lib.current_stream_ptr())
    if rc != 0:
        raise _lib.CotrHipError(f'cotr_crop_resize_pairs failed (code {rc})')


_MEAN = (0.485, 0.456, 0.406)
_STD = (0.229, 0.224, 0.225)


def cropped_K(K, box, out=OUT):
    """``crop_pinhole_camera`` with a ``CropCamConfig``: scale = out / size, fx, fy *= scale, cx = (cx - x) scale,
    cy = (cy - y) scale, in float64; (fx, fy, cx, cy) are all the reference's PinholeCamera keeps of K"""
    x, y, size = (float(v) for v in box)
    K = np.asarray(K, dtype=np.float64)
    scale = out / size
    return np.array([[K[0, 0] * scale, 0.0, (K[0, 2] - x) * scale], [0.0, K[1, 1] * scale, (K[1, 2] - y) * scale], [0.0, 0.0, 1.0]])


def crop_capture(cap, box, out=OUT):
    """``capture.crop_capture(cap, CropCamConfig(x, y, size, size, out, out))``: box = (x, y, size) inside the capture ->
    Capture with device tensors.  The image goes through ``cotr_crop_resize_pairs`` (Pillow's 8-bit BILINEAR, bit-exact;
    its normalised float output is brought back to the uint8 it was computed from, which is exact), the depth through
    ``cotr_crop_depth_nearest`` (Pillow NEAREST in mode 'F', bit-exact), K by ``cropped_K``; the pose is unchanged.
    The image kernel resizes to 256 only: another ``out`` needs ``cap.image`` None (depth-only capture)."""
    H, W = _check_capture(cap, need_image=False)
    x, y, size = (int(v) for v in box)
    if not (size >= 1 and 0 <= x and 0 <= y and x + size <= W and y + size <= H):
        raise ValueError(f'box {tuple(box)} must lie inside the {H} x {W} capture')
    if not 1 <= int(out) <= 4096:
        raise ValueError('out must be in [1, 4096]')
    device = _device_of([cap])
    depth = on(cap.depth, device)
    boxes = torch.tensor([[x, y, size]], dtype=torch.int32).to(device)
    zdepth = _crop_depths([depth], boxes, int(out))[0]
    image = None
    if cap.image is not None:
        if out != OUT or size < 2 or size > 7936:
            raise ValueError('the image crop resizes boxes of 2 ... 7936 pixels to 256 x 256 only')
        img = on(cap.image, device)
        sbs = torch.empty((1, 3, OUT, 2 * OUT), dtype=torch.float32, device=device)
        _crop_images(img, img, torch.cat([boxes, boxes], 1).contiguous(), sbs, size)
        mean, std = (torch.tensor(v, device=device).view(3, 1, 1) for v in (_MEAN, _STD))
        image = ((sbs[0, :, :, :OUT] * std + mean) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    return Capture(image, zdepth, cropped_K(cap.K, (x, y, size), out), np.asarray(cap.c2w))


def draw_rand(batch, num_kp, max_try=MAX_TRY, generator=None, device=None):
    """The uniform numbers of one batch, float64 in [0, 1), drawn from ``generator`` (a device generator, or None for
    the default one) in this order: seed [B, max_try], zoom [B], jitter [B, 2], trim [B, num_kp], flip [B]."""
    device = device or torch.device('cuda', torch.cuda.current_device())
    return {k: torch.rand(shape(batch, num_kp, max_try), dtype=torch.float64, device=device, generator=generator)
            for k, shape in _RAND_SHAPES.items()}


def _rand_on(rand, batch, num_kp, generator, device, need):
    if rand is None:
        return draw_rand(batch, num_kp, generator=generator, device=device)
    out = {}
    for k in need:
        if k not in rand:
            raise ValueError(f'rand[{k!r}] is missing')
        t = rand[k]
        if torch.is_tensor(t) and not t.is_cuda:
            raise _lib.CotrHipError(f'rand[{k!r}]: got a CPU tensor; pass a numpy array or move the tensor with .cuda()')
        t = on(np.asarray(t, dtype=np.float64) if not torch.is_tensor(t) else t, device).double()
        want = _RAND_SHAPES[k](batch, num_kp, t.shape[1] if k == 'seed' and t.dim() == 2 else MAX_TRY)
        if tuple(t.shape) != want:
            raise ValueError(f'rand[{k!r}] must have shape {want}, got {tuple(t.shape)}')
        out[k] = t
    return out


def _pick(u, count):
    """floor(u * count) as an index below count (0 where count is 0): u [B, k] float64, count [B]"""
    c = count.to(torch.float64).unsqueeze(1)
    return torch.minimum(torch.floor(u * c), (c - 1).clamp(min=0)).to(torch.int64)


def _device_boxes(shape_hw, pos, scale):
    """``patch_boxes`` / ``get_patch_centered_at`` on the device: shape_hw [B, 2] (h, w), pos [B, 2] (x, y), scale [B], all
    float64 -> (x, y, size) float64 [B, 3] holding integers"""
    h, w = shape_hw[:, 0], shape_hw[:, 1]
    size = torch.floor(torch.minimum(h, w) * scale.clamp(0.0, 1.0) / 2) * 2
    lu = torch.trunc(pos - (size / 2).unsqueeze(1)).clamp(min=0.0)
    lim = torch.stack([w, h], 1) - size.unsqueeze(1)
    lu = torch.where(lu > lim, lim, lu)
    return torch.cat([lu, size.unsqueeze(1)], 1)


def _zoomed_cams(K_host, boxes, out):
    """fx, fy, cx, cy [B, 4] float64 (device) of the captures cropped to ``boxes`` [B, 3] (device): ``cropped_K``"""
    scale = out / boxes[:, 2]
    return torch.stack([K_host[:, 0] * scale, K_host[:, 1] * scale, (K_host[:, 2] - boxes[:, 0]) * scale,
                        (K_host[:, 3] - boxes[:, 1]) * scale], 1)


def _assemble(image, rows, counts, ok, num_kp, u_trim, u_flip, bidirectional):
    """steps 5-9: trim, flip, + 256, normalise, stack.  rows [B, cap, 4] = (x_query, y_query, x_nn, y_nn) float64"""
    B = rows.shape[0]
    valid = ok & (counts >= num_kp)
    idx = _pick(u_trim, counts).clamp(max=rows.shape[1] - 1)
    corrs = torch.gather(rows, 1, idx.unsqueeze(2).expand(B, num_kp, 4))
    corrs = torch.where(valid.view(B, 1, 1), corrs, torch.zeros_like(corrs))      # rows past a count are not initialised
    flip = u_flip < 0.5
    f3 = flip.view(B, 1)
    x0 = torch.where(f3, (OUT - 1) - corrs[..., 0], corrs[..., 0])
    x2 = torch.where(f3, (OUT - 1) - corrs[..., 2], corrs[..., 2]) + OUT
    corrs = torch.stack([x0, corrs[..., 1], x2, corrs[..., 3]], 2) / torch.tensor([2.0 * OUT, OUT, 2.0 * OUT, OUT], dtype=torch.float64,
                                                                                   device=rows.device)
    halves = image.view(B, 3, OUT, 2, OUT)
    image = torch.where(flip.view(B, 1, 1, 1, 1), halves.flip(4), halves).reshape(B, 3, OUT, 2 * OUT)
    corrs = corrs.float()
    if bidirectional:
        queries = torch.cat([corrs[..., :2], corrs[..., 2:]], 1)
        targets = torch.cat([corrs[..., 2:], corrs[..., :2]], 1)
    else:
        queries, targets = corrs[..., :2].contiguous(), corrs[..., 2:].contiguous()
    return {'image': image, 'corrs': corrs, 'queries': queries, 'targets': targets, 'valid': valid}


def _validate(query_caps, nn_caps, num_kp):
    query_caps, nn_caps = list(query_caps), list(nn_caps)
    if not query_caps or len(query_caps) != len(nn_caps):
        raise ValueError('query_caps and nn_caps must be lists of one non-zero length')
    if int(num_kp) != num_kp or num_kp < 1:
        raise ValueError('num_kp must be a positive integer')
    for i, (q, n) in enumerate(zip(query_caps, nn_caps)):
        _check_capture(q, f'query_caps[{i}]')
        _check_capture(n, f'nn_caps[{i}]')
    return query_caps, nn_caps


def _upload(query_caps, nn_caps):
    device = _device_of(query_caps + nn_caps)
    up = lambda c: Capture(on(c.image, device), on(c.depth, device), np.asarray(c.K), np.asarray(c.c2w))   # noqa: E731
    return [up(c) for c in query_caps], [up(c) for c in nn_caps], device


def _angle(angle):
    try:
        a = float(angle)
    except (TypeError, ValueError):
        a = math.nan
    if not math.isfinite(a):
        raise ValueError(f'the angle must be a finite number of degrees, got {angle!r}')
    return a


def _angles(angles, n):
    try:
        a = np.asarray(angles, dtype=np.float64)
    except (TypeError, ValueError, RuntimeError):
        a = np.full(0, np.nan)
    if a.shape != (n,) or not np.isfinite(a).all():
        raise ValueError(f'angles must be {n} finite floats (degrees), one per capture')
    return a


def _rot_sides(H, W, what):
    if not (1 <= H <= ROT_MAX and 1 <= W <= ROT_MAX):
        raise ValueError(f'{what}: the rotation takes sides in [1, {ROT_MAX}], got {H} x {W}')


def rotation_matrix(shape_hw, angle):
    """``m0..m5`` float64 [6]: what ``cv2.warpAffine`` works with for ``capture.rotate_image(image, angle)`` - the matrix of
    ``cv2.getRotationMatrix2D((W / 2, H / 2), angle, 1.0)``, inverted the way ``warpAffine`` inverts it, so that it maps a
    destination pixel to the source: ``(m0 x + m1 y + m2, m3 x + m4 y + m5)``.  Host float64, the C library's cos / sin
    (DESIGN.md 3l)."""
    H, W = (int(v) for v in shape_hw)
    _rot_sides(H, W, 'shape_hw')
    t = _angle(angle) * (math.pi / 180)                  # cv2: angle *= CV_PI / 180
    al, be = math.cos(t), math.sin(t)
    cx, cy = W / 2, H / 2
    m = [al, be, (1 - al) * cx - be * cy, -be, al, be * cx + (1 - al) * cy]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return np.array(m, dtype=np.float64)


def rotated_c2w(c2w, angle):
    """``rotate_camera_pose``: ``w2c' = Rz . inv(c2w)`` with ``Rz = [[cos r, sin r, 0, 0], [-sin r, cos r, 0, 0], [0, 0, 1, 0],
    [0, 0, 0, 1]]``, ``r = angle / 180 * pi`` -> ``c2w' = inv(w2c')``, float64 4 x 4 on the host.  The reference's float32
    quaternion + translation storage of the result is not reproduced.  Angle 0 returns ``c2w`` as it is."""
    c2w = np.asarray(c2w)
    if c2w.shape != (4, 4) or c2w.dtype != np.float64 or not np.isfinite(c2w).all():
        raise ValueError('c2w must be a finite float64 4 x 4 host array')
    a = _angle(angle)
    if a == 0:
        return c2w
    r = a / 180 * np.pi
    s, c = np.sin(r), np.cos(r)
    rz = np.array([[c, s, 0.0, 0.0], [-s, c, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    return np.linalg.inv(np.matmul(rz, np.linalg.inv(c2w)))


def _rotate_launch(items, device):
    """ONE cotr_rotate_captures launch: items = [(image uint8 [H, W, 3] or None, depth float32 [H, W] or None, m float64 [6])],
    contiguous tensors on ``device`` -> [(rotated image or None, rotated depth or None)], freshly allocated.  The three
    tables travel as one upload."""
    n = len(items)
    table = np.zeros(11 * n, dtype=np.int64)
    ptrs, shapes, mats = table[:4 * n].reshape(n, 4), table[4 * n:5 * n].view(np.int32).reshape(n, 2), table[5 * n:].view(np.float64).reshape(n, 6)
    outs = []
    for k, (image, depth, m) in enumerate(items):
        out = tuple(None if x is None else torch.empty_like(x) for x in (image, depth))
        ptrs[k] = [0 if x is None else x.data_ptr() for x in (image, out[0], depth, out[1])]
        shapes[k] = (image if depth is None else depth).shape[:2]
        mats[k] = m
        outs.append(out)
    dev = torch.from_numpy(table).to(device)
    with torch.cuda.device(device):
        check_op(_lib.load_library().cotr_rotate_captures(ptr(dev[:4 * n]), ptr(dev[4 * n:5 * n]), ptr(dev[5 * n:]), n,
                                                          int(shapes[:, 0].max()), int(shapes[:, 1].max()),
                                                          _lib.current_stream_ptr()), 'cotr_rotate_captures')
    return outs


def _rotate(caps, angles, device):
    """rotate_captures after its checks"""
    caps = list(caps)
    turn = [k for k, a in enumerate(angles) if a != 0]
    if not turn:
        return caps
    items = []
    for k in turn:
        c = caps[k]
        items.append((None if c.image is None else on(c.image, device), on(c.depth, device),
                      rotation_matrix(c.depth.shape, angles[k])))
    for k, (image, depth) in zip(turn, _rotate_launch(items, device)):
        caps[k] = Capture(image, depth, caps[k].K, rotated_c2w(caps[k].c2w, angles[k]))
    return caps


def rotate_captures(caps, angles):
    """``capture.rotate_capture(cap, angle)`` for a list of captures (any mix of shapes) in ONE launch: the image through
    ``cv2.warpAffine(..., INTER_LINEAR)`` and the depth through ``cv2.warpAffine(..., INTER_NEAREST)`` about the centre
    ``(W / 2, H / 2)`` with the border value 0, the pose turned about the optical axis (``rotated_c2w``); the rule is in
    DESIGN.md 3l.  angles: degrees, one finite float per capture.  -> list of ``Capture`` with device tensors, ``K`` the same
    array; a capture whose ``image`` is None has only its depth rotated, and a capture with angle 0 comes back as it is
    (the same object, no kernel work), as in the reference's ``rot == 0`` branch."""
    caps = list(caps)
    if not caps:
        raise ValueError('caps must be a non-empty list of captures')
    for i, c in enumerate(caps):
        _rot_sides(*_check_capture(c, f'caps[{i}]', need_image=False), f'caps[{i}]')
    angles = _angles(angles, len(caps))
    return _rotate(caps, angles, _device_of(caps))


def rotate_capture(cap, angle):
    """``rotate_captures`` for one capture"""
    return rotate_captures([cap], [_angle(angle)])[0]


def rotate_image(image, angle, nearest=False):
    """``capture.rotate_image(image, angle)`` for one uint8 [H, W, 3] image (``cv2.INTER_LINEAR``), or with ``nearest=True``
    for one float32 [H, W] map (``interpolation=cv2.INTER_NEAREST``, what the reference applies to a depth map) -> device
    tensor of the same shape.  numpy array or device tensor; one ``cotr_rotate_captures`` launch."""
    want = 'a float32 [H, W] map' if nearest else 'a uint8 [H, W, 3] image'
    if torch.is_tensor(image):
        if not image.is_cuda:
            raise _lib.CotrHipError('image: the batch builders run on an MI355X only (HIP kernels, no CPU fallback): '
                                    'got a CPU tensor; pass a numpy array or move the tensor with .cuda()')
    elif not isinstance(image, np.ndarray):
        raise ValueError(f'image must be a numpy array or a device tensor, got {type(image).__name__}')
    ok = image.dtype in ((np.float32, torch.float32) if nearest else (np.uint8, torch.uint8)) and \
        (len(image.shape) == 2 if nearest else len(image.shape) == 3 and image.shape[2] == 3)
    if not ok:
        raise ValueError(f'image must be {want}, got {image.dtype} {tuple(image.shape)}')
    _rot_sides(int(image.shape[0]), int(image.shape[1]), 'image')
    m = rotation_matrix(image.shape[:2], angle)
    device = image.device if torch.is_tensor(image) else torch.device('cuda', torch.cuda.current_device())
    x = on(image, device)
    return _rotate_launch([(None, x, m) if nearest else (x, None, m)], device)[0][1 if nearest else 0]


def draw_rotations(batch, max_rotation, rotation_chance, rng=None):
    """The angles of ``augment_with_rotation`` for one batch -> float64 [B, 2] degrees on the host, column 0 the query
    capture, column 1 the nn capture: per capture two uniforms ``u_c``, ``u_t`` from ``rng`` (a ``numpy.random.Generator``;
    None: a fresh ``default_rng()``), in the order query then nn; the angle is ``(2 u_t - 1) max_rotation`` if
    ``u_c < rotation_chance``, else 0.  Host-side because the pose and the matrix are formed there; bit-parity with the
    reference's ``random.random()`` / ``np.random.uniform`` streams is not a goal (it draws ``u_t`` only after a hit)."""
    if int(batch) != batch or batch < 1:
        raise ValueError('batch must be a positive integer')
    if not (math.isfinite(max_rotation) and math.isfinite(rotation_chance)):
        raise ValueError('max_rotation and rotation_chance must be finite')
    rng = np.random.default_rng() if rng is None else rng
    u = rng.random((int(batch), 2, 2))                    # [sample, (query, nn), (u_c, u_t)]
    return np.where(u[..., 0] < rotation_chance, (2.0 * u[..., 1] - 1.0) * float(max_rotation), 0.0)


def _rotated_pairs(q, n, rotations):
    """the ``rotations`` [B, 2] of a batch builder applied to its validated captures: all 2B in one launch"""
    B = len(q)
    try:
        rot = np.asarray(rotations, dtype=np.float64)
    except (TypeError, ValueError, RuntimeError):
        rot = None
    if rot is None or rot.shape != (B, 2) or not np.isfinite(rot).all():
        raise ValueError(f'rotations [B, 2] must be {B} x 2 finite floats (degrees): column 0 the query capture, column 1 the nn capture')
    rot = rot.T.ravel()                                   # the order of q + n
    if not rot.any():
        return q, n
    for i, c in enumerate(q + n):
        _rot_sides(c.depth.shape[0], c.depth.shape[1], ('query_caps' if i < B else 'nn_caps') + f'[{i % B}]')
    caps = _rotate(q + n, rot, _device_of(q + n))
    return caps[:B], caps[B:]


def make_batch(query_caps, nn_caps, num_kp, bidirectional=True, rand=None, generator=None, rotations=None):
    """``COTRDataset.__getitem__`` for a batch of 256 x 256 capture pairs (no zoom) ->
    ``{'image' [B, 3, 256, 512] float32, 'corrs' [B, num_kp, 4], 'queries', 'targets', 'valid' [B] bool}`` on the device.
    As the reference does there, the nn capture is projected into the query capture (rows in the nn capture's row-major
    order) and a row of ``corrs`` is (x_query, y_query, x_nn + 256, y_nn) / (512, 256, 512, 256).  Uniforms: ``rand`` with
    'trim' [B, num_kp] and 'flip' [B], else ``draw_rand``.  See ``make_zoom_batch`` for the steps, the contract and ``rotations``."""
    q, n = _validate(query_caps, nn_caps, num_kp)
    B = len(q)
    for c in q + n:
        if tuple(c.depth.shape) != (OUT, OUT):
            raise ValueError(f'make_batch takes {OUT} x {OUT} captures (make_zoom_batch crops larger ones)')
    if rotations is not None:
        q, n = _rotated_pairs(q, n, rotations)
    q, n, device = _upload(q, n)
    rand = _rand_on(rand, B, num_kp, generator, device, ('trim', 'flip'))
    rows, counts = depth_corrs(n, q)
    rows = rows[..., [2, 3, 0, 1]]
    image = torch.empty((B, 3, OUT, 2 * OUT), dtype=torch.float32, device=device)
    box = torch.tensor([[0, 0, OUT, 0, 0, OUT]], dtype=torch.int32).to(device)
    for b in range(B):
        _crop_images(q[b].image, n[b].image, box, image[b:b + 1], OUT)
    return _assemble(image, rows, counts, torch.ones(B, dtype=torch.bool, device=device), num_kp, rand['trim'], rand['flip'], bidirectional)


def make_zoom_batch(query_caps, nn_caps, num_kp, zooms, zoom_jitter, bidirectional=True, rand=None, generator=None, rotations=None):
    """``COTRZoomDataset.__getitem__`` for a batch of capture pairs ->
    ``{'image' [B, 3, 256, 512] float32, 'corrs' [B, num_kp, 4], 'queries', 'targets', 'valid' [B] bool}`` on the device.

    Per sample, in the reference's order: (1) seed: ``max_try`` valid pixels of the nn capture are projected into the
    query capture, the first survivor is the seed; (2) zoom boxes by the ``get_patch_centered_at`` rule around the seed,
    the query side's centre jittered; (3) both captures cropped to 256 x 256 (image: Pillow BILINEAR, depth: Pillow
    NEAREST, K: ``cropped_K``); (4) ``depth_corrs(query_zoom, nn_zoom)``; (5) trim to ``num_kp``; (6) flip (x -> 255 - x on
    both halves, images mirrored); (7) + 256 on the target x; (8) / (512, 256, 512, 256); (9) bidirectional stacking.
    No count is read back: the boxes are computed on the device, and a sample whose seed search fails or whose count is
    below ``num_kp`` comes back with ``valid`` False (its other entries are filler) - redraw it, which replaces the
    reference's recursive ``__getitem__``.

    Randomness: every choice is a function of uniforms in [0, 1), passed as ``rand`` = {'seed' [B, max_try], 'zoom' [B],
    'jitter' [B, 2], 'trim' [B, num_kp], 'flip' [B]} (float64; numpy or device tensors) or drawn by ``draw_rand(...,
    generator)`` in that order.  seed: draw t picks valid pixel floor(u * count) of the nn capture; zoom:
    zooms[floor(u * len)]; jitter: (2u - 1) * zoom_jitter per axis, in units of the patch size; trim: row
    floor(u * count), with replacement; flip: u < 0.5.  Bit-parity with ``np.random`` is not a goal.
    Two deliberate differences from the reference: seed candidates are drawn WITH replacement (the reference draws 100
    without), and the shuffle before the trim is dropped (it does not change the distribution of a with-replacement
    draw; the seed is likewise the first survivor in draw order instead of a shuffled one).

    rotations: None, or float64 [B, 2] degrees (column 0 the query capture, column 1 the nn capture; ``draw_rotations``):
    step 0, the reference's ``augment_with_rotation`` - all 2B captures go through ``rotate_captures`` in one launch before
    step 1; a capture with angle 0 is left alone, and None or all zeros add no launch."""
    q, n = _validate(query_caps, nn_caps, num_kp)
    B = len(q)
    zooms_h = np.asarray(zooms, dtype=np.float64).ravel()
    if zooms_h.size == 0 or not np.isfinite(zooms_h).all():
        raise ValueError('zooms must be a non-empty list of finite scales')
    shorts = [min(c.depth.shape) for c in q + n]
    if min(shorts) * float(np.clip(zooms_h, 0.0, 1.0).min()) < 2 or max(shorts) > 7936:
        raise ValueError('every zoom must leave a patch of at least 2 pixels, and the short sides must be <= 7936')
    if rotations is not None:
        q, n = _rotated_pairs(q, n, rotations)
    q, n, device = _upload(q, n)
    rand = _rand_on(rand, B, num_kp, generator, device, ('seed', 'zoom', 'jitter', 'trim', 'flip'))
    f64 = dict(dtype=torch.float64, device=device)

    # 1. seed
    vidx, vcount = valid_pixels([c.depth for c in n])
    subset = torch.gather(vidx, 1, _pick(rand['seed'], vcount))
    subset = torch.where((vcount > 0).unsqueeze(1), subset, torch.full_like(subset, -1)).contiguous()
    max_try = subset.shape[1]
    ptrs, shapes, _ = _tables([c.depth for c in n], [c.depth for c in q], [subset[b] for b in range(B)], device)
    cams = torch.from_numpy(np.stack([_cam_rows(a, b) for a, b in zip(n, q)])).to(device)
    seeds, seed_count = _compact(False, ptrs, shapes, cams, B, max_try, max_try, device)
    seed = seeds[:, 0]                                   # (x_nn, y_nn, u_query, v_query); zeros where nothing survived
    # 2. boxes
    scale = torch.tensor(zooms_h, **f64)[_pick(rand['zoom'].unsqueeze(1), torch.full((B,), zooms_h.size, device=device))[:, 0]]
    hw_q = torch.tensor([tuple(c.depth.shape) for c in q], **f64)
    hw_n = torch.tensor([tuple(c.depth.shape) for c in n], **f64)
    box_n = _device_boxes(hw_n, seed[:, 0:2], scale)
    first = _device_boxes(hw_q, seed[:, 2:4], scale)
    box_q = _device_boxes(hw_q, seed[:, 2:4] + first[:, 2:3] * ((2 * rand['jitter'] - 1) * float(zoom_jitter)), scale)
    # 3. crops
    boxes_i = torch.cat([box_q, box_n], 0).to(torch.int32).contiguous()
    zdepth = _crop_depths([c.depth for c in q] + [c.depth for c in n], boxes_i, OUT)
    image = torch.empty((B, 3, OUT, 2 * OUT), dtype=torch.float32, device=device)
    boxes6 = torch.cat([boxes_i[:B], boxes_i[B:]], 1).contiguous()
    for b in range(B):
        _crop_images(q[b].image, n[b].image, boxes6[b:b + 1], image[b:b + 1], max(shorts[b], shorts[B + b]))
    K4 = lambda caps: torch.tensor([(c.K[0, 0], c.K[1, 1], c.K[0, 2], c.K[1, 2]) for c in caps], **f64)   # noqa: E731
    kq, kn = _zoomed_cams(K4(q), box_q, OUT), _zoomed_cams(K4(n), box_n, OUT)
    # 4. depth_corrs(query_zoom, nn_zoom): Kinv of the zoomed query camera in closed form, P = K_zoom . w2c row by row
    zero, one = torch.zeros(B, **f64), torch.ones(B, **f64)
    kinv = torch.stack([1 / kq[:, 0], zero, -kq[:, 2] / kq[:, 0], zero, 1 / kq[:, 1], -kq[:, 3] / kq[:, 1], zero, zero, one], 1)
    c2w = torch.tensor(np.stack([c.c2w.ravel() for c in q]), **f64)
    E = torch.tensor(np.stack([np.linalg.inv(c.c2w)[0:3, :] for c in n]), **f64)
    P = torch.cat([kn[:, 0:1] * E[:, 0] + kn[:, 2:3] * E[:, 2], kn[:, 1:2] * E[:, 1] + kn[:, 3:4] * E[:, 2], E[:, 2]], 1)
    zcams = torch.cat([kinv, c2w, P], 1).contiguous()
    zq, zn = [zdepth[b] for b in range(B)], [zdepth[B + b] for b in range(B)]
    ptrs, shapes, _ = _tables(zq, zn, [None] * B, device)
    rows, counts = _compact(False, ptrs, shapes, zcams, B, OUT * OUT, OUT * OUT, device, zero=False)
    # 5-9
    return _assemble(image, rows, counts, seed_count > 0, num_kp, rand['trim'], rand['flip'], bidirectional)
