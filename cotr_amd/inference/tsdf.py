"""A fused model of registered RGB-D captures on the device: a truncated signed distance (TSDF) volume that averages their
depth maps, and the raycast of that volume from a pose - the model half of KinectFusion, whose tracking half is ``icp_depth``.

``TsdfVolume`` holds the two float32 tensors [Nz,Ny,Nx] and the scalars; ``integrate_depths`` is ``cotr_tsdf_integrate``
(cotr_amd/csrc/tsdf.hip) with device tensors, ``fuse_captures`` the same on ``cotr_amd.data.Capture``s; ``raycast_volume`` is
``cotr_tsdf_raycast``: a float32 depth map (and normals) of the kind ``icp_depth`` reads, so ``track_capture`` - a raycast at
the predicted pose and ``icp_depth`` against it, one device sequence - is frame-to-model tracking with no ICP code of its own.
``extract_mesh`` is ``cotr_tsdf_mesh``: the volume's surface as an indexed triangle mesh (marching tetrahedra),
which ``write_ply`` puts into a file.  A volume made with ``color=True`` also averages the captures' images near the surface
(``integrate_colors``, and ``fuse_captures`` by itself); ``sample_colors`` reads its colour at points such as the mesh vertices,
``color_depth_map`` and ``raycast_volume(colors=True)`` at the pixels of a depth map.  The rules are the
library's own.  No CPU fallback."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args, icp
from ._args import F64, I32
from .icp import _enqueue_icp

MAX_CAPTURES = 32
MAX_VOXELS = 1 << 28
MAX_MESH_VOXELS = 1 << 27
MAX_STEPS = 1 << 16
D3 = ctypes.c_double * 3


class TsdfVolume:
    """``dims`` = (Nx, Ny, Nz) voxels of side ``voxel``; ``origin``: the world position of the centre of voxel (0, 0, 0).
    ``tsdf`` and ``weight``: float32 device tensors [Nz,Ny,Nx], 1 and 0 when fresh.  ``trunc``: the truncation distance (3 voxels
    unless given); ``max_weight``: where a voxel's weight stops growing, so that the model keeps following the captures.
    ``color=True``: ``color``, a float32 device tensor [Nz,Ny,Nx,4] = (r, g, b, colour weight) on the images' scale 0 .. 255, all 0
    when fresh; None otherwise."""

    def __init__(self, origin, voxel, dims, trunc=None, max_weight=64.0, device=None, color=False):
        o = np.asarray(origin, dtype=np.float64)
        if o.shape != (3,) or not np.isfinite(o).all():
            raise ValueError(f'origin must be 3 finite numbers, got {origin}')
        _args.check_positive('voxel', voxel)
        if len(dims) != 3:
            raise ValueError(f'dims must be (Nx, Ny, Nz), got {dims}')
        for name, v in zip(('Nx', 'Ny', 'Nz'), dims):
            _args.check_int_range(name, v, 2, MAX_VOXELS)
        if int(dims[0]) * int(dims[1]) * int(dims[2]) > MAX_VOXELS:
            raise ValueError(f'dims: at most 2^28 voxels, got {dims[0]} x {dims[1]} x {dims[2]}')
        trunc = 3.0 * voxel if trunc is None else trunc
        _args.check_positive('trunc', trunc)
        if not max_weight > 0:
            raise ValueError(f'max_weight must be > 0, got {max_weight}')
        self.origin, self.voxel, self.dims = o, float(voxel), tuple(int(v) for v in dims)
        self.trunc, self.max_weight = float(trunc), float(max_weight)
        self.device = _args.device(device)
        Nx, Ny, Nz = self.dims
        self.tsdf, self.weight = _args.empty(self.device, ((Nz, Ny, Nx), torch.float32), ((Nz, Ny, Nx), torch.float32))
        self.color = _args.empty(self.device, ((Nz, Ny, Nx, 4), torch.float32))[0] if color else None
        self.reset()

    def reset(self):
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.color is not None:
            self.color.zero_()
        return self

    def corners(self):
        """the centres of the 8 corner voxels, [8, 3]"""
        far = self.origin + self.voxel * (np.asarray(self.dims, np.float64) - 1)
        return np.array([[(self.origin, far)[b >> a & 1][a] for a in range(3)] for b in range(8)])


def _volume_args(volume):
    Nx, Ny, Nz = volume.dims
    return ptr(volume.tsdf), ptr(volume.weight), Nx, Ny, Nz, D3(*volume.origin), volume.voxel


def _color_args(volume):
    Nx, Ny, Nz = volume.dims
    return ptr(volume.color), Nx, Ny, Nz, D3(*volume.origin), volume.voxel


def _check_volume(volume):
    if not isinstance(volume, TsdfVolume):
        raise ValueError(f'volume must be a TsdfVolume, got {type(volume).__name__}')


def _check_color_volume(volume):
    _check_volume(volume)
    if getattr(volume, 'color', None) is None:
        raise ValueError('volume holds no colour: make it with TsdfVolume(..., color=True)')


def _capture_args(volume, depths, Ks, c2ws, found, weights, images=None):
    """the argument rules of ``integrate_depths`` (and of ``integrate_colors``, with ``images``) -> (depths, the cameras, the pose
    rows, found, weights[, images]) with every tensor on the volume's device"""
    if len(depths.shape) != 3 or depths.shape[0] < 1:
        raise ValueError(f'depths must be [n, H, W] with n >= 1, got shape {tuple(depths.shape)}')
    _args.check_depth(depths[0])
    n = int(depths.shape[0])
    if images is not None:
        _check_images(images, tuple(depths.shape))
    k = np.asarray(Ks.cpu() if torch.is_tensor(Ks) else Ks, dtype=np.float64)
    if k.shape == (3, 3):
        k = np.broadcast_to(k, (n, 3, 3))
    if k.shape != (n, 3, 3):
        raise ValueError(f'Ks must be [{n}, 3, 3] or [3, 3], got shape {k.shape}')
    ks = [_args.camera(m, 'Ks') for m in k]
    rows = _args.c2w_rows(c2ws, n)
    if weights is not None:
        weights = [float(v) for v in np.asarray(weights, dtype=np.float64).reshape(-1)]
        if len(weights) != n:
            raise ValueError(f'weights must be [{n}], got {len(weights)}')
        for v in weights:
            _args.check_positive('weights', v)
    if found is not None and not torch.is_tensor(found):
        found = np.asarray(found)
    if found is not None and int(np.prod(tuple(found.shape))) != n:
        raise ValueError(f'found must be [{n}], got shape {tuple(found.shape)}')
    _args.no_cpu_tensors('the TSDF volume runs', depths, c2ws, found, images)
    device = volume.device
    out = on(depths, device), ks, on(rows, device), _args.found_i32(found, device), weights
    return out if images is None else out + (on(images, device),)


def _check_images(images, shape, what='images'):
    """uint8, three channels behind the ``shape`` of the depths"""
    if not torch.is_tensor(images):
        images = np.asarray(images)
    if images.dtype != (torch.uint8 if torch.is_tensor(images) else np.uint8):
        raise ValueError(f'{what} must be uint8, got {images.dtype}')
    if tuple(images.shape) != tuple(shape) + (3,):
        raise ValueError(f'{what} must be {list(shape) + [3]}, three channels for every pixel of the depth, got shape {tuple(images.shape)}')


def _enqueue_integrate(lib, volume, depths, ks, c2ws, found, weights):
    """every tensor on the volume's device already, every argument checked, at most 32 maps -> info int32 [n,4]"""
    n, H, W = (int(v) for v in depths.shape)
    info, = _args.empty(volume.device, ((n, 4), I32))
    K = (ctypes.c_double * (9 * n))(*[v for k in ks for v in k])
    w = None if weights is None else (ctypes.c_double * n)(*weights)
    check_op(lib.cotr_tsdf_integrate(*_volume_args(volume), volume.trunc, ptr(depths), n, H, W, K, ptr(c2ws), ptr(found), w, volume.max_weight,
                                     ptr(info), _lib.current_stream_ptr()), 'cotr_tsdf_integrate')
    return info


def integrate_depths(volume, depths, Ks, c2ws, found=None, weights=None):
    """``cotr_tsdf_integrate`` on the current stream: the depth maps ``depths`` float32 [n,H,W] with the cameras ``Ks`` [n,3,3]
    (host; one [3,3] serves every map) and the camera-to-world poses ``c2ws`` [n,4,4] (float64; device tensors are read in
    place) are averaged into ``volume`` in the order 0 .. n-1.  ``found`` int [n]: a map whose entry is 0 is skipped (a device
    tensor is read in place); ``weights`` [n] > 0: the weight of each map's observations (1).  More than 32 maps go in calls of
    32.  -> info int32 device tensor [n,4] = (integrated, voxels updated, voxels whose pixel held a valid depth, 0)."""
    _check_volume(volume)
    depths, ks, rows, found, weights = _capture_args(volume, depths, Ks, c2ws, found, weights)
    with torch.cuda.device(volume.device):
        lib = _lib.load_library()
        infos = [_enqueue_integrate(lib, volume, depths[a:a + MAX_CAPTURES], ks[a:a + MAX_CAPTURES], rows[a:a + MAX_CAPTURES],
                                    None if found is None else found[a:a + MAX_CAPTURES], None if weights is None else weights[a:a + MAX_CAPTURES])
                 for a in range(0, len(ks), MAX_CAPTURES)]
    return infos[0] if len(infos) == 1 else torch.cat(infos)


def _enqueue_integrate_colors(lib, volume, depths, images, ks, c2ws, found, weights):
    """as ``_enqueue_integrate``, with ``images`` uint8 [n,H,W,3] and a volume that holds colour -> info int32 [n,4]"""
    n, H, W = (int(v) for v in depths.shape)
    info, = _args.empty(volume.device, ((n, 4), I32))
    K = (ctypes.c_double * (9 * n))(*[v for k in ks for v in k])
    w = None if weights is None else (ctypes.c_double * n)(*weights)
    check_op(lib.cotr_tsdf_color_integrate(*_color_args(volume), volume.trunc, ptr(depths), ptr(images), n, H, W, K, ptr(c2ws), ptr(found), w,
                                           volume.max_weight, ptr(info), _lib.current_stream_ptr()), 'cotr_tsdf_color_integrate')
    return info


def integrate_colors(volume, depths, images, Ks, c2ws, found=None, weights=None):
    """``cotr_tsdf_color_integrate`` on the current stream: the images ``images`` uint8 [n,H,W,3] of the depth maps ``depths``
    averaged into ``volume.color`` (a volume made with ``color=True``) where a voxel lies within ``trunc`` of the surface its pixel
    saw; every other argument as in ``integrate_depths``, whose call it neither needs nor disturbs: ``tsdf`` and ``weight`` are not
    read.  More than 32 maps go in calls of 32.  -> info int32 device tensor [n,4] = (integrated, voxels coloured, voxels whose
    pixel held a valid depth, 0)."""
    _check_color_volume(volume)
    depths, ks, rows, found, weights, images = _capture_args(volume, depths, Ks, c2ws, found, weights, images)
    with torch.cuda.device(volume.device):
        lib = _lib.load_library()
        infos = [_enqueue_integrate_colors(lib, volume, depths[a:a + MAX_CAPTURES], images[a:a + MAX_CAPTURES], ks[a:a + MAX_CAPTURES],
                                           rows[a:a + MAX_CAPTURES], None if found is None else found[a:a + MAX_CAPTURES],
                                           None if weights is None else weights[a:a + MAX_CAPTURES])
                 for a in range(0, len(ks), MAX_CAPTURES)]
    return infos[0] if len(infos) == 1 else torch.cat(infos)


def fuse_captures(caps, volume=None, origin=None, voxel=None, dims=None, weights=None, **kw):
    """The posed RGB-D captures ``caps`` (``cotr_amd.data.Capture``: image, depth, K, c2w) averaged into ``volume``, or into a
    fresh ``TsdfVolume(origin, voxel, dims, **kw)`` (``kw``: trunc, max_weight, device, color), in list order; neighbours of one
    depth-map size share a call.  The image is read only by a volume that holds colour (``color=True``): each depth call is then
    followed by ``cotr_tsdf_color_integrate`` on the same arguments, and every capture needs its image uint8 [H,W,3].
    -> (volume, one dict(integrated, updated, valid) per capture, with ``colored`` for a volume that holds colour)."""
    caps = list(caps)
    if not caps:
        raise ValueError('fuse_captures needs at least one capture')
    for cap in caps:
        _args.check_depth(cap.depth)
        _args.camera(cap.K, 'K')
        if _args.pose_matrix(cap.c2w) is None:
            raise ValueError('c2w must be a finite [4, 4] matrix, got None')
    if weights is not None and len(weights) != len(caps):
        raise ValueError(f'weights must be [{len(caps)}], got {len(weights)}')
    _args.no_cpu_tensors('the TSDF volume runs', *[cap.depth for cap in caps])
    colored = bool(kw.get('color', False)) if volume is None else getattr(volume, 'color', None) is not None
    if colored:
        for cap in caps:
            if cap.image is None:
                raise ValueError('a volume that holds colour needs the image of every capture, got None')
            _check_images(cap.image, cap.depth.shape, 'image')
        _args.no_cpu_tensors('the TSDF volume runs', *[cap.image for cap in caps])
    if volume is None:
        if origin is None or voxel is None or dims is None:
            raise ValueError('fuse_captures needs a volume, or origin, voxel and dims for a fresh one')
        volume = TsdfVolume(origin, voxel, dims, **kw)
    elif kw or origin is not None or voxel is not None or dims is not None:
        raise ValueError('origin, voxel, dims, trunc, max_weight and device describe a fresh volume: give them or a volume, not both')
    _check_volume(volume)
    infos, cinfos, a = [], [], 0
    while a < len(caps):
        b = a + 1
        while b < len(caps) and b - a < MAX_CAPTURES and tuple(caps[b].depth.shape) == tuple(caps[a].depth.shape):
            b += 1
        depths = torch.stack([on(cap.depth, volume.device) for cap in caps[a:b]])
        args = (np.stack([np.asarray(cap.K, np.float64) for cap in caps[a:b]]), [cap.c2w for cap in caps[a:b]])
        infos.append(integrate_depths(volume, depths, *args, weights=None if weights is None else weights[a:b]))
        if colored:
            images = torch.stack([on(cap.image, volume.device) for cap in caps[a:b]])
            cinfos.append(integrate_colors(volume, depths, images, *args, weights=None if weights is None else weights[a:b]))
        a = b
    rows = torch.cat(infos).cpu().numpy()
    out = [dict(integrated=bool(r[0]), updated=int(r[1]), valid=int(r[2])) for r in rows]
    if colored:
        for d, r in zip(out, torch.cat(cinfos).cpu().numpy()):
            d['colored'] = int(r[1])
    return volume, out


def _enqueue_raycast(lib, volume, k, c2w, found, H, W, near, far, step, normals):
    """``c2w`` float64 [16] and ``found`` on the volume's device already, every argument checked -> the dict of ``raycast_volume``"""
    depth, info = _args.empty(volume.device, ((H, W), torch.float32), (4, I32))
    out = dict(depth=depth, info=info)
    if normals:
        out['normals'], = _args.empty(volume.device, ((H, W, 3), F64))
    check_op(lib.cotr_tsdf_raycast(*_volume_args(volume), k, ptr(c2w), ptr(found), H, W, float(near), float(far), float(step), ptr(depth),
                                   ptr(out.get('normals')), ptr(info), _lib.current_stream_ptr()), 'cotr_tsdf_raycast')
    return out


def _enqueue_color_map(lib, volume, depth, k, c2w, found):
    """``depth`` float32 [H,W], ``c2w`` float64 [16] and ``found`` on the volume's device already, every argument checked, a volume
    that holds colour -> (rgb uint8 [H,W,3], info int32 [4])"""
    H, W = (int(v) for v in depth.shape)
    rgb, info = _args.empty(volume.device, ((H, W, 3), torch.uint8), (4, I32))
    check_op(lib.cotr_tsdf_color_map(*_color_args(volume), ptr(depth), H, W, k, ptr(c2w), ptr(found), ptr(rgb), ptr(info), _lib.current_stream_ptr()),
             'cotr_tsdf_color_map')
    return rgb, info


def _ray_args(volume, c2w, shape, near, far, step):
    """-> (the pose as float64 [16] where it was, H, W, near, far, step) with the defaults filled in and every rule checked"""
    _check_volume(volume)
    if len(shape) != 2:
        raise ValueError(f'shape must be (H, W), got {shape}')
    H, W = shape
    _args.check_int_range('H', H, 1, 1 << 28)
    _args.check_int_range('W', W, 1, 1 << 28)
    if int(H) * int(W) > 1 << 28:
        raise ValueError(f'shape: at most 2^28 pixels, got {H} x {W}')
    near = 0.0 if near is None else near
    step = volume.trunc / 2 if step is None else step
    if not (near >= 0 and np.isfinite(near)):
        raise ValueError(f'near must be finite and >= 0, got {near}')
    _args.check_positive('step', step)
    if torch.is_tensor(c2w) and c2w.is_cuda:
        if c2w.dtype != F64 or c2w.numel() != 16:
            raise ValueError(f'c2w on the device must be float64 [4, 4], got {c2w.dtype} {list(c2w.shape)}')
        if far is None:
            raise ValueError('far must be given when c2w is a device tensor: its default is worked out from the pose on the host')
        pose = c2w.reshape(16)
    else:
        m = _args.pose_matrix(c2w)
        if m is None:
            raise ValueError('c2w must be a finite [4, 4] matrix, got None')
        if far is None:
            far = float(np.linalg.norm(volume.corners() - m[:3, 3], axis=1).max())
            far = max(far, near + step)
        pose = torch.from_numpy(m.reshape(16))
    if not (far > near and np.isfinite(far)):
        raise ValueError(f'far must be finite and > near, got {far}')
    if np.ceil((far - near) / step) > MAX_STEPS:
        raise ValueError(f'at most 65536 steps from near to far, got {np.ceil((far - near) / step):.0f}')
    return pose, int(H), int(W), float(near), float(far), float(step)


def raycast_volume(volume, K, c2w, shape, near=None, far=None, step=None, normals=False, colors=False):
    """``cotr_tsdf_raycast`` on the current stream: ``volume`` seen from the camera-to-world pose ``c2w`` [4,4] (float64; a
    device tensor is read in place) through the camera ``K`` [3,3] at ``shape`` = (H, W): every ray walks from ``near`` (0) to
    ``far`` in steps of ``step`` (half the truncation distance) to the first crossing from in front of the surface to behind
    it.  ``far`` defaults to the largest distance from the camera centre to a corner of the volume, worked out on the host: it
    must be given with a device ``c2w``.  -> dict of device tensors: depth float32 [H,W] (0 where no surface is hit: a valid
    input of ``icp_depth``, ``lift_pixels`` and ``integrate_depths``), info int32 [4] = (ok, pixels hit, rays ended at a back
    face, 0), with ``normals=True`` normals float64 [H,W,3] in the camera frame (NaN where there is none), with ``colors=True`` (a
    volume that holds colour) rgb uint8 [H,W,3]: ``cotr_tsdf_color_map`` of that depth map, enqueued behind the raycast in the
    same device sequence ((0, 0, 0) where no surface is hit or none of the cell's corners is coloured)."""
    k = _args.camera(K, 'K')
    pose, H, W, near, far, step = _ray_args(volume, c2w, shape, near, far, step)
    if colors:
        _check_color_volume(volume)
    _args.no_cpu_tensors('the TSDF volume runs', c2w)
    with torch.cuda.device(volume.device):
        lib, pose = _lib.load_library(), on(pose, volume.device)
        out = _enqueue_raycast(lib, volume, k, pose, None, H, W, near, far, step, normals)
        if colors:
            out['rgb'] = _enqueue_color_map(lib, volume, out['depth'], k, pose, None)[0]
        return out


def color_depth_map(volume, depth, K, c2w):
    """``cotr_tsdf_color_map`` on the current stream: the colour of ``volume`` (made with ``color=True``) at the pixels of the
    depth map ``depth`` float32 [H,W] seen through the camera ``K`` [3,3] from the camera-to-world pose ``c2w`` [4,4] (float64; a
    device tensor is read in place): each pixel with a finite depth > 0 is lifted into the world and takes the blend of the
    coloured corners of its cell.  -> dict of device tensors: rgb uint8 [H,W,3] ((0, 0, 0) where there is no depth or no colour),
    info int32 [4] = (ok, pixels coloured, pixels with a depth, 0)."""
    _check_color_volume(volume)
    _args.check_depth(depth)
    k = _args.camera(K, 'K')
    if torch.is_tensor(c2w) and c2w.is_cuda:
        if c2w.dtype != F64 or c2w.numel() != 16:
            raise ValueError(f'c2w on the device must be float64 [4, 4], got {c2w.dtype} {list(c2w.shape)}')
        pose = c2w.reshape(16)
    else:
        m = _args.pose_matrix(c2w)
        if m is None:
            raise ValueError('c2w must be a finite [4, 4] matrix, got None')
        pose = torch.from_numpy(m.reshape(16))
    _args.no_cpu_tensors('the TSDF volume runs', depth, c2w)
    with torch.cuda.device(volume.device):
        rgb, info = _enqueue_color_map(_lib.load_library(), volume, on(depth, volume.device), k, on(pose, volume.device), None)
    return dict(rgb=rgb, info=info)


def sample_colors(volume, points):
    """``cotr_tsdf_color_points`` on the current stream: the colour of ``volume`` (made with ``color=True``) at the world points
    ``points`` [n,3] (a device tensor is read in place when it is float64; n may be 0), such as the vertices ``extract_mesh``
    returns: the blend of the coloured corners of each point's cell, the volume's faces included.  -> (rgb uint8 [n,3], valid bool
    [n]), device tensors; an invalid point - outside the volume, NaN, or in a cell with no coloured corner - is (0, 0, 0)."""
    _check_color_volume(volume)
    pts = _args.points(points, 'points', 3)
    n = int(pts.shape[0])
    if n > MAX_VOXELS:
        raise ValueError(f'at most 2^28 points, got {n}')
    _args.no_cpu_tensors('the TSDF volume runs', points)
    device = volume.device
    with torch.cuda.device(device):
        pts = on(pts, device)
        rgb, valid, info = _args.empty(device, ((n, 3), torch.uint8), (n, torch.uint8), (4, I32))
        check_op(_lib.load_library().cotr_tsdf_color_points(*_color_args(volume), ptr(pts) if n else None, n, None, ptr(rgb) if n else None,
                                                            ptr(valid) if n else None, ptr(info), _lib.current_stream_ptr()), 'cotr_tsdf_color_points')
    return rgb, valid.bool()


def _check_mesh_volume(volume):
    _check_volume(volume)
    Nx, Ny, Nz = volume.dims
    if Nx * Ny * Nz > MAX_MESH_VOXELS:
        raise ValueError(f'extract_mesh: at most 2^27 voxels (12 triangles a cell in an int32), got {Nx} x {Ny} x {Nz}')


def _enqueue_mesh(lib, volume, found, max_verts, max_tris, normals, scratch=None):
    """``found`` on the volume's device already, every argument checked -> (verts [max_verts,3], tris [max_tris,3], normals or
    None, info int32 [4]), device tensors; ``scratch``: what ``_args.scratch`` returned for this volume, to use it again"""
    device = volume.device
    buf, nbytes = scratch if scratch is not None else _args.scratch(lib, 'cotr_tsdf_mesh_scratch_bytes', *volume.dims, device=device)
    verts, tris, info = _args.empty(device, ((max_verts, 3), F64), ((max_tris, 3), I32), (4, I32))
    nrm = _args.empty(device, ((max_verts, 3), F64))[0] if normals else None
    check_op(lib.cotr_tsdf_mesh(*_volume_args(volume), ptr(found), ptr(verts) if max_verts else None, max_verts, ptr(nrm) if max_verts else None,
                                ptr(tris) if max_tris else None, max_tris, ptr(info), ptr(buf), nbytes, _lib.current_stream_ptr()), 'cotr_tsdf_mesh')
    return verts, tris, nrm, info


def extract_mesh(volume, max_verts=None, max_tris=None, normals=False):
    """``cotr_tsdf_mesh`` on the current stream: the surface of ``volume`` (at most 2^27 voxels) as an indexed triangle mesh by
    marching tetrahedra, closed and oriented outwards (towards tsdf > 0) wherever the cells around it have been
    observed.  With ``max_verts`` and ``max_tris`` both given it is one capturable call with no host wait: the tensors come
    back padded to the capacities (what lies beyond one is counted in ``info`` but not written; the rows of ``tris`` past the
    count are -1, those of ``verts`` and ``normals`` are not written) and ``info`` stays on the device.  With both ``None`` a first
    call only counts, the two counts are read on the host (the one host wait) and a second call writes tensors of exactly that
    size.  -> (verts float64 [V,3] in the world frame, tris int32 [T,3], normals float64 [V,3] (NaN where the volume around the
    vertex is not observed) or None, info int32 device tensor [4] = (ok, vertices, triangles, valid cells))."""
    _check_mesh_volume(volume)
    if (max_verts is None) != (max_tris is None):
        raise ValueError('max_verts and max_tris go together: give both for one capturable call, or neither for an exact mesh')
    if max_verts is not None:
        _args.check_int_range('max_verts', max_verts, 0, (1 << 31) - 1)
        _args.check_int_range('max_tris', max_tris, 0, (1 << 31) - 1)
    with torch.cuda.device(volume.device):
        lib = _lib.load_library()
        if max_verts is not None:
            return _enqueue_mesh(lib, volume, None, int(max_verts), int(max_tris), normals)
        scratch = _args.scratch(lib, 'cotr_tsdf_mesh_scratch_bytes', *volume.dims, device=volume.device)
        counts = _enqueue_mesh(lib, volume, None, 0, 0, False, scratch)[3].cpu().numpy()   # the host wait
        return _enqueue_mesh(lib, volume, None, int(counts[1]), int(counts[2]), normals, scratch)


def write_ply(path, verts, tris, normals=None, colors=None):
    """A binary little-endian PLY file of the mesh ``extract_mesh`` returned (tensors or arrays): float64 x, y, z (and nx, ny,
    nz, and with ``colors`` uint8 [V,3], as ``sample_colors`` returns them, uchar red, green, blue) per vertex, a uchar count and
    three int32 indices per face.  Triangle rows of -1 (the padding of a fixed capacity) are dropped; with padded vertices pass
    ``verts[:V]``.  A host helper: device tensors are copied first."""
    host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)   # noqa: E731
    v, t = np.ascontiguousarray(host(verts), dtype='<f8'), np.asarray(host(tris))
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f'verts must be [V, 3], got shape {v.shape}')
    if t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in 'iu':
        raise ValueError(f'tris must be integers [T, 3], got {t.dtype} {t.shape}')
    t = t[(t != -1).all(1)]
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError(f'tris refers to vertices outside [0, {len(v)})')
    cols = [v]
    if normals is not None:
        n = np.ascontiguousarray(host(normals), dtype='<f8')
        if n.shape != v.shape:
            raise ValueError(f'normals must be [V, 3] like verts, got shape {n.shape}')
        cols.append(n)
    rows = np.ascontiguousarray(np.hstack(cols))
    if colors is not None:
        c = np.asarray(host(colors))
        if c.shape != v.shape or c.dtype != np.uint8:
            raise ValueError(f'colors must be uint8 [V, 3] like verts, got {c.dtype} {c.shape}')
        packed = np.empty(len(v), dtype=[('d', '<f8', (rows.shape[1],)), ('c', 'u1', (3,))])
        packed['d'], packed['c'] = rows, c
        rows = packed
    faces = np.empty(len(t), dtype=[('n', 'u1'), ('v', '<i4', (3,))])
    faces['n'], faces['v'] = 3, t
    header = ['ply', 'format binary_little_endian 1.0', f'element vertex {len(v)}'] + [f'property double {c}' for c in 'xyz']
    header += [f'property double n{c}' for c in 'xyz'] if normals is not None else []
    header += [f'property uchar {c}' for c in ('red', 'green', 'blue')] if colors is not None else []
    header += [f'element face {len(t)}', 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as f:
        f.write(('\n'.join(header) + '\n').encode('ascii'))
        f.write(rows.tobytes())
        f.write(faces.tobytes())


def track_capture(volume, cap, c2w0, max_dist=0.05, near=None, far=None, step=None, normal_cos=icp.NORMAL_COS, edge=icp.EDGE,
                  cond_tol=icp.COND_TOL, iters=10, stride=1):
    """Frame-to-model tracking: ``volume`` is raycast at the predicted pose ``c2w0`` [4,4] with the camera and map size of the
    RGB-D capture ``cap`` (its c2w is not read), and ``icp_depth`` refines ``c2w0`` with that map as A and ``cap.depth`` as B, in
    one device sequence -> (c2w float64 [4,4], info) as ``refine_registration`` returns them."""
    _args.check_map(cap.depth, 'cap.depth')
    k = _args.camera(cap.K, 'K')
    start = _args.pose_matrix(c2w0)
    pose, H, W, near, far, step = _ray_args(volume, start, tuple(cap.depth.shape), near, far, step)
    icp.check(max_dist, normal_cos, edge, cond_tol, iters, stride)
    _args.no_cpu_tensors('the TSDF volume runs', cap.depth)
    device = volume.device
    with torch.cuda.device(device):
        lib = _lib.load_library()
        pose = on(pose, device)
        model = _enqueue_raycast(lib, volume, k, pose, None, H, W, near, far, step, False)
        R0, t0 = on(np.ascontiguousarray(start[:3, :3]).reshape(9), device), on(np.ascontiguousarray(start[:3, 3]), device)
        r = _enqueue_icp(lib, model['depth'], k, on(cap.depth, device), k, R0, t0, pose, None, None, max_dist, normal_cos, edge, cond_tol, iters,
                         stride, False, device)
    return icp.host_result(r)
