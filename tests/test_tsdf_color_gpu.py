"""The colour volume on the MI355X (cotr_amd/csrc/tsdf.hip) against the numpy restatement tests/tsdf_color_oracle.py: the colour
volume after every integration, the bytes of every sampled point and of every coloured depth map bit for bit, the counts
exactly, at the smallest sizes at which the indexing can go wrong; the ``found`` gate, the guard bands, repeatability, and the
wrappers on top.

Voxels, points and pixels the restatement flags as near a decision (within 1e-9) are left out of a comparison, at most 0.1 % of
a case; every case prints its share.  The accuracy figures - the colour at the mesh vertices and in the raycast from A's pose
against the texture the images were made from - are held to 1.5 times the restatement's own figure on the same case (the
family's factor, as tests/test_tsdf_gpu.py).  Measured figures: DESIGN.md 3h-14."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.data import Capture
from cotr_amd.inference import (TsdfVolume, ZoomEngine, color_depth_map, extract_mesh, fuse_captures, integrate_colors, integrate_depths, raycast_volume,
                                sample_colors, write_ply)
from cotr_amd.inference import _args, tsdf as tsdf_mod
from tests import icp_oracle as io
from tests import pnp_oracle as po
from tests import tsdf_color_oracle as tc
from tests import tsdf_oracle as to
from tests.guard_arena import Arena

pytestmark = pytest.mark.gpu

CAP = 0.001
VOLUMES = ((2, 2, 2), (3, 5, 7), (4, 4, 4), (7, 3, 3), (65, 2, 2), (67, 3, 2), (8, 8, 8), (64, 64, 64))
ALL_IN_BAND = ((2, 2, 2), (4, 4, 4), (7, 3, 3))
MAPS = ((24, 32), (48, 64))
SHAPES = ((1, 1), (3, 3), (7, 9), (8, 8), (5, 13), (48, 64))
COUNTS = (0, 1, 63, 64, 65, 257)


def origin_of(dims):
    return to.ORIGIN_64 if dims == (64, 64, 64) else to.small_origin(dims)


def same_color(vol, o, what):
    """the device's colour volume against the restatement's, outside the flagged voxels -> their share"""
    torch.cuda.synchronize()
    C = vol.color.cpu().numpy()
    keep, share = ~o['near'], to.share(o['near'])
    assert share <= CAP, (what, share)
    assert C.shape == o['color'].shape and C.dtype == np.float32 and np.array_equal(C[keep], o['color'][keep]), what
    return share


def same_bytes(rgb, valid, o, what):
    """sampled bytes against the restatement's (rgb, valid, near) -> the share of flagged elements"""
    keep, share = ~o[2], to.share(o[2]) if o[2].size else 0.0
    assert share <= CAP, (what, share)
    assert rgb.dtype == np.uint8 and rgb.shape == o[0].shape and np.array_equal(rgb[keep], o[0][keep]), what
    assert valid is None or np.array_equal(valid[keep], o[1][keep]), what
    return share


def color_both(vol, state, depths, images, Ks, c2ws, found=None, weights=None, on_device=False):
    """one call on the device (``on_device``: poses and ``found`` as device tensors) and in the restatement (from the colour
    ``state``) -> (info of the device, the restatement's dict)"""
    f = None if found is None else (torch.tensor(found, dtype=torch.int32, device='cuda') if on_device else np.asarray(found))
    info = integrate_colors(vol, depths, images, Ks, torch.from_numpy(c2ws).cuda() if on_device else c2ws, found=f, weights=weights).cpu().numpy()
    o = tc.integrate(state, vol.origin, vol.voxel, vol.trunc, depths, images, Ks, c2ws, found=found, weights=weights, max_weight=vol.max_weight)
    return info, o


# ---- integration ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', MAPS, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('dims', VOLUMES, ids=lambda d: 'x'.join(str(v) for v in d))
def test_integration_at_every_size_with_a_second_call_and_the_cap(dims, shape):
    depths, Ks, c2ws = to.captures(*shape)
    images = tc.images(*shape)
    vol = TsdfVolume(origin_of(dims), to.VOXEL_64, dims, max_weight=3.0, color=True)
    assert (vol.color == 0).all() and tuple(vol.color.shape) == dims[::-1] + (4,) and vol.color.dtype == torch.float32
    assert TsdfVolume(origin_of(dims), to.VOXEL_64, dims).color is None
    info, o = color_both(vol, tc.fresh(dims), depths, images, Ks, c2ws)
    share = same_color(vol, o, 'first call')
    assert np.array_equal(info, o['info']) and (info[:, 1] > 0).all(), (info, o['info'])
    assert (info[:, 1] == info[:, 2]).all() if dims in ALL_IN_BAND else (info[:, 1] < info[:, 2]).all(), info
    # neither tsdf nor weight was touched, and the depth call reports the same third column
    assert (vol.tsdf == 1).all() and (vol.weight == 0).all()
    assert np.array_equal(integrate_depths(vol, depths, Ks, c2ws).cpu().numpy()[:, 2], info[:, 2])
    # the same captures again with other weights: accumulation, and the cap at 3
    info2, o2 = color_both(vol, o['color'], depths, images, Ks, c2ws, weights=[1.5, 0.75])
    o2['near'] |= o['near']
    share2 = same_color(vol, o2, 'second call')
    assert np.array_equal(info2, o2['info']) and np.array_equal(info2, info)
    assert (o2['color'][..., 3] == 3.0).any() and (o2['color'][..., 3] <= 3.0).all() and not np.array_equal(o2['color'], o['color'])
    print(f'{dims} with maps {shape}: coloured {info[:, 1].tolist()} of valid {info[:, 2].tolist()}, flagged {100 * share:.4f} % / {100 * share2:.4f} % of the voxels')
    if dims == (64, 64, 64) and shape == (48, 64):
        assert info.tolist() == [[1, 16280, 119400, 0], [1, 13636, 97491, 0]]


@pytest.mark.parametrize('n', [1, 2, 3, 32])
@pytest.mark.parametrize('dims', [(8, 8, 8), (67, 3, 2)], ids=['8x8x8', '67x3x2'])
def test_captures_per_call(dims, n):
    depths, Ks, c2ws = to.captures(24, 32, n)
    images = tc.images(24, 32, n)
    weights = [1.0 + 0.25 * (c % 3) for c in range(n)]
    vol = TsdfVolume(origin_of(dims), to.VOXEL_64, dims, max_weight=20.0, color=True)
    info, o = color_both(vol, tc.fresh(dims), depths, images, Ks, c2ws, weights=weights)
    share = same_color(vol, o, f'{n} captures')
    assert info.shape == (n, 4) and np.array_equal(info, o['info']) and (info[:, 0] == 1).all()
    assert (o['color'][..., 3] == 20.0).any() == (n == 32)
    # and the same bits as n calls of one capture each
    one = TsdfVolume(origin_of(dims), to.VOXEL_64, dims, max_weight=20.0, color=True)
    rows = [integrate_colors(one, depths[c:c + 1], images[c:c + 1], Ks[c:c + 1], c2ws[c:c + 1], weights=weights[c:c + 1]) for c in range(n)]
    assert torch.equal(one.color, vol.color) and np.array_equal(torch.cat(rows).cpu().numpy(), info)
    print(f'{dims}, {n} captures in one call: flagged {100 * share:.4f} % of the voxels')


@pytest.mark.parametrize('on_device', [True, False], ids=['device', 'host'])
def test_found_skips_the_first_a_middle_and_the_last_capture(on_device):
    depths, Ks, c2ws = to.captures(24, 32, 5)
    images = tc.images(24, 32, 5)
    dims, found = (8, 8, 8), [0, 1, 0, 1, 0]
    vol = TsdfVolume(origin_of(dims), to.VOXEL_64, dims, color=True)
    info, o = color_both(vol, tc.fresh(dims), depths, images, Ks, c2ws, found=found, on_device=on_device)
    same_color(vol, o, 'found')
    assert np.array_equal(info, o['info']) and (info[[0, 2, 4]] == 0).all() and (info[[1, 3], 0] == 1).all() and (info[[1, 3], 1] > 0).all()
    # nothing found: the volume stays fresh
    vol.reset()
    info, _ = color_both(vol, tc.fresh(dims), depths, images, Ks, c2ws, found=[0] * 5, on_device=on_device)
    assert (info == 0).all() and (vol.color == 0).all()


def test_more_than_32_captures_go_in_calls_of_32():
    depths, Ks, c2ws = to.captures(24, 32, 35)
    images = tc.images(24, 32, 35)
    dims = (7, 3, 3)
    vol = TsdfVolume(origin_of(dims), to.VOXEL_64, dims, color=True)
    info, o = color_both(vol, tc.fresh(dims), depths, images, Ks, c2ws)
    same_color(vol, o, '35 captures')
    assert info.shape == (35, 4) and np.array_equal(info, o['info'])


def test_the_colour_call_and_the_depth_call_in_either_order():
    depths, Ks, c2ws = to.captures(48, 64)
    images = tc.images(48, 64)
    a, b = (TsdfVolume(to.ORIGIN_64, to.VOXEL_64, (64, 64, 64), color=True) for _ in range(2))
    ia = (integrate_depths(a, depths, Ks, c2ws), integrate_colors(a, depths, images, Ks, c2ws))
    ib = (integrate_colors(b, depths, images, Ks, c2ws), integrate_depths(b, depths, Ks, c2ws))
    assert torch.equal(a.tsdf, b.tsdf) and torch.equal(a.weight, b.weight) and torch.equal(a.color, b.color)
    assert torch.equal(ia[0], ib[1]) and torch.equal(ia[1], ib[0]) and torch.equal(ia[0][:, 2], ia[1][:, 2])
    f = to.fused()
    assert np.array_equal(a.tsdf.cpu().numpy(), f['tsdf']) and np.array_equal(a.weight.cpu().numpy(), f['weight'])
    same_color(a, tc.fused(weights=None), 'after the depth call')


# ---- points ---------------------------------------------------------------------------------------------------------------
_FUSED = {}


def fused_volume():
    """the corner's two textured 48 x 64 captures in the 64^3 volume, depth and colour, integrated on the device once and checked
    against the restatements"""
    if 'vol' not in _FUSED:
        f = to.fused()
        vol = TsdfVolume(f['origin'], f['voxel'], f['dims'], color=True)
        integrate_depths(vol, *to.captures(48, 64))
        integrate_colors(vol, to.captures(48, 64)[0], tc.images(48, 64), *to.captures(48, 64)[1:], weights=tc.FUSED_WEIGHTS)
        same_color(vol, tc.fused(), 'the fused corner')
        assert np.array_equal(vol.tsdf.cpu().numpy(), f['tsdf'])
        _FUSED['vol'] = vol
    return _FUSED['vol']


def point_set():
    """257 points around the fused corner, of every kind in turn so that the first n hold a mix: voxel centres, points on the one
    face of this box that holds coloured voxels (x = 0; every face: test_points_on_every_face_edge_and_corner_of_a_box), points
    just outside it, NaN, points in cells with 8, with 1 to 7 and with no coloured corner -> (points float64 [257, 3], kind [257])"""
    col = tc.fused()['color'][..., 3] > 0
    corners = sum(col[dz:63 + dz, dy:63 + dy, dx:63 + dx].astype(np.int64) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
    rng = np.random.default_rng(12)
    cells = {name: np.argwhere(m)[:, ::-1] for name, m in (('full', corners == 8), ('part', (corners > 0) & (corners < 8)), ('none', corners == 0))}
    voxels = np.argwhere(col)[:, ::-1]
    centres = voxels[((voxels > 0) & (voxels < 63)).all(1)]
    on = voxels[voxels[:, 0] == 0]
    assert all(len(c) > 40 for c in cells.values()) and len(on) > 40
    p, kinds = [], []
    for a in range(257):
        kind = ('centre', 'full', 'face', 'part', 'outside', 'none', 'nan', 'part')[a % 8]
        if kind == 'centre':
            g = centres[rng.integers(len(centres))].astype(np.float64)
        elif kind == 'face':       # on the face, between the voxel centres of a coloured voxel's cell
            g = np.clip(on[rng.integers(len(on))] + rng.uniform(0.05, 0.95, 3), 0.0, 62.95)
            g[0] = 0.0             # origin + voxel * 0 is the origin itself: the grid coordinate comes back as 0 exactly
        elif kind == 'outside':    # just outside one face, inside on the other axes
            g = rng.uniform(1, 62, 3)
            g[a % 3] = (-1e-7, 63 + 1e-7, -0.5, 63.5)[(a // 8) % 4]
        elif kind == 'nan':
            g = rng.uniform(1, 62, 3)
            g[a % 3] = np.nan
        else:
            g = cells[kind][rng.integers(len(cells[kind]))] + rng.uniform(0.05, 0.95, 3)
        p.append(np.asarray(to.ORIGIN_64) + to.VOXEL_64 * g)
        kinds.append(kind)
    p, kinds = np.array(p), np.array(kinds)
    assert (((p - np.asarray(to.ORIGIN_64)) / to.VOXEL_64)[kinds == 'face'][:, 0] == 0).all()
    return p, kinds


@pytest.mark.parametrize('n', COUNTS)
def test_points_of_every_kind_at_every_count(n):
    vol, f = fused_volume(), tc.fused()
    p, kinds = point_set()
    p, kinds = p[:n], kinds[:n]
    rgb, valid = sample_colors(vol, torch.from_numpy(p).cuda() if n % 2 else p)
    torch.cuda.synchronize()
    assert valid.dtype == torch.bool and tuple(rgb.shape) == (n, 3) and tuple(valid.shape) == (n,)
    rgb, valid = rgb.cpu().numpy(), valid.cpu().numpy()
    o = tc.sample(f['color'], to.ORIGIN_64, to.VOXEL_64, p.reshape(n, 3))
    share = same_bytes(rgb, valid, o, f'{n} points')
    assert (rgb[~valid] == 0).all()
    if n:
        assert valid[kinds == 'centre'].all() and valid[kinds == 'full'].all()
    if n == 257:
        assert valid[kinds == 'face'].all() and valid[kinds == 'part'].all() and not valid[np.isin(kinds, ('outside', 'none', 'nan'))].any()
        assert (rgb[valid] > 0).all() and len(np.unique(rgb[valid], axis=0)) > 100
    print(f'{n} points: {int(valid.sum())} valid, flagged {100 * share:.4f} %')


def test_points_on_every_face_edge_and_corner_of_a_box():
    """a box whose origin and voxel are binary fractions, so that grid coordinates of 0 and N - 1 can be hit exactly on every axis
    (with the corner scene's origin -3.2 and voxel 0.1 no double comes back as 63: the grid coordinate steps over it), all of it
    inside the band of the far wall"""
    dims, voxel, origin = (8, 7, 6), 0.0625, (-0.21875, -0.1875, 5.84375)
    depths, Ks, c2ws = to.captures(48, 64)
    vol = TsdfVolume(origin, voxel, dims, trunc=0.3, color=True)
    info, o = color_both(vol, tc.fresh(dims), depths, tc.images(48, 64), Ks, c2ws, weights=tc.FUSED_WEIGHTS)
    same_color(vol, o, 'the box')
    assert (o['color'][..., 3] > 0).all() and not o['near'].any()
    # every combination of low face, inside and high face over the three axes but the one that is inside on all: 26 kinds, 5 of each
    rng = np.random.default_rng(21)
    g = np.array([[(0.0, rng.uniform(0.05, n - 1.05), n - 1.0)[k] for k, n in zip(kind, dims)]
                  for kind in np.ndindex(3, 3, 3) if kind != (1, 1, 1) for _ in range(5)])
    p = np.asarray(origin) + voxel * g
    on = (g == 0) | (g == np.asarray(dims) - 1.0)
    assert np.array_equal(((p - np.asarray(origin)) / voxel)[on], g[on]) and on.any(1).all()   # exactly on the faces
    out = np.asarray(origin) + voxel * np.where(g == 0, -2.0 ** -20, np.where(g == np.asarray(dims) - 1.0, g + 2.0 ** -20, g))   # and a hair outside them
    both = np.concatenate([p, out])
    rgb, valid = sample_colors(vol, both)
    rgb, valid = rgb.cpu().numpy(), valid.cpu().numpy()
    want = tc.sample(o['color'], origin, voxel, both)
    share = same_bytes(rgb, valid, want, 'the faces')
    assert valid[:130].all() and not valid[130:].any() and (rgb[130:] == 0).all() and (rgb[:130] > 0).all()
    print(f'130 points on the faces, edges and corners of an {dims} box and 130 a hair outside: flagged {100 * share:.4f} %')


def test_every_vertex_of_the_mesh_has_the_restatements_colour_and_both_are_near_the_texture():
    vol, f = fused_volume(), tc.fused()
    verts, tris, _, info = extract_mesh(vol)
    rgb, valid = sample_colors(vol, verts)
    v, rgb, valid = verts.cpu().numpy(), rgb.cpu().numpy(), valid.cpu().numpy()
    o = tc.sample(f['color'], to.ORIGIN_64, to.VOXEL_64, v)
    share = same_bytes(rgb, valid, o, 'the mesh vertices')
    # A vertex lies on an edge whose inside end has tsdf <= 0: a capture saw it at -trunc <= sdf <= 0, inside the band, so that end
    # is coloured, and it is a corner of the vertex's cell with beta > 0.  Only a vertex whose coordinate comes back beyond the
    # last voxel layer can be invalid.
    q = (v - np.asarray(to.ORIGIN_64)) / to.VOXEL_64
    inside = ((q > 0) & (q < 63)).all(1)
    assert len(v) == int(info[1]) > 10000 and valid[inside].all() and inside.mean() > 0.9
    # the raw call reports the count
    n, out = len(v), _args.empty(vol.device, ((len(v), 3), torch.uint8), (len(v), torch.uint8), (4, torch.int32))
    with torch.cuda.device(vol.device):
        rc = _lib.load_library().cotr_tsdf_color_points(*tsdf_mod._color_args(vol), _lib.ptr(verts), n, None, *(_lib.ptr(t) for t in out), _lib.current_stream_ptr())
    assert rc == 0 and out[2].tolist() == [1, int(valid.sum()), 0, 0] and np.array_equal(out[0].cpu().numpy(), rgb)
    e, w = tc.texture_error(rgb, valid, v), tc.texture_error(o[0], o[1], v)
    print(f'{len(v)} vertices, {int(valid.sum())} coloured, flagged {100 * share:.4f} %; against the texture: median {e[0].round(3).tolist()} '
          f'(restatement {w[0].round(3).tolist()}), p90 {e[1].round(3).tolist()} ({w[1].round(3).tolist()})')
    assert (e <= 1.5 * w).all() and (w[0] <= tc.GRADIENT * to.VOXEL_64).all()


# ---- maps -----------------------------------------------------------------------------------------------------------------
def camera(shape):
    """the first camera of the corner scene at ``shape``; below 16 pixels from inside the box, between its near face and the far
    wall, where the few rays there are all hit"""
    sc = io.corner_scene()
    pose = sc['c2w_a'].copy()
    if shape[0] * shape[1] < 16:
        pose[:3, 3] = (0.213, -0.107, 3.021)
    return io.scaled_camera(sc['K_a'], *shape), pose


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_maps_at_every_size_with_pixels_of_depth_0_nan_and_inf(shape):
    vol, f = fused_volume(), tc.fused()
    K, pose = camera(shape)
    depth = raycast_volume(vol, K, pose, shape, near=0.37, far=7.93, step=0.15)['depth']
    hit = torch.nonzero(depth.reshape(-1) > 0).reshape(-1)
    assert len(hit) >= 1
    if len(hit) >= 4:              # three of the pixels that were hit, spread over the map
        for at, bad in zip((hit[0], hit[len(hit) // 2], hit[-1]), (0.0, float('nan'), float('inf'))):
            depth.reshape(-1)[at] = bad
    r = color_depth_map(vol, depth if shape[0] % 2 else depth.cpu().numpy(), K, torch.from_numpy(pose).cuda() if shape[1] % 2 else pose)
    torch.cuda.synchronize()
    rgb, info = r['rgb'].cpu().numpy(), r['info'].cpu().numpy()
    d = depth.cpu().numpy()
    o = tc.color_map(f['color'], to.ORIGIN_64, to.VOXEL_64, d, K, pose)
    share = same_bytes(rgb, None, (o['rgb'], None, o['near']), f'{shape}')
    if not o['near'].any():
        assert np.array_equal(info, o['info']), (info, o['info'])
    has = (d > 0) & np.isfinite(d)
    assert rgb.shape == shape + (3,) and (rgb[~has] == 0).all() and info[0] == 1 and info[2] == has.sum() and 0 < info[1] <= info[2]
    if len(hit) >= 4:
        assert has.sum() == len(hit) - 3
    print(f'{shape}: info {info.tolist()}, flagged {100 * share:.4f} % of the pixels')


def test_found_0_zeroes_every_output_of_the_map_and_of_the_points():
    vol = fused_volume()
    K, pose = camera((7, 9))
    k, c2w = _args.camera(K, 'K'), torch.from_numpy(pose.reshape(16)).cuda()
    depth = raycast_volume(vol, K, pose, (7, 9), near=0.37, far=7.93, step=0.15)['depth']
    zero, one = torch.zeros(1, dtype=torch.int32, device='cuda'), torch.ones(1, dtype=torch.int32, device='cuda')
    with torch.cuda.device(vol.device):
        lib = _lib.load_library()
        off, on_, free = (tsdf_mod._enqueue_color_map(lib, vol, depth, k, c2w, fl) for fl in (zero, one, None))
        p = torch.from_numpy(point_set()[0][:65]).cuda()
        outs = []
        for fl in (zero, one, None):
            rgb, valid, info = torch.full((65, 3), 9, dtype=torch.uint8, device='cuda'), torch.full((65,), 9, dtype=torch.uint8, device='cuda'), \
                torch.full((4,), 9, dtype=torch.int32, device='cuda')
            assert lib.cotr_tsdf_color_points(*tsdf_mod._color_args(vol), _lib.ptr(p), 65, _lib.ptr(fl), _lib.ptr(rgb), _lib.ptr(valid), _lib.ptr(info),
                                              _lib.current_stream_ptr()) == 0
            outs.append((rgb, valid, info))
    for a in range(2):
        assert (off[a] == 0).all() and torch.equal(on_[a], free[a])
    assert free[1][0] == 1 and free[1][1] > 0
    for a in range(3):
        assert (outs[0][a] == 0).all() and torch.equal(outs[1][a], outs[2][a])
    assert outs[2][2].tolist() == [1, int(outs[2][1].sum()), 0, 0] and outs[2][1].sum() > 20


# ---- bounds ---------------------------------------------------------------------------------------------------------------
FILL = 0xA5


def test_each_entry_point_stays_inside_what_it_was_given():
    """one raw call of each entry point with every buffer between two guard bands, at the least alignment the header promises"""
    lib = _lib.load_library()
    dims, shape, n = (67, 3, 2), (24, 32), 3
    depths, Ks, c2ws = to.captures(*shape, n)
    images = tc.images(*shape, n)
    origin = origin_of(dims)
    o = tc.integrate(tc.fresh(dims), origin, to.VOXEL_64, 0.3, depths, images, Ks, c2ws)
    O3, K3 = (ctypes.c_double * 3)(*origin), (ctypes.c_double * (9 * n))(*Ks.reshape(-1))
    here = _lib.current_stream_ptr()
    a = Arena('cuda', FILL).add('color', o['color'].nbytes, 'a16').add_input('depths', depths).add_input('images', images)
    a.add_input('c2w', c2ws.reshape(n, 16)).add_output('info', np.int32, (n, 4)).build()
    a.raw('color').zero_()           # a fresh colour volume
    assert a.addr('color') % 32 == 16 and a.addr('images') % 2 == 1
    rc = lib.cotr_tsdf_color_integrate(a.ptr('color'), *dims, O3, to.VOXEL_64, 0.3, a.ptr('depths'), a.ptr('images'), n, *shape, K3, a.ptr('c2w'), None, None,
                                       64.0, a.ptr('info'), here)
    assert rc == 0, lib.cotr_raster_last_error()
    torch.cuda.synchronize()
    a.check()
    assert np.array_equal(a.view('color', np.float32, o['color'].shape), o['color']) and np.array_equal(a.view('info', np.int32, (n, 4)), o['info'])
    # the points and the map on the fused corner: 65 points of every kind, the last workgroup a partial one
    color, dims, O3 = tc.fused()['color'], (64, 64, 64), (ctypes.c_double * 3)(*to.ORIGIN_64)
    p = point_set()[0][:65]
    want = tc.sample(color, to.ORIGIN_64, to.VOXEL_64, p)
    b = Arena('cuda', FILL).add_input('color', color, kind='a16').add_input('points', p).add_output('rgb', np.uint8, (65, 3))
    b.add_output('valid', np.uint8, (65,)).add_output('info', np.int32, (4,)).build()
    rc = lib.cotr_tsdf_color_points(b.ptr('color'), *dims, O3, to.VOXEL_64, b.ptr('points'), 65, None, b.ptr('rgb'), b.ptr('valid'), b.ptr('info'), here)
    assert rc == 0, lib.cotr_raster_last_error()
    torch.cuda.synchronize()
    b.check()
    assert not want[2].any() and 20 < want[1].sum() < 65
    assert np.array_equal(b.view('rgb', np.uint8, (65, 3)), want[0]) and np.array_equal(b.view('valid', np.uint8, (65,)), want[1].astype(np.uint8))
    assert b.view('info', np.int32, (4,)).tolist() == [1, int(want[1].sum()), 0, 0]
    # the map: 5 x 13 of the scene's renderer, one tile of 16 x 16 with most of its threads outside the image
    sc = io.corner_scene()
    Km, pose = io.scaled_camera(sc['K_a'], 5, 13), sc['c2w_a']
    d = io.render(5, 13, Km, pose, io.PLANES)
    d[0, 0], d[4, 12] = np.nan, 0.0
    wantm = tc.color_map(color, to.ORIGIN_64, to.VOXEL_64, d, Km, pose)
    c = Arena('cuda', FILL).add_input('color', color, kind='a16').add_input('depth', d).add_input('c2w', pose.reshape(16))
    c.add_output('rgb', np.uint8, (5, 13, 3)).add_output('info', np.int32, (4,)).build()
    rc = lib.cotr_tsdf_color_map(c.ptr('color'), *dims, O3, to.VOXEL_64, c.ptr('depth'), 5, 13, _args.camera(Km, 'K'), c.ptr('c2w'), None, c.ptr('rgb'),
                                 c.ptr('info'), here)
    assert rc == 0, lib.cotr_raster_last_error()
    torch.cuda.synchronize()
    c.check()
    assert not wantm['near'].any() and np.array_equal(c.view('rgb', np.uint8, (5, 13, 3)), wantm['rgb'])
    assert np.array_equal(c.view('info', np.int32, (4,)), wantm['info']) and 20 < wantm['info'][1] <= wantm['info'][2] <= 63
    print(f'points {b.view("info", np.int32, (4,)).tolist()}, map {wantm["info"].tolist()}')


# ---- repeatability ----------------------------------------------------------------------------------------------------------
def test_same_bits_across_calls_streams_and_graph_replay():
    f, vol = tc.fused(), fused_volume()
    depths, Ks, c2ws = to.captures(48, 64)
    K, pose = camera((48, 64))
    lib = _lib.load_library()
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    d_dev, i_dev, c_dev, pose_dev = cu(depths), cu(tc.images(48, 64)), cu(c2ws.reshape(2, 16)), cu(pose.reshape(16))
    verts = extract_mesh(vol)[0]
    model = raycast_volume(vol, K, pose, (48, 64), near=0.37, far=7.93, step=0.15)['depth']
    n = int(verts.shape[0])
    K2, K1, W2 = (ctypes.c_double * 18)(*Ks.reshape(-1)), _args.camera(K, 'K'), (ctypes.c_double * 2)(*tc.FUSED_WEIGHTS)
    origin = (ctypes.c_double * 3)(*to.ORIGIN_64)
    torch.cuda.synchronize()

    def buffers():
        full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device='cuda')   # noqa: E731
        return dict(color=torch.zeros((64, 64, 64, 4), dtype=torch.float32, device='cuda'), info=full((2, 4), -3, torch.int32), rgb=full((n, 3), 7, torch.uint8),
                    valid=full((n,), 7, torch.uint8), pinfo=full((4,), -3, torch.int32), map=full((48, 64, 3), 7, torch.uint8), minfo=full((4,), -3, torch.int32))

    def enqueue(b, stream):
        rc = lib.cotr_tsdf_color_integrate(p(b['color']), 64, 64, 64, origin, to.VOXEL_64, 3 * to.VOXEL_64, p(d_dev), p(i_dev), 2, 48, 64, K2, p(c_dev), None,
                                           W2, 64.0, p(b['info']), stream)
        assert rc == 0, lib.cotr_raster_last_error()
        rc = lib.cotr_tsdf_color_points(p(b['color']), 64, 64, 64, origin, to.VOXEL_64, p(verts), n, None, p(b['rgb']), p(b['valid']), p(b['pinfo']), stream)
        assert rc == 0, lib.cotr_raster_last_error()
        rc = lib.cotr_tsdf_color_map(p(b['color']), 64, 64, 64, origin, to.VOXEL_64, p(model), 48, 64, K1, p(pose_dev), None, p(b['map']), p(b['minfo']), stream)
        assert rc == 0, lib.cotr_raster_last_error()

    def same(a, b):
        for key in a:
            assert torch.equal(a[key], b[key]), key
    first, again = buffers(), buffers()
    here = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    enqueue(first, here)
    enqueue(again, here)
    torch.cuda.synchronize()
    same(first, again)
    assert np.array_equal(first['color'].cpu().numpy(), f['color']) and first['info'][:, 1].tolist() == [16280, 13636]
    assert first['pinfo'][1] > 10000 and first['minfo'][1] > 1500 and first['minfo'][1] <= first['minfo'][2]
    b = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    enqueue(b, ctypes.c_void_p(side.cuda_stream))
    side.synchronize()
    same(first, b)
    # captured once (a single linear chain on the capture stream), replayed once
    b = buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue(b, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    graph.replay()
    torch.cuda.synchronize()
    same(first, b)


# ---- the wrappers on top ----------------------------------------------------------------------------------------------------
def test_fuse_captures_with_colour_a_coloured_raycast_and_a_written_ply(tmp_path):
    f, fc = to.fused(), tc.fused()
    sc = io.scene(48, 64, 48, 64, 3)
    images = tc.images(48, 64)
    cap_a = Capture(images[0], sc['depth_a'], sc['K_a'], sc['c2w_a'])
    cap_b = Capture(torch.from_numpy(images[1].copy()).cuda(), torch.from_numpy(sc['depth_b']).cuda(), sc['K_b'], sc['c2w_b'])
    vol, infos = fuse_captures([cap_a, cap_b], origin=f['origin'], voxel=f['voxel'], dims=f['dims'], color=True, weights=list(tc.FUSED_WEIGHTS))
    same_color(vol, fc, 'fuse_captures')
    fw = to.integrate(*to.fresh(f['dims']), f['origin'], f['voxel'], f['trunc'], *to.captures(48, 64), weights=tc.FUSED_WEIGHTS)   # the same weights
    assert np.array_equal(vol.tsdf.cpu().numpy(), fw['tsdf']) and np.array_equal(vol.weight.cpu().numpy(), fw['weight']) and not fw['near'].any()
    assert infos == [dict(integrated=True, updated=62639, valid=119400, colored=16280), dict(integrated=True, updated=49100, valid=97491, colored=13636)]
    # a volume without colour is fused as before, and its dicts have no new key
    plain, pinfos = fuse_captures([cap_a._replace(image=None), cap_b], origin=f['origin'], voxel=f['voxel'], dims=f['dims'], weights=list(tc.FUSED_WEIGHTS))
    assert plain.color is None and torch.equal(plain.tsdf, vol.tsdf) and pinfos == [{k: v for k, v in d.items() if k != 'colored'} for d in infos]
    with pytest.raises(ValueError, match='image of every capture'):
        fuse_captures([cap_a._replace(image=None)], vol)
    # captures of two sizes: each depth call is followed by its colour call
    small_d, small_i = to.captures(24, 32), tc.images(24, 32)
    mixed = [cap_a, Capture(small_i[1], small_d[0][1], small_d[1][1], small_d[2][1]), cap_b]
    vol3, infos3 = fuse_captures(mixed, origin=f['origin'], voxel=f['voxel'], dims=f['dims'], color=True)
    o = tc.fresh(f['dims'])
    for cap in mixed:
        host = lambda x: x.cpu().numpy() if torch.is_tensor(x) else x   # noqa: E731
        o = tc.integrate(o, f['origin'], f['voxel'], f['trunc'], host(cap.depth)[None], host(cap.image)[None], cap.K[None], cap.c2w[None])['color']
    assert np.array_equal(vol3.color.cpu().numpy(), o) and len(infos3) == 3 and all(d['colored'] > 0 for d in infos3)
    # the raycast with colours: the colour call on its own depth map, in the same sequence
    r = raycast_volume(vol, sc['K_a'], sc['c2w_a'], (48, 64), near=0.5, far=8.0, colors=True)
    again = color_depth_map(vol, r['depth'], sc['K_a'], sc['c2w_a'])
    d = r['depth'].cpu().numpy()
    want = tc.color_map(fc['color'], f['origin'], f['voxel'], d, sc['K_a'], sc['c2w_a'])
    assert sorted(r) == ['depth', 'info', 'rgb'] and torch.equal(r['rgb'], again['rgb']) and not want['near'].any()
    assert np.array_equal(r['rgb'].cpu().numpy(), want['rgb']) and np.array_equal(again['info'].cpu().numpy(), want['info']) and (d > 0).sum() == want['info'][2] > 2000
    assert sorted(raycast_volume(vol, sc['K_a'], sc['c2w_a'], (48, 64), near=0.5, far=8.0)) == ['depth', 'info']
    with pytest.raises(ValueError, match='color=True'):
        raycast_volume(plain, sc['K_a'], sc['c2w_a'], (48, 64), colors=True)
    # the raycast's colour against the texture at the lifted pixels
    p, has = tc.lift(d, sc['K_a'], sc['c2w_a'])
    got = r['rgb'].cpu().numpy()
    valid = got.any(-1)
    e, w = tc.texture_error(got, valid, p), tc.texture_error(want['rgb'], want['rgb'].any(-1), p)
    print(f'the coloured raycast from the pose of A, {int(valid.sum())} of {int(has.sum())} pixels: median {e[0].round(3).tolist()} (restatement '
          f'{w[0].round(3).tolist()}), p90 {e[1].round(3).tolist()} ({w[1].round(3).tolist()})')
    assert valid.sum() == want['info'][1] and (e <= 1.5 * w).all() and (w[0] <= tc.GRADIENT * to.VOXEL_64).all()
    # the mesh with its colours in a file
    verts, tris, normals, info = extract_mesh(vol, normals=True)
    rgb, ok = sample_colors(vol, verts)
    path = tmp_path / 'corner.ply'
    write_ply(path, verts, tris, normals, colors=rgb)
    cols, rows, colors, faces = tc.read_ply(path)
    assert cols == ['x', 'y', 'z', 'nx', 'ny', 'nz'] and np.array_equal(rows[:, :3], verts.cpu().numpy()) and np.array_equal(colors, rgb.cpu().numpy())
    assert np.array_equal(faces, tris.cpu().numpy()) and len(rows) == int(info[1]) and len(faces) == int(info[2]) and ok.float().mean() > 0.99


def test_zoom_engine_fuse_on_a_colour_volume():
    from tests.engine_fixtures import CyclicFakeModel, synthetic_pair
    img_a, img_b = synthetic_pair(1)
    H, W = img_a.shape[:2]
    Hb, Wb = img_b.shape[:2]
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    depth_a = (4.0 + xs / 64.0 + ys / 128.0).astype(np.float32)
    xs, ys = np.meshgrid(np.arange(Wb), np.arange(Hb))
    depth_b = (3.5 + xs / 96.0 + ys / 80.0).astype(np.float32)
    K_a = np.array([[300.0, 0.5, W / 2], [0.0, 310.0, H / 2], [0.0, 0.0, 1.0]])
    K_b = np.array([[280.0, -0.5, Wb / 2], [0.0, 290.0, Hb / 2], [0.0, 0.0, 1.0]])
    cap_a = Capture(img_a, depth_a, K_a, po.pose_matrix((5.0, -3.0, 2.0), (0.3, 0.1, -0.2)))
    cap_b = Capture(img_b, depth_b, K_b, np.eye(4))
    eng = ZoomEngine(CyclicFakeModel().cuda())
    rng = np.random.default_rng(0)
    q = np.stack([rng.uniform(5, W - 5, 40), rng.uniform(5, H - 5, 40)], 1).astype(np.float32)
    kw = dict(queries_a=q, threshold=0.5, max_iters=100, seed=3, icp_max_dist=0.3)
    make = lambda: TsdfVolume((-2.0, -2.0, 3.0), 0.125, (40, 36, 33), color=True)   # noqa: E731
    with torch.no_grad():
        vol, poses, found = eng.fuse([cap_a, cap_b], make(), icp_iters=2, **kw)
    placed = [cap_a] + ([cap_b._replace(c2w=poses[1])] if poses[1] is not None else [])
    want, infos = fuse_captures(placed, make())
    assert found[0] and torch.equal(vol.tsdf, want.tsdf) and torch.equal(vol.color, want.color) and infos[0]['colored'] > 0
    o = tc.integrate(tc.fresh(vol.dims), vol.origin, vol.voxel, vol.trunc, depth_a[None], img_a[None], K_a[None], cap_a.c2w[None])
    assert (vol.color[..., 3] > 0).any() and infos[0]['colored'] == o['info'][0, 1]
