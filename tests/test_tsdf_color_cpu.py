"""The colour volume without a GPU: the numpy restatement (tests/tsdf_color_oracle.py) against scalar loops and against scenes
whose answer is known - a constant image, a sample at a voxel centre, the weight cap, one call against n calls - the shares of
flagged voxels the GPU tests rely on, the argument checks of the three C-ABI calls (they run before any HIP call) and of the
Python wrappers, and ``write_ply`` with colours."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.build import declared_symbols
from cotr_amd.data import Capture
from cotr_amd.inference import TsdfVolume, color_depth_map, fuse_captures, integrate_colors, raycast_volume, sample_colors, write_ply
from tests import tsdf_color_oracle as tc
from tests import tsdf_oracle as to

NAMES = ['cotr_tsdf_color_integrate', 'cotr_tsdf_color_points', 'cotr_tsdf_color_map']
VOLUMES = ((2, 2, 2), (3, 5, 7), (4, 4, 4), (7, 3, 3), (65, 2, 2), (67, 3, 2), (8, 8, 8), (64, 64, 64))
ALL_IN_BAND = ((2, 2, 2), (4, 4, 4), (7, 3, 3))
F32 = 2.0 ** -24   # the relative rounding of a float32


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_integration_against_a_scalar_loop_on_a_tiny_volume():
    dims, voxel, trunc = (4, 3, 5), 0.1, 0.3
    origin = to.small_origin(dims)
    depths, Ks, c2ws = to.captures(24, 32)
    images = tc.images(24, 32)
    r = tc.integrate(tc.fresh(dims), origin, voxel, trunc, depths, images, Ks, c2ws, weights=[1.0, 2.5], max_weight=3.0)
    C = tc.fresh(dims)
    for c in range(2):
        for k in range(dims[2]):
            for j in range(dims[1]):
                for i in range(dims[0]):
                    C[k, j, i] = tc.integrate_voxel(C[k, j, i], i, j, k, origin, voxel, trunc, depths[c], images[c], Ks[c], c2ws[c], (1.0, 2.5)[c], 3.0)
    assert np.array_equal(r['color'], C) and (r['info'][:, 0] == 1).all() and (r['info'][:, 1] > 0).all() and (C[..., 3] == 3.0).any()
    assert not r['near'].any() and np.array_equal(r['band'], C[..., 3] > 0)
    # the third column is the depth call's
    d = to.integrate(*to.fresh(dims), origin, voxel, trunc, depths, Ks, c2ws)
    assert np.array_equal(r['info'][:, 2], d['info'][:, 2]) and (r['info'][:, 1] <= d['info'][:, 1]).all()


def test_samples_against_a_scalar_loop():
    f = tc.fused(24, 32, (8, 8, 8), to.small_origin((8, 8, 8)))
    origin, voxel = np.asarray(to.small_origin((8, 8, 8))), to.VOXEL_64
    rng = np.random.default_rng(5)
    p = origin + voxel * rng.uniform(-0.5, 7.5, (300, 3))
    p[:8] = origin + voxel * np.array([[0, 0, 0], [7, 7, 7], [7, 0, 3.5], [3.5, 7, 0], [0, 2.25, 7], [7.5, 1, 1], [1, -0.25, 1], [np.nan, 1, 1]])
    rgb, valid, near = tc.sample(f['color'], origin, voxel, p)
    assert 0 < valid.sum() < len(p) and rgb.dtype == np.uint8 and not valid[5:8].any()
    for a in range(len(p)):
        one, ok = tc.sample_point(f['color'], origin, voxel, p[a])
        assert ok == valid[a] and tuple(rgb[a]) == one, a
    assert (rgb[~valid] == 0).all()


def _plane_case(z0=2.0, H=24, W=32):
    """a fronto-parallel plane at depth z0 seen from the world's origin, and a 16 x 12 x 20 volume across it whose voxel centres
    sit on multiples of 2^-5: their grid coordinates are exact"""
    K = np.array([[40.0, 0.2, W / 2 - 0.3], [0.0, 41.0, H / 2 + 0.2], [0.0, 0.0, 1.0]])
    depth = np.full((H, W), z0, np.float32)
    dims, voxel, trunc = (16, 12, 20), 0.0625, 0.15
    origin = (-0.375, -0.28125, z0 - 0.59375)
    return depth, K, np.eye(4), dims, voxel, trunc, origin


def test_a_constant_image_colours_the_band_and_nothing_else():
    depth, K, c2w, dims, voxel, trunc, origin = _plane_case()
    image = np.broadcast_to(np.array([200, 17, 91], np.uint8), depth.shape + (3,))
    r = tc.integrate(tc.fresh(dims), origin, voxel, trunc, np.stack([depth] * 3), np.stack([image] * 3), np.stack([K] * 3), np.stack([c2w] * 3),
                     weights=[1.0, 0.3, 2.2])
    d = to.integrate(*to.fresh(dims), origin, voxel, trunc, depth[None], K[None], c2w[None])
    z = origin[2] + voxel * np.arange(dims[2])
    sd = np.broadcast_to((2.0 - z)[:, None, None], dims[::-1])
    seen, col = d['weight'] > 0, r['color'][..., 3] > 0
    assert np.array_equal(col, r['band'])   # (every pixel holds the same depth and colour: a projection at a tie changes nothing)
    # the band and only the band: free space in front of the plane is updated by the depth call and takes no colour
    assert np.array_equal(col, seen & (np.abs(sd) <= trunc)) and 0 < col.sum() < seen.sum() and (seen & (sd > trunc)).any()
    assert (r['color'][~col] == 0).all()
    # an average of equal values is that value exactly, whatever the weights: (c W + c w) / (W + w) rounds to c
    assert (r['color'][col][:, :3] == np.array([200, 17, 91], np.float32)).all() and np.allclose(r['color'][col][:, 3], 3.5)
    # and so is every valid sample, whichever corners of its cell are coloured
    rng = np.random.default_rng(2)
    p = np.asarray(origin) + voxel * rng.uniform(0, np.asarray(dims) - 1, (2000, 3))
    rgb, valid, _ = tc.sample(r['color'], origin, voxel, p)
    assert 100 < valid.sum() < 2000 and (rgb[valid] == [200, 17, 91]).all() and (rgb[~valid] == 0).all()


def test_a_sample_at_a_voxel_centre_is_the_stored_colour_rounded():
    depth, K, c2w, dims, voxel, trunc, origin = _plane_case()
    rng = np.random.default_rng(3)
    image = rng.integers(0, 256, depth.shape + (3,), dtype=np.uint8)
    r = tc.integrate(tc.fresh(dims), origin, voxel, trunc, np.stack([depth, depth]), np.stack([image, image[::-1].copy()]), np.stack([K] * 2),
                     np.stack([c2w] * 2), weights=[1.0, 0.7])
    kk, jj, ii = np.meshgrid(*(np.arange(n) for n in dims[::-1]), indexing='ij')
    p = np.asarray(origin) + voxel * np.stack([ii, jj, kk], -1)
    rgb, valid, near = tc.sample(r['color'], origin, voxel, p)
    col = r['color'][..., 3] > 0
    assert np.array_equal(valid, col) and col.sum() > 500 and not col.all()   # a centre's own corner has beta 1, the other seven 0
    keep = col & ~near
    assert keep.sum() >= 0.99 * col.sum() and np.array_equal(rgb[keep], np.rint(r['color'][keep][:, :3]).astype(np.uint8))
    assert (rgb[~col] == 0).all() and (np.abs(r['color'][col][:, :3] - np.rint(r['color'][col][:, :3])) > 0).any()


def test_the_colour_weight_stops_at_its_cap_and_a_capped_voxel_is_pulled_by_its_share():
    depth, K, c2w, dims, voxel, trunc, origin = _plane_case()
    a, b = np.full(depth.shape + (3,), 60, np.uint8), np.full(depth.shape + (3,), 180, np.uint8)
    st = lambda x, n: np.stack([x] * n)   # noqa: E731
    r = tc.integrate(tc.fresh(dims), origin, voxel, trunc, st(depth, 5), st(a, 5), st(K, 5), st(c2w, 5), weights=[1, 1, 1, 1, 0.5], max_weight=3.0)
    col = r['color'][..., 3] > 0
    assert (r['color'][col][:, 3] == 3.0).all() and (r['color'][col][:, :3] == 60).all()
    pulled = tc.integrate(r['color'], origin, voxel, trunc, depth[None], b[None], K[None], c2w[None], max_weight=3.0)
    assert (pulled['color'][col][:, 3] == 3.0).all() and (pulled['color'][col][:, :3] == 90).all()   # (3 * 60 + 180) / 4
    pulled = tc.integrate(r['color'], origin, voxel, trunc, depth[None], b[None], K[None], c2w[None], weights=[0.5], max_weight=3.0)
    assert np.abs(pulled['color'][col][:, :3] - (3 * 60 + 0.5 * 180) / 3.5).max() <= 256 * F32


def test_n_captures_in_one_call_are_n_calls():
    depths, Ks, c2ws = to.captures(24, 32, 5)
    images = tc.images(24, 32, 5)
    dims = (8, 8, 8)
    origin = to.small_origin(dims)
    found = [1, 0, 1, 1, 0]
    once = tc.integrate(tc.fresh(dims), origin, 0.1, 0.3, depths, images, Ks, c2ws, found=found, weights=[1, 2, 3, 4, 5], max_weight=6.0)
    C = tc.fresh(dims)
    for c in range(5):
        step = tc.integrate(C, origin, 0.1, 0.3, depths[c:c + 1], images[c:c + 1], Ks[c:c + 1], c2ws[c:c + 1], found=found[c:c + 1], weights=[c + 1], max_weight=6.0)
        C = step['color']
        assert list(step['info'][0]) == list(once['info'][c]) and (step['info'][0, 0] == 1) == (found[c] == 1)
    assert np.array_equal(once['color'], C) and (once['info'][[1, 4]] == 0).all() and (C[..., 3] == 6.0).any()


def test_the_two_cameras_agree_on_the_colour_of_the_surface():
    depths, Ks, c2ws = to.captures(48, 64)
    images = tc.images(48, 64)
    assert images.shape == (2, 48, 64, 3) and images.dtype == np.uint8 and (images[depths > 0] > 0).all() and (images[depths == 0] == 0).all()
    f = tc.fused()
    # A coloured voxel lies within trunc of the surface point its pixel saw, and a sample blends the voxels of one cell.  The
    # texture changes by at most GRADIENT (amplitude times the length of the wave vector) per unit length, so an error beyond
    # GRADIENT * (trunc + a cell's diagonal) + a rounding to a byte on either side would mean the cameras disagree; half of the
    # points sit within a voxel.
    p, has = tc.lift(depths[0], Ks[0], c2ws[0])
    rgb, valid, _ = tc.sample(f['color'], to.ORIGIN_64, to.VOXEL_64, p)
    e = tc.texture_error(rgb, valid, p)
    worst = np.abs(rgb[valid].astype(np.float64) - tc.texture(p[valid])).max(0)
    print(f'the fused colour at the lifted pixels of A against the texture: median {e[0].round(2).tolist()}, p90 {e[1].round(2).tolist()}, '
          f'max {worst.round(2).tolist()} of {int(valid.sum())} pixels')
    assert valid.sum() > 2000 and (worst <= tc.GRADIENT * (0.3 + np.sqrt(3) * to.VOXEL_64) + 1.0).all() and (e[0] <= tc.GRADIENT * to.VOXEL_64).all()


@pytest.mark.parametrize('shape', [(24, 32), (48, 64)], ids=['24x32', '48x64'])
def test_the_cases_of_the_gpu_tests_flag_nothing_and_have_voxels_outside_the_band(shape):
    depths, Ks, c2ws = to.captures(*shape)
    images = tc.images(*shape)
    for dims in VOLUMES:
        origin = to.ORIGIN_64 if dims == (64, 64, 64) else to.small_origin(dims)
        r = tc.integrate(tc.fresh(dims), origin, to.VOXEL_64, 3 * to.VOXEL_64, depths, images, Ks, c2ws)
        coloured, valid = r['info'][:, 1], r['info'][:, 2]
        print(f'{dims} with maps {shape}: {coloured.tolist()} of {valid.tolist()} valid voxels coloured, {int(r["near"].sum())} flagged')
        assert not r['near'].any() and (coloured > 0).all()
        assert (coloured == valid).all() if dims in ALL_IN_BAND else (coloured < valid).all(), dims
        if dims == (64, 64, 64) and shape == (48, 64):
            assert r['info'].tolist() == [[1, 16280, 119400, 0], [1, 13636, 97491, 0]]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound_and_take_no_scratch():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cotr_hip.h')).read()
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and name in declared_symbols()
        assert getattr(_lib.load_library(), name) is not None
        args = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', header, flags=re.S).group(1)
        assert 'scratch' not in args and args.rstrip().endswith('cotr_stream stream')
    assert _lib.load_library().cotr_abi_version() == 2


K9 = (ctypes.c_double * 9)(100.0, 0.5, 64.0, 0.0, 100.0, 48.0, 0.0, 0.0, 1.0)
P = ctypes.c_void_p(4096)              # never dereferenced: every call below fails its checks before any HIP call
ODD16, ODD8, ODD4 = ctypes.c_void_p(4104), ctypes.c_void_p(4100), ctypes.c_void_p(4098)
NAN, INF = float('nan'), float('inf')
VOLUME_CASES = ((dict(Nx=1), b'2^28'), (dict(Ny=1), b'2^28'), (dict(Nz=1), b'2^28'), (dict(Nx=1 << 10, Ny=1 << 10, Nz=(1 << 8) + 1), b'2^28'),
                (dict(Nx=1 << 16, Ny=1 << 16, Nz=1 << 16), b'2^28'), (dict(voxel=0.0), b'voxel'), (dict(voxel=-1.0), b'voxel'),
                (dict(voxel=INF), b'voxel'), (dict(voxel=NAN), b'voxel'), (dict(color=None), b'NULL'), (dict(origin=None), b'NULL'),
                (dict(origin=(ctypes.c_double * 3)(0.0, NAN, 0.0)), b'origin'), (dict(origin=(ctypes.c_double * 3)(INF, 0.0, 0.0)), b'origin'),
                (dict(color=ODD16), b'16-byte'), (dict(color=ODD8), b'16-byte'), (dict(color=ODD4), b'16-byte'))
O3 = (ctypes.c_double * 3)(0.0, 0.0, 0.0)


def _bad_k(i, v, n=1):
    k = (ctypes.c_double * (9 * n))(*(list(K9) * n))
    k[i] = v
    return k


def _check(call, cases, name):
    lib = _lib.load_library()
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())
        assert name in lib.cotr_raster_last_error()


def test_color_integrate_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    K2 = (ctypes.c_double * 18)(*(list(K9) * 2))

    def call(color=P, Nx=8, Ny=8, Nz=8, origin=O3, voxel=0.1, trunc=0.3, depths=P, images=P, n=2, H=96, W=128, Ks=K2, c2w=P, found=None, obs=None,
             max_weight=64.0, info=P):
        return lib.cotr_tsdf_color_integrate(color, Nx, Ny, Nz, origin, voxel, trunc, depths, images, n, H, W, Ks, c2w, found, obs, max_weight, info, None)
    w2 = lambda a, b: (ctypes.c_double * 2)(a, b)   # noqa: E731
    _check(call, VOLUME_CASES + (
        (dict(trunc=0.0), b'trunc'), (dict(trunc=-0.1), b'trunc'), (dict(trunc=INF), b'trunc'), (dict(trunc=NAN), b'trunc'),
        (dict(n=0), b'[1, 32]'), (dict(n=33), b'[1, 32]'), (dict(H=0), b'pixels'), (dict(W=0), b'pixels'),
        (dict(H=1 << 14, W=(1 << 14) + 1), b'pixels'), (dict(max_weight=0.0), b'max_weight'), (dict(max_weight=-1.0), b'max_weight'),
        (dict(max_weight=NAN), b'max_weight'), (dict(depths=None), b'NULL'), (dict(images=None), b'NULL'), (dict(Ks=None), b'NULL'),
        (dict(c2w=None), b'NULL'), (dict(info=None), b'NULL'), (dict(Ks=_bad_k(0, 0.0, 2)), b'focal'), (dict(Ks=_bad_k(9 + 4, 0.0, 2)), b'focal'),
        (dict(Ks=_bad_k(9 + 2, NAN, 2)), b'focal'), (dict(Ks=_bad_k(1, INF, 2)), b'focal'), (dict(obs=w2(1.0, 0.0)), b'obs_weight'),
        (dict(obs=w2(-1.0, 1.0)), b'obs_weight'), (dict(obs=w2(1.0, INF)), b'obs_weight'), (dict(obs=w2(NAN, 1.0)), b'obs_weight'),
        (dict(depths=ODD4), b'aligned'), (dict(c2w=ODD8), b'aligned'), (dict(found=ODD4), b'aligned'), (dict(info=ODD4), b'aligned')),
        b'cotr_tsdf_color_integrate')


def test_color_points_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()

    def call(color=P, Nx=8, Ny=8, Nz=8, origin=O3, voxel=0.1, points=P, n=5, found=None, rgb=P, valid=P, info=P):
        return lib.cotr_tsdf_color_points(color, Nx, Ny, Nz, origin, voxel, points, n, found, rgb, valid, info, None)
    _check(call, VOLUME_CASES + (
        (dict(n=-1), b'[0, 2^28]'), (dict(n=(1 << 28) + 1), b'[0, 2^28]'), (dict(points=None), b'NULL'), (dict(rgb=None), b'NULL'),
        (dict(valid=None), b'NULL'), (dict(info=None), b'NULL'), (dict(n=0, info=None), b'NULL'), (dict(points=ODD8), b'aligned'),
        (dict(found=ODD4), b'aligned'), (dict(info=ODD4), b'aligned')), b'cotr_tsdf_color_points')


def test_color_map_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()

    def call(color=P, Nx=8, Ny=8, Nz=8, origin=O3, voxel=0.1, depth=P, H=96, W=128, K=K9, c2w=P, found=None, rgb=P, info=P):
        return lib.cotr_tsdf_color_map(color, Nx, Ny, Nz, origin, voxel, depth, H, W, K, c2w, found, rgb, info, None)
    _check(call, VOLUME_CASES + (
        (dict(H=0), b'pixels'), (dict(W=0), b'pixels'), (dict(H=(1 << 14) + 1, W=1 << 14), b'pixels'), (dict(depth=None), b'NULL'),
        (dict(K=None), b'NULL'), (dict(c2w=None), b'NULL'), (dict(rgb=None), b'NULL'), (dict(info=None), b'NULL'),
        (dict(K=_bad_k(0, 0.0)), b'focal'), (dict(K=_bad_k(4, 0.0)), b'focal'), (dict(K=_bad_k(5, NAN)), b'focal'),
        (dict(depth=ODD4), b'aligned'), (dict(c2w=ODD8), b'aligned'), (dict(found=ODD4), b'aligned'), (dict(info=ODD4), b'aligned')),
        b'cotr_tsdf_color_map')


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
K = np.array([[100.0, 0.5, 6.0], [0.0, 100.0, 5.0], [0.0, 0.0, 1.0]])
D = np.ones((2, 10, 12), np.float32)
I = np.ones((2, 10, 12, 3), np.uint8)
C = np.stack([np.eye(4)] * 2)


def _volume(color=True):
    """a volume's scalars without its tensors: every check below fails before a tensor is read"""
    v = TsdfVolume.__new__(TsdfVolume)
    v.origin, v.voxel, v.dims, v.trunc, v.max_weight = np.zeros(3), 0.1, (8, 8, 8), 0.3, 64.0
    v.device, v.tsdf, v.weight, v.color = torch.device('cpu'), None, None, ('a colour tensor' if color else None)
    return v


def test_wrapper_argument_errors_without_a_gpu():
    v, plain = _volume(), _volume(color=False)
    for kw, word in ((dict(volume=None), 'TsdfVolume'), (dict(volume=plain), 'color=True'), (dict(depths=D[0]), r'\[n, H, W\]'),
                     (dict(depths=D.astype(np.float64)), 'float32'), (dict(images=I.astype(np.float32)), 'uint8'), (dict(images=I[0]), 'three channels'),
                     (dict(images=I[:, :, :, :2]), 'three channels'), (dict(images=I[:, :9]), 'three channels'), (dict(images=torch.ones(I.shape)), 'uint8'),
                     (dict(Ks=np.eye(4)), r'\[3, 3\]'), (dict(Ks=np.stack([K] * 3)), r'\[3, 3\]'), (dict(Ks=np.diag([0.0, 1.0, 1.0])), 'focal'),
                     (dict(c2ws=C[:1]), 'c2ws'), (dict(c2ws=np.stack([np.eye(3)] * 2)), r'\[4, 4\]'), (dict(c2ws=C * NAN), r'\[4, 4\]'),
                     (dict(weights=[1.0]), 'weights'), (dict(weights=[1.0, 0.0]), 'weights'), (dict(weights=[INF, 1.0]), 'weights'),
                     (dict(found=[1, 1, 1]), 'found')):
        args = dict(volume=v, depths=D, images=I, Ks=K, c2ws=C)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            integrate_colors(**args)
    for kw, word in ((dict(volume=None), 'TsdfVolume'), (dict(volume=plain), 'color=True'), (dict(points=np.zeros((4, 2))), r'\[N, 3\]'),
                     (dict(points=np.zeros(3)), r'\[N, 3\]')):
        args = dict(volume=v, points=np.zeros((4, 3)))
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            sample_colors(**args)
    for kw, word in ((dict(volume=None), 'TsdfVolume'), (dict(volume=plain), 'color=True'), (dict(depth=D), r'\[H, W\]'),
                     (dict(depth=D[0].astype(np.float64)), 'float32'), (dict(K=np.eye(2)), r'\[3, 3\]'), (dict(K=np.diag([1.0, 0.0, 1.0])), 'focal'),
                     (dict(c2w=np.eye(3)), r'\[4, 4\]'), (dict(c2w=None), r'\[4, 4\]'), (dict(c2w=np.full((4, 4), INF)), r'\[4, 4\]')):
        args = dict(volume=v, depth=D[0], K=K, c2w=np.eye(4))
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            color_depth_map(**args)
    with pytest.raises(ValueError, match='color=True'):
        raycast_volume(plain, K, np.eye(4), (10, 12), colors=True)
    with pytest.raises(ValueError, match='step'):      # the raycast's own rules come first
        raycast_volume(plain, K, np.eye(4), (10, 12), step=0.0, colors=True)
    cap = Capture(I[0], D[0], K, np.eye(4))
    fresh = dict(volume=None, origin=(0, 0, 0), voxel=0.1, dims=(8, 8, 8), color=True)
    for kw, word in ((dict(caps=[cap, cap._replace(image=None)]), 'image of every capture'), (dict(caps=[cap._replace(image=I[0].astype(np.float32))]), 'uint8'),
                     (dict(caps=[cap._replace(image=I[0, :9])]), 'three channels'), (dict(caps=[cap._replace(image=I[0, :, :, 0])]), 'three channels'),
                     (dict(caps=[cap._replace(image=None)], **fresh), 'image of every capture'), (dict(caps=[cap._replace(image=I[0, 1:])], **fresh), 'three channels'),
                     (dict(caps=[cap._replace(depth=D[0].astype(np.float64))]), 'float32'), (dict(caps=[cap], weights=[1.0, 2.0]), 'weights')):
        args = dict(caps=[cap], volume=v)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            fuse_captures(**args)


def test_cpu_tensors_are_refused():
    v = _volume()
    for kw in (dict(depths=torch.ones((2, 10, 12))), dict(images=torch.ones(I.shape, dtype=torch.uint8)),
               dict(c2ws=torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)), dict(found=torch.ones(2, dtype=torch.int32))):
        args = dict(volume=v, depths=D, images=I, Ks=K, c2ws=C)
        args.update(kw)
        with pytest.raises(_lib.CotrHipError, match='MI355X only'):
            integrate_colors(**args)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        sample_colors(v, torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        color_depth_map(v, torch.ones((10, 12)), K, np.eye(4))
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        color_depth_map(v, D[0], K, torch.eye(4, dtype=torch.float64))
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        fuse_captures([Capture(torch.ones((10, 12, 3), dtype=torch.uint8), D[0], K, np.eye(4))], v)


# ---- the PLY file ---------------------------------------------------------------------------------------------------------
def _mesh():
    rng = np.random.default_rng(9)
    verts, normals = rng.normal(size=(7, 3)), rng.normal(size=(7, 3))
    tris = np.array([[0, 1, 2], [2, 3, 4], [-1, -1, -1], [4, 5, 6]], np.int32)
    return verts, tris, normals, rng.integers(0, 256, (7, 3), dtype=np.uint8)


@pytest.mark.parametrize('with_normals', [False, True], ids=['plain', 'normals'])
def test_write_ply_with_colours_is_parsed_back(tmp_path, with_normals):
    verts, tris, normals, colors = _mesh()
    path = tmp_path / 'mesh.ply'
    write_ply(path, torch.from_numpy(verts), tris, normals if with_normals else None, colors=torch.from_numpy(colors))
    raw = path.read_bytes()
    head, body = raw[:raw.index(b'end_header\n') + 11].decode('ascii'), raw[raw.index(b'end_header\n') + 11:]
    lines = head.split('\n')
    names = [ln.split()[2] for ln in lines if ln.startswith('property') and 'list' not in ln]
    want = list('xyz') + (['nx', 'ny', 'nz'] if with_normals else []) + ['red', 'green', 'blue']
    assert lines[:3] == ['ply', 'format binary_little_endian 1.0', 'element vertex 7'] and names == want and 'element face 3' in lines
    assert [ln.split()[1] for ln in lines if ln.startswith('property') and 'list' not in ln] == ['double'] * (len(want) - 3) + ['uchar'] * 3
    nd = len(want) - 3
    vt = np.dtype([('d', '<f8', (nd,)), ('c', 'u1', (3,))])
    ft = np.dtype([('n', 'u1'), ('v', '<i4', (3,))])
    assert len(body) == 7 * vt.itemsize + 3 * ft.itemsize and vt.itemsize == 8 * nd + 3
    v = np.frombuffer(body[:7 * vt.itemsize], vt)
    f = np.frombuffer(body[7 * vt.itemsize:], ft)
    assert np.array_equal(v['d'][:, :3], verts) and np.array_equal(v['c'], colors) and (not with_normals or np.array_equal(v['d'][:, 3:], normals))
    assert (f['n'] == 3).all() and np.array_equal(f['v'], tris[[0, 1, 3]])
    for bad, word in ((colors[:6], 'colors'), (colors.astype(np.float64), 'colors'), (colors[:, :2], 'colors')):
        with pytest.raises(ValueError, match=word):
            write_ply(path, verts, tris, colors=bad)


@pytest.mark.parametrize('with_normals', [False, True], ids=['plain', 'normals'])
def test_write_ply_without_colours_is_the_file_it_was(tmp_path, with_normals):
    verts, tris, normals, _ = _mesh()
    path = tmp_path / 'mesh.ply'
    write_ply(path, verts, tris, normals if with_normals else None)
    # the bytes as the function wrote them before it knew colours: the header, the doubles of every vertex, the faces
    t = tris[[0, 1, 3]]
    header = ['ply', 'format binary_little_endian 1.0', 'element vertex 7'] + [f'property double {c}' for c in 'xyz']
    header += [f'property double n{c}' for c in 'xyz'] if with_normals else []
    header += ['element face 3', 'property list uchar int vertex_indices', 'end_header']
    faces = np.empty(3, dtype=[('n', 'u1'), ('v', '<i4', (3,))])
    faces['n'], faces['v'] = 3, t
    cols = [verts.astype('<f8')] + ([normals.astype('<f8')] if with_normals else [])
    want = ('\n'.join(header) + '\n').encode('ascii') + np.ascontiguousarray(np.hstack(cols)).tobytes() + faces.tobytes()
    assert path.read_bytes() == want
