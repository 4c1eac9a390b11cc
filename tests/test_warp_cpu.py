"""The warps without a GPU: the numpy restatement (tests/warp_oracle.py) against hand-computed cases and against the exact
bilinear value within a derived bound, get_perspective_transform, the argument checks of the Python layer and of the C
entry points (they run before any HIP call), and the declarations of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.build import declared_symbols
from cotr_amd.inference import get_perspective_transform, paste_by_corners, warp_by_corr, warp_by_map, warp_perspective
from cotr_amd.inference import warp as warp_mod
from tests import warp_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def const_map(Hd, Wd, x, y, dtype=np.float32):
    m = np.empty((Hd, Wd, 2), dtype)
    m[..., 0], m[..., 1] = x, y
    return m


# ---- the restatement against hand-computed cases ------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_identity_map_returns_the_image(C, dtype):
    img = wo.image(19, 23, C, 0)
    dst, cover = wo.remap(img, wo.identity_map(19, 23, dtype))
    assert dst.dtype == np.uint8 and np.array_equal(dst, img) and cover.all()
    g, cover = wo.remap(img[..., 0], wo.identity_map(19, 23, dtype))
    assert g.shape == (19, 23) and np.array_equal(g, img[..., 0])


def test_integer_shift_is_exact_with_zeros_shifted_in():
    img = wo.image(11, 17, 3, 1)
    m = wo.identity_map(11, 17) + np.float32([3, -2])              # dst[i, j] = src[i - 2, j + 3]
    dst, cover = wo.remap(img, m)
    want = np.zeros_like(img)
    want[2:, :14] = img[:9, 3:]
    assert np.array_equal(dst, want)
    want_cover = np.zeros((11, 17), bool)
    want_cover[2:, :14] = True
    assert np.array_equal(cover, want_cover)


def test_ties_at_k_over_64_go_to_even():
    # v * 32 = k / 2: rint takes the even neighbour
    assert list(wo.fix(np.float32([0.5 / 32, 1.5 / 32, 2.5 / 32, 3.5 / 32, -0.5 / 32, -1.5 / 32, 5 + 1 / 64, 5 + 3 / 64]))) == \
        [0, 2, 2, 4, 0, -2, 160, 162]
    src = np.array([[0, 64]], np.uint8)
    # x = 1/64 rounds to fx = 0 -> 0; x = 3/64 rounds to fx = 2 -> (2 * 32 * 64 + 512) >> 10 = 4
    dst, _ = wo.remap(src, np.float32([[[1 / 64, 0], [3 / 64, 0]]]))
    assert list(dst[0]) == [0, 4]


def test_negative_coordinates_floor():
    X = wo.fix(np.float32([-0.5]))
    assert X[0] == -16 and X[0] >> 5 == -1 and X[0] & 31 == 16
    src = np.array([[200, 100], [50, 10]], np.uint8)
    # x = -0.5, y = 0: taps (-1, 0) outside and (0, 0) = 200, weights 16 * 32 each -> (512 * 200 + 512) >> 10 = 100
    dst, cover = wo.remap(src, np.float32([[[-0.5, 0.0]]]))
    assert dst[0, 0] == 100 and cover[0, 0]
    # x = y = -0.5: only (0, 0) inside, weight 256 -> (256 * 200 + 512) >> 10 = 50
    dst, cover = wo.remap(src, np.float32([[[-0.5, -0.5]]]))
    assert dst[0, 0] == 50 and cover[0, 0]
    # x = -1: taps -1 (weight 1024, outside) and 0 (weight 0): uncovered although tap 0 is inside
    dst, cover = wo.remap(src, np.float32([[[-1.0, 0.0]]]))
    assert dst[0, 0] == 0 and not cover[0, 0]
    # x = 1 (the last column): tap 1 carries all the weight, tap 2 is outside with weight 0: covered, exact
    dst, cover = wo.remap(src, np.float32([[[1.0, 1.0]]]))
    assert dst[0, 0] == 10 and cover[0, 0]


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 26, -2.0 ** 26])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_unusable_coordinates_give_the_border_value(bad, dtype):
    img = np.full((5, 7, 3), 255, np.uint8)
    bg = wo.image(2, 2, 3, 2)
    for m in (const_map(2, 2, bad, 1.0, dtype), const_map(2, 2, 2.0, bad, dtype), const_map(2, 2, bad, bad, dtype)):
        dst, cover = wo.remap(img, m)
        assert (dst == 0).all() and not cover.any()
        dst, cover = wo.remap(img, m, background=bg)
        assert np.array_equal(dst, bg) and not cover.any()
    # the largest usable magnitude is simply far outside
    dst, cover = wo.remap(img, const_map(1, 1, np.float32(2.0 ** 26 - 4), 0.0))
    assert dst[0, 0, 0] == 0 and not cover[0, 0]


def test_float64_map_is_rounded_to_float32_first():
    src = np.array([[0, 64]], np.uint8)
    x = 3 / 64 - 1e-12                          # float64: just below the tie, rint -> fx = 1; as float32 it IS the tie -> fx = 2
    assert wo.fix(np.float64([x]))[0] == 2
    dst, _ = wo.remap(src, np.float64([[[x, 0.0]]]))
    assert dst[0, 0] == 4
    assert wo.fix(np.float64([1e300]))[0] == wo.OUTSIDE          # overflows to inf


def test_one_by_one_source():
    src = np.array([[[40, 80, 120]]], np.uint8)
    m = np.float32([[[0, 0], [0.5, 0], [0, 0.25], [-0.75, -0.5], [1, 0], [0.96875, 0.96875], [-1, -1]]])
    dst, cover = wo.remap(src, m)
    # weights of tap (0, 0): 1024, 512, 768, 8 * 16 = 128, 0, 1 * 1 = 1, 0
    for k, w in enumerate([1024, 512, 768, 128, 0, 1, 0]):
        assert list(dst[0, k]) == [(w * v + 512) >> 10 for v in (40, 80, 120)], k
        assert cover[0, k] == (w != 0), k


def test_background_fills_exactly_the_uncovered_pixels():
    img, bg = wo.image(9, 9, 3, 3), wo.image(12, 14, 3, 4)
    m = wo.smooth_map(12, 14, 9, 9, 5, margin=0.4)
    plain, cover = wo.remap(img, m)
    pasted, cover2 = wo.remap(img, m, background=bg)
    assert np.array_equal(cover, cover2) and cover.any() and not cover.all()
    assert np.array_equal(pasted[cover], plain[cover]) and np.array_equal(pasted[~cover], bg[~cover])
    assert (plain[~cover] == 0).all()


# ---- the independent bound ------------------------------------------------------------------------------------------------
def bound_holds(img, m):
    dst, _ = wo.remap(img, m)
    value, Gx, Gy = wo.exact(img, m)
    d3 = dst if dst.ndim == 3 else dst[..., None]
    err = np.abs(d3.astype(np.float64) - value)
    slack = 0.5 + (Gx + Gy) / 64 - err
    assert (slack >= -1e-9).all(), (err.max(), float(slack.min()))       # (1e-9: the float64 evaluation of `exact` itself)
    return err.max()


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_restatement_is_within_the_derived_bound_of_exact_bilinear(C, dtype):
    rng = np.random.default_rng(C)
    img = wo.image(37, 53, C, C)
    noise = rng.integers(0, 256, (37, 53, C)).astype(np.uint8)          # every pair of neighbours far apart
    worst = 0.0
    for src in (img, noise, img[..., 0] if C == 1 else img):
        for m in (wo.smooth_map(64, 80, 37, 53, 1, dtype), wo.smooth_map(64, 80, 37, 53, 2, dtype, margin=0.3),
                  rng.uniform(-3, 56, (40, 40, 2)).astype(dtype),
                  (rng.integers(-2 * 64, 55 * 64, (40, 40, 2)) / 64).astype(dtype),      # every value on a k/64 tie or grid point
                  wo.identity_map(37, 53, dtype) + dtype(0.5)):
            worst = max(worst, bound_holds(src, m))
    assert worst > 0.4                                                   # the cases do exercise the rounding


def test_bound_with_unusable_values_and_tiny_sources():
    rng = np.random.default_rng(7)
    m = rng.uniform(-2, 4, (30, 30, 2)).astype(np.float32)
    m[rng.random((30, 30)) < 0.2] = np.nan
    m[rng.random((30, 30)) < 0.1, 0] = np.inf
    m[rng.random((30, 30)) < 0.1, 1] = -1e30
    for shape in ((1, 1, 3), (1, 5, 1), (4, 1, 4), (2, 2, 3)):
        bound_holds(rng.integers(0, 256, shape).astype(np.uint8), m)


# ---- get_perspective_transform ----------------------------------------------------------------------------------------------
def project(M, pts):
    q = np.hstack([pts, np.ones((len(pts), 1))]) @ M.T
    return q[:, :2] / q[:, 2:]


@pytest.mark.parametrize('seed', range(5))
def test_get_perspective_transform_maps_the_points(seed):
    rng = np.random.default_rng(seed)
    src = np.array([[0, 0], [1000, 0], [0, 1200], [1000, 1200]], np.float64) + rng.uniform(-50, 50, (4, 2))
    dst = np.array([[932, 1025], [2469, 901], [908, 2927], [2436, 3080]], np.float64) + rng.uniform(-200, 200, (4, 2))
    M = get_perspective_transform(src, dst)
    assert M.dtype == np.float64 and M.shape == (3, 3) and M[2, 2] == 1.0
    assert np.abs(project(M, src) - dst).max() <= 1e-9
    M32 = get_perspective_transform(src.astype(np.float32), dst.astype(np.float32))      # cv2 takes float32 points
    assert np.abs(project(M32, src.astype(np.float32).astype(np.float64)) - dst.astype(np.float32)).max() <= 1e-9


def test_get_perspective_transform_identity_and_errors():
    pts = np.array([[3, 4], [100, 7], [5, 90], [120, 130]], np.float32)
    assert np.abs(get_perspective_transform(pts, pts) - np.eye(3)).max() <= 1e-12
    with pytest.raises(ValueError, match=r'\[4, 2\]'):
        get_perspective_transform(pts[:3], pts[:3])
    with pytest.raises(ValueError, match='singular'):
        get_perspective_transform(np.array([[0, 0], [1, 1], [2, 2], [3, 3]], np.float32), pts)
    with pytest.raises(ValueError, match='finite'):
        get_perspective_transform(pts * np.nan, pts)


def test_paste_corner_order_is_the_demos():
    # demo_homography.py:41: rep_coord = [[0, 0], [W, 0], [0, H], [W, H]] of rep_img.shape = (H, W, 3), float32
    shape = (1200, 1000, 3)
    rep_coord = np.array([[0, 0], [shape[1], 0], [0, shape[0]], [shape[1], shape[0]]]).astype(np.float32)
    got = warp_mod.picture_corners(shape)
    assert got.dtype == np.float32 and np.array_equal(got, rep_coord)


# ---- the perspective restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 3, 4])
def test_perspective_identity_returns_the_image(C):
    img = wo.image(21, 33, C, 5)
    dst, cover = wo.warp_perspective(img, np.eye(3), 21, 33)
    assert np.array_equal(dst, img) and cover.all()
    dst, cover = wo.warp_perspective(img, np.eye(3) * 0.125, 21, 33)      # homogeneous scale: the same positions
    assert np.array_equal(dst, img) and cover.all()


def test_perspective_integer_translation_equals_the_shifted_image():
    img = wo.image(21, 33, 3, 6)
    Minv = np.array([[1, 0, -4], [0, 1, 3], [0, 0, 1]], np.float64)       # dst[i, j] = src[i + 3, j - 4]
    dst, cover = wo.warp_perspective(img, Minv, 21, 33)
    want = np.zeros_like(img)
    want[:18, 4:] = img[3:, :29]
    assert np.array_equal(dst, want)
    assert cover[:18, 4:].all() and cover.sum() == 18 * 29
    X, Y = wo.perspective_coords(Minv, 21, 33)
    assert np.array_equal(X, (np.arange(33)[None, :] - 4) * 32 + np.zeros((21, 1), np.int64))
    assert np.array_equal(Y, (np.arange(21)[:, None] + 3) * 32 + np.zeros((1, 33), np.int64))


def test_perspective_pixel_on_the_horizon_is_uncovered():
    img = np.full((8, 8, 3), 200, np.uint8)
    Minv = np.array([[1, 0, 0], [0, 1, 0], [0.25, 0, 0]], np.float64)     # W = x / 4 = 0 in column 0; elsewhere (4, 4 y / x)
    dst, cover = wo.warp_perspective(img, Minv, 8, 8)
    X, Y = wo.perspective_coords(Minv, 8, 8)
    assert (X[:, 0] == wo.OUTSIDE).all() and (Y[:, 0] == wo.OUTSIDE).all()
    assert not cover[:, 0].any() and (dst[:, 0] == 0).all()
    assert (X[:, 1:] == 4 * 32).all() and cover[:2, 1:].all() and (dst[:2, 1:] == 200).all()
    # huge but finite positions next to the horizon are clamped and lie outside; NaN positions are uncovered too
    Minv = np.array([[1e300, 0, 1e300], [0, 1, 0], [1e-300, 0, -4e-300]], np.float64)
    dst, cover = wo.warp_perspective(img, Minv, 8, 8)
    assert not cover.any()


# ---- the Python layer's argument checks ---------------------------------------------------------------------------------------
def test_wrapper_argument_errors_without_a_gpu():
    img, m = np.zeros((4, 5, 3), np.uint8), np.zeros((6, 7, 2), np.float32)
    with pytest.raises(ValueError, match='uint8'):
        warp_by_map(img.astype(np.float32), m)
    with pytest.raises(ValueError, match='1, 3 or 4 channels'):
        warp_by_map(np.zeros((4, 5, 2), np.uint8), m)
    with pytest.raises(ValueError, match=r'\[H, W\] or \[H, W, C\]'):
        warp_by_map(np.zeros((4, 5, 3, 1), np.uint8), m)
    with pytest.raises(ValueError, match=r'\[H, W, 2\]'):
        warp_by_map(img, np.zeros((6, 7, 3), np.float32))
    with pytest.raises(ValueError, match='float32 or float64'):
        warp_by_map(img, np.zeros((6, 7, 2), np.float16))
    with pytest.raises(ValueError, match='background'):
        warp_by_map(img, m, background=np.zeros((6, 8, 3), np.uint8))
    with pytest.raises(ValueError, match='background'):
        warp_by_map(img, m, background=np.zeros((6, 7), np.uint8))
    with pytest.raises(ValueError, match='uint8'):
        warp_by_map(img, m, background=np.zeros((6, 7, 3), np.int32))
    with pytest.raises(ValueError, match='16384'):
        warp_by_map(img, np.zeros((1, 16385, 2), np.float32))
    with pytest.raises(ValueError, match='16384'):
        warp_by_map(np.zeros((0, 5, 3), np.uint8), m)
    with pytest.raises(ValueError, match='singular'):
        warp_perspective(img, np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]]), (7, 6))
    with pytest.raises(ValueError, match='singular'):
        warp_perspective(img, np.zeros((3, 3)), (7, 6))
    with pytest.raises(ValueError, match='3 x 3'):
        warp_perspective(img, np.eye(2), (7, 6))
    with pytest.raises(ValueError, match='finite'):
        warp_perspective(img, np.eye(3) * np.nan, (7, 6), inverse_map=True)
    with pytest.raises(ValueError, match='dsize'):
        warp_perspective(img, np.eye(3), (7, 6, 3))
    with pytest.raises(ValueError, match='dsize'):
        warp_perspective(img, np.eye(3), (0, 6))
    with pytest.raises(ValueError, match=r'\[4, 2\]'):
        paste_by_corners(img, np.zeros((3, 2)), img)
    with pytest.raises(ValueError, match='uint8'):
        warp_by_corr(img.astype(np.float64), img, np.zeros((5, 4)))
    # a CPU tensor is not a device tensor: no fallback
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        warp_by_map(torch.from_numpy(img), m)
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        warp_by_map(img, torch.from_numpy(m))
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        warp_perspective(torch.from_numpy(img), np.eye(3), (7, 6))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    names = declared_symbols()
    assert 'cotr_warp_map' in names and 'cotr_warp_perspective' in names
    header = open(os.path.join(ROOT, 'include', 'cotr_hip.h')).read()
    assert re.search(r'#define\s+COTR_HIP_ABI_VERSION\s+2\b', header)
    lib = _lib.load_library()
    assert lib.cotr_abi_version() == 2
    assert 'cotr_warp_map' in _lib.EXPORTED_SYMBOLS and 'cotr_warp_perspective' in _lib.EXPORTED_SYMBOLS
    assert callable(lib.cotr_warp_map) and callable(lib.cotr_warp_perspective)


def test_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    P, Q, R = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 31)   # never dereferenced
    M = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)

    def wmap(src=P, Hs=8, Ws=8, C=3, map_=Q, f64=0, Hd=8, Wd=8, dst=R, cover=None, bg=None):
        return lib.cotr_warp_map(src, Hs, Ws, C, map_, f64, Hd, Wd, dst, cover, bg, None)

    def wpersp(src=P, Hs=8, Ws=8, C=3, M_=M, Hd=8, Wd=8, dst=R, cover=None, bg=None):
        return lib.cotr_warp_perspective(src, Hs, Ws, C, M_, Hd, Wd, dst, cover, bg, None)
    cases = [(dict(src=None), b'NULL'), (dict(dst=None), b'NULL'), (dict(C=2), b'1, 3 or 4'), (dict(C=5), b'1, 3 or 4'),
             (dict(C=0), b'1, 3 or 4'), (dict(Hs=0), b'[1, 16384]'), (dict(Ws=0), b'[1, 16384]'), (dict(Hd=0), b'[1, 16384]'),
             (dict(Wd=0), b'[1, 16384]'), (dict(Hs=16385), b'[1, 16384]'), (dict(Ws=16385), b'[1, 16384]'),
             (dict(Hd=16385), b'[1, 16384]'), (dict(Wd=16385), b'[1, 16384]'), (dict(Hd=-1), b'[1, 16384]'),
             (dict(dst=P), b'alias src'), (dict(dst=ctypes.c_void_p((1 << 20) + 100)), b'alias src'),
             (dict(bg=R), b'alias background'), (dict(bg=ctypes.c_void_p((1 << 31) + 8 * 8 * 3 - 1)), b'alias background')]
    for call in (wmap, wpersp):
        for kw, word in cases:
            assert call(**kw) == -1, (call.__name__, kw)
            assert word in lib.cotr_raster_last_error(), (call.__name__, kw, lib.cotr_raster_last_error())
    assert wmap(map_=None) == -1 and b'map must not be NULL' in lib.cotr_raster_last_error()
    assert wmap(map_=ctypes.c_void_p((1 << 30) + 4)) == -1 and b'aligned' in lib.cotr_raster_last_error()
    assert wmap(map_=ctypes.c_void_p((1 << 30) + 8), f64=1) == -1 and b'aligned' in lib.cotr_raster_last_error()
    assert wpersp(M_=None) == -1 and b'M must not be NULL' in lib.cotr_raster_last_error()
    for bad in (float('nan'), float('inf')):
        Mb = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, bad, 1)
        assert wpersp(M_=Mb) == -1 and b'finite' in lib.cotr_raster_last_error()
