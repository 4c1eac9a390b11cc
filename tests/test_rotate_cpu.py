"""The rotation augmentation without a GPU: the numpy restatement (tests/rotate_oracle.py) against hand-computed cases and
against the exact bilinear value within a derived bound, the pose rule against the reference's own rotate_camera_pose
(tests/golden/rotate_pose.npz), the property that pose and image turn the same way, draw_rotations, and the argument checks
of the Python layer and of the C entry point (they run before any HIP call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cotr_amd
from cotr_amd import _lib, data
from cotr_amd.build import declared_symbols
from cotr_amd.data import Capture
from tests import dataset_oracle as do
from tests import rotate_oracle as ro
from tests import warp_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLES = [1e-3, 17, -23.5, 45, 90, 180, 270, 359.999, -720.25]
IDENTITY = np.array([1.0, 0, 0, 0, 1.0, 0])


# ---- the restatement against hand-computed cases ------------------------------------------------------------------------
def test_identity_matrix_is_an_exact_copy():
    img, depth = wo.image(19, 23, 3, 0), ro.depth_map(19, 23, 0)
    X, Y = ro.linear_coords(IDENTITY, 19, 23)                       # (1024 x + 16) >> 5 = 32 x: fraction 0
    assert np.array_equal(X, 32 * np.arange(23)[None, :] + np.zeros((19, 1), np.int64))
    assert np.array_equal(Y, 32 * np.arange(19)[:, None] + np.zeros((1, 23), np.int64))
    assert np.array_equal(ro.warp_linear(img, IDENTITY), img)
    assert np.array_equal(ro.warp_nearest(depth, IDENTITY).view(np.uint32), depth.view(np.uint32))   # NaN payloads included
    assert np.isnan(depth).any() and (depth.view(np.uint32) == 0x80000000).any()


def test_half_turn_on_even_sides_mirrors_about_w_half_h_half():
    """180 degrees about (W/2, H/2) - not ((W-1)/2, (H-1)/2): dst[y, x] = src[H - y, W - x], so row 0 and column 0 are 0"""
    H, W = 12, 18
    img, depth = wo.image(H, W, 3, 1), ro.depth_map(H, W, 1, special=False) + np.float32(1)
    m = ro.matrix((H, W), 180)
    want_i, want_d = np.zeros_like(img), np.zeros_like(depth)
    want_i[1:, 1:] = img[:0:-1, :0:-1]
    want_d[1:, 1:] = depth[:0:-1, :0:-1]
    assert np.array_equal(ro.warp_linear(img, m), want_i)
    assert np.array_equal(ro.warp_nearest(depth, m), want_d)
    assert want_i[5, 7, 0] == img[H - 5, W - 7, 0]


def test_quarter_turn_on_a_square():
    """90 degrees on N x N: the source of (x, y) is (N - y, x), so dst[y, x] = src[x, N - y] and row 0 is 0"""
    N = 10
    img, depth = wo.image(N, N, 3, 2), ro.depth_map(N, N, 2, special=False) + np.float32(1)
    m = ro.matrix((N, N), 90)
    X, Y = ro.nearest_coords(m, N, N)
    assert np.array_equal(X, N - np.arange(N)[:, None] + np.zeros((1, N), np.int64))
    assert np.array_equal(Y, np.arange(N)[None, :] + np.zeros((N, 1), np.int64))
    want_i, want_d = np.zeros_like(img), np.zeros_like(depth)
    for y in range(1, N):
        want_i[y], want_d[y] = img[:, N - y], depth[:, N - y]
    assert np.array_equal(ro.warp_linear(img, m), want_i)
    assert np.array_equal(ro.warp_nearest(depth, m), want_d)


def test_one_by_one_source():
    img, depth = np.array([[[40, 80, 120]]], np.uint8), np.array([[3.5]], np.float32)
    assert np.array_equal(ro.warp_linear(img, IDENTITY), img) and np.array_equal(ro.warp_nearest(depth, IDENTITY), depth)
    # 45 degrees about (0.5, 0.5): the source of pixel (0, 0) is (0.5, 0.5 - sqrt(0.5)) = (0.5, -0.2071...)
    m = ro.matrix((1, 1), 45)
    assert abs(m[2] - 0.5) < 1e-15 and abs(m[5] - (0.5 - np.sqrt(0.5))) < 1e-15
    SX, SY = ro.sums(m, 1, 1)
    assert (SX[0, 0], SY[0, 0]) == (512, -212)                      # rint(512), rint(-212.08)
    X, Y = ro.linear_coords(m, 1, 1)
    assert (X[0, 0], Y[0, 0]) == (16, -7)                           # (512 + 16) >> 5, (-212 + 16) >> 5 = floor(-6.125)
    # ix = 0, fx = 16, iy = -1, fy = 25: only tap (0, 0) is inside, weight (32 - 16) * 25 = 400
    assert list(ro.warp_linear(img, m)[0, 0]) == [(400 * v + 512) >> 10 for v in (40, 80, 120)] == [16, 31, 47]
    X, Y = ro.nearest_coords(m, 1, 1)
    assert (X[0, 0], Y[0, 0]) == (1, 0)                             # (512 + 512) >> 10 = 1: 0.5 rounds up, out of the source
    assert ro.warp_nearest(depth, m)[0, 0] == 0.0


def test_ties_by_hand_and_the_side_they_fall_on():
    src = np.array([[0, 64]], np.uint8)

    def shift(tx):
        return np.array([1.0, 0, tx, 0, 1.0, 0])
    # a position on a 1/64-px tie goes UP under warpAffine's (+16) >> 5, where the perspective rule's rint(v * 32) goes to even:
    # x = 1/64: fx = 1 -> (1 * 32 * 64 + 512) >> 10 = 2; the rule of 3i gives fx = 0 -> 0
    X, _ = ro.linear_coords(shift(1 / 64), 1, 1)
    assert X[0, 0] == 1 and wo.fix(np.float32([1 / 64]))[0] == 0
    assert ro.warp_linear(src, shift(1 / 64))[0, 0] == 2 and wo.remap(src, np.float32([[[1 / 64, 0]]]))[0][0, 0] == 0
    # x = 3/64: both rules give fx = 2 -> (2 * 32 * 64 + 512) >> 10 = 4
    assert ro.linear_coords(shift(3 / 64), 1, 1)[0][0, 0] == 2 and ro.warp_linear(src, shift(3 / 64))[0, 0] == 4
    # negative ties go up as well: -1/64 -> (-16 + 16) >> 5 = 0; -3/64 -> (-48 + 16) >> 5 = -1 = ix -1, fx 31
    assert ro.linear_coords(shift(-1 / 64), 1, 1)[0][0, 0] == 0
    Xn = ro.linear_coords(shift(-3 / 64), 1, 1)[0][0, 0]
    assert Xn == -1 and Xn >> 5 == -1 and Xn & 31 == 31
    # the table rounding itself is to even: m2 * 1024 = 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> 0, -1.5 -> -2
    assert [int(ro.sums(shift(k / 1024), 1, 1)[0][0, 0]) for k in (0.5, 1.5, 2.5, -0.5, -1.5)] == [0, 2, 2, 0, -2]
    # nearest: a source position of exactly k + 0.5 takes pixel k + 1: (512 + 512) >> 10 = 1; just below stays at 0
    d = np.array([[1.0, 2.0]], np.float32)
    assert ro.warp_nearest(d, shift(0.5))[0, 0] == 2.0 and ro.warp_nearest(d, shift(0.5 - 1 / 1024))[0, 0] == 1.0
    assert ro.warp_nearest(d, shift(-0.5))[0, 0] == 1.0 and ro.warp_nearest(d, shift(-0.5 - 1 / 1024))[0, 0] == 0.0


def test_matrix_helper_equals_the_restatement_and_inverts_the_forward_rotation():
    for shape in ((1, 1), (5, 7), (48, 64), (480, 640), (16384, 16384)):
        for a in ANGLES + [0.0]:
            m = data.rotation_matrix(shape, a)
            assert m.dtype == np.float64 and m.shape == (6,) and np.array_equal(m, ro.matrix(shape, a))
            t = np.deg2rad(a)
            fwd = np.array([[np.cos(t), np.sin(t), (1 - np.cos(t)) * shape[1] / 2 - np.sin(t) * shape[0] / 2],
                            [-np.sin(t), np.cos(t), np.sin(t) * shape[1] / 2 + (1 - np.cos(t)) * shape[0] / 2], [0, 0, 1]])
            assert np.abs(np.vstack([m.reshape(2, 3), [0, 0, 1]]) @ fwd - np.eye(3)).max() < 1e-8
            # no fixed-point value of a rotation of sides <= 16384 leaves 2^26 (the kernel's int32 is enough)
            assert abs(m[2]) <= 2 * 16384 and abs(m[5]) <= 2 * 16384
    assert cotr_amd.rotation_matrix is data.rotation_matrix


# ---- the independent bound ------------------------------------------------------------------------------------------------
def test_restatement_is_within_the_derived_bound_of_exact_bilinear():
    """|restatement - exact| <= 0.5 + (Gx + Gy) (1/64 + 1/1024): the two table roundings (X0, ad) move a coordinate by at most
    1/1024 px together, the (+16) >> 5 step by at most 1/64; the quantised position can leave the exact position's cell, so G is
    the largest tap difference over the 3 x 3 cells around it; the bilinear surface is continuous and piecewise linear in
    each coordinate with slope at most G; (sum + 512) >> 10 is the exact value at the quantised position rounded, at most 0.5
    more.  Measured position error at 17 degrees on 48 x 64: 0.01649 px (bound 0.01660)."""
    rng = np.random.default_rng(0)
    worst, worst_pos = 0.0, 0.0
    for H, W in ((48, 64), (37, 53), (1, 9), (2, 2)):
        for img in (wo.image(H, W, 3, 3), rng.integers(0, 256, (H, W, 3)).astype(np.uint8)):
            for a in ANGLES:
                m = ro.matrix((H, W), a)
                X, Y = ro.linear_coords(m, H, W)
                u, v = ro.affine_position(m, H, W)
                pos = max(np.abs(X / 32 - u).max(), np.abs(Y / 32 - v).max())
                assert pos <= ro.POS_ERR + 1e-12, (H, W, a, pos)
                worst_pos = max(worst_pos, pos)
                if (H, W, a) == (48, 64, 17):
                    assert abs(pos - 0.01649) < 5e-6
                value, Gx, Gy = ro.exact(img, m)
                err = np.abs(ro.warp_linear(img, m).astype(np.float64) - value)
                slack = 0.5 + (Gx + Gy) * ro.POS_ERR - err
                assert (slack >= -1e-9).all(), (H, W, a, err.max(), float(slack.min()))   # (1e-9: the float64 evaluation of `exact`)
                worst = max(worst, err.max())
    print('largest |restatement - exact|', worst, 'largest position error', worst_pos)
    assert worst > 0.4 and worst_pos > 1 / 64                       # the cases do exercise the rounding


def test_nearest_takes_the_pixel_whose_centre_is_nearest():
    for a in ANGLES:
        m = ro.matrix((48, 64), a)
        X, Y = ro.nearest_coords(m, 48, 64)
        u, v = ro.affine_position(m, 48, 64)
        for got, pos in ((X, u), (Y, v)):
            clear = np.abs(pos + 0.5 - np.rint(pos + 0.5)) > 2 / 1024            # not within the table roundings of a half
            assert np.array_equal(got[clear], np.floor(pos + 0.5).astype(np.int64)[clear])
            assert (np.abs(got - pos) <= 0.5 + 1 / 1024 + 1e-12).all()


# ---- the pose ---------------------------------------------------------------------------------------------------------------
def test_rotated_c2w_against_the_references_rotate_camera_pose():
    """tests/golden/rotate_pose.npz holds what the reference's rotate_camera_pose returned.  The difference is the float32
    quaternion + translation the reference stores its result as: the largest |ours - reference| over the largest |entry| of a
    pose, over the golden, is 1.19e-7 (float32 rounding); asserted at ten times that.  A wrong sign or a row / column mix-up
    would show as about 1e-2 or more."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'rotate_pose.npz'))
    assert len(g['angles']) >= 12 and set(g['angles']) >= {0.0, 17.0, -17.0, 45.0, 90.0, 180.0, -123.4}
    worst = 0.0
    for a, c_in, c_out in zip(g['angles'], g['c2w_in'], g['c2w_out']):
        got = data.rotated_c2w(c_in, a)
        assert got.dtype == np.float64 and got.shape == (4, 4)
        rel = np.abs(got - c_out).max() / np.abs(c_out).max()
        worst = max(worst, rel)
        assert rel <= 1.2e-6, (a, rel)
        if a:
            assert np.abs(ro.rotated_c2w(c_in, a) - got).max() <= 1e-12
            assert np.abs(got - c_in).max() > 1e-2                  # the pose did turn
        else:
            assert got is c_in                                      # angle 0: as it is
    print('largest relative difference to the reference', worst)
    assert worst > 1e-9                                             # the golden does carry the float32 storage


@pytest.mark.parametrize('angle', [17, -40, 90])
def test_pose_and_image_turn_the_same_way(angle):
    cap, m = ro.property_case(angle)
    ro.check_turns_the_same_way(cap, ro.rotate_capture(cap, angle), m)
    # the other sign convention is off by far more than the tolerance
    wrong = cap._replace(c2w=ro.rotated_c2w(cap.c2w, -angle), depth=ro.warp_nearest(cap.depth, m))
    r = do.reproject(wrong.depth, cap.depth, cap.K, wrong.c2w, cap.K, cap.c2w)
    u, _ = ro.affine_position(m, *cap.depth.shape)
    assert np.abs(r['uv'][:, 0] - u.reshape(-1))[wrong.depth.reshape(-1) > 0].max() > 1.0


# ---- draw_rotations -----------------------------------------------------------------------------------------------------------
def test_draw_rotations():
    rot = data.draw_rotations(5, 30.0, 0.5, np.random.default_rng(7))
    assert rot.shape == (5, 2) and rot.dtype == np.float64
    u = np.random.default_rng(7).random(20).reshape(5, 2, 2)        # per sample: query (u_c, u_t), then nn (u_c, u_t)
    want = np.where(u[..., 0] < 0.5, (2 * u[..., 1] - 1) * 30.0, 0.0)
    assert np.array_equal(rot, want) and (rot == 0).any() and (rot != 0).any()
    assert np.array_equal(rot, data.draw_rotations(5, 30.0, 0.5, np.random.default_rng(7)))          # the same seed
    assert not np.array_equal(rot, data.draw_rotations(5, 30.0, 0.5, np.random.default_rng(8)))
    assert not data.draw_rotations(64, 30.0, 0.0, np.random.default_rng(1)).any()                    # chance 0
    full = data.draw_rotations(64, 30.0, 1.0, np.random.default_rng(1))                              # chance 1
    assert (np.abs(full) <= 30.0).all() and (full != 0).all() and full.min() < -15 and full.max() > 15
    gen = np.random.default_rng(2)
    a, b = data.draw_rotations(3, 10.0, 1.0, gen), data.draw_rotations(3, 10.0, 1.0, gen)            # the generator advances
    assert not np.array_equal(a, b)
    assert data.draw_rotations(2, 10.0, 0.5).shape == (2, 2)                                         # a generator of its own
    assert cotr_amd.draw_rotations is data.draw_rotations and data.draw_rand.__defaults__ == (data.MAX_TRY, None, None)
    assert list(data._RAND_SHAPES) == ['seed', 'zoom', 'jitter', 'trim', 'flip']
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match='batch'):
            data.draw_rotations(bad, 10.0, 0.5)
    with pytest.raises(ValueError, match='finite'):
        data.draw_rotations(2, np.nan, 0.5)


# ---- the Python layer's argument checks ---------------------------------------------------------------------------------------
def _cap(H=4, W=5, image=True):
    return Capture(np.zeros((H, W, 3), np.uint8) if image else None, np.zeros((H, W), np.float32), np.eye(3), np.eye(4))


def test_wrapper_argument_errors_without_a_gpu():
    for name in ('rotation_matrix', 'rotated_c2w', 'rotate_captures', 'rotate_capture', 'rotate_image', 'draw_rotations'):
        assert name in cotr_amd.__all__ and getattr(cotr_amd, name) is getattr(data, name)
    for bad in ([1.0], [1.0, 2.0, 3.0], [1.0, np.nan], [np.inf, 0.0], ['a', 'b'], None, [[1.0, 2.0]], 5.0):
        with pytest.raises(ValueError, match='finite floats'):
            data.rotate_captures([_cap(), _cap()], bad)
    with pytest.raises(ValueError, match='finite'):
        data.rotate_capture(_cap(), np.nan)
    with pytest.raises(ValueError, match='finite'):
        data.rotate_capture(_cap(), 'x')
    with pytest.raises(ValueError, match='non-empty'):
        data.rotate_captures([], [])
    with pytest.raises(ValueError, match='16384'):
        data.rotate_captures([Capture(None, np.zeros((1, 16385), np.float32), np.eye(3), np.eye(4))], [3.0])
    with pytest.raises(ValueError, match='16384'):
        data.rotate_captures([Capture(None, np.zeros((16385, 1), np.float32), np.eye(3), np.eye(4))], [3.0])
    with pytest.raises(ValueError, match='float32'):
        data.rotate_captures([_cap()._replace(depth=np.zeros((4, 5), np.float64))], [3.0])
    with pytest.raises(ValueError, match=r'\[H, W, 3\]'):
        data.rotate_captures([_cap()._replace(image=np.zeros((4, 6, 3), np.uint8))], [3.0])
    with pytest.raises(ValueError, match='c2w'):
        data.rotate_captures([_cap()._replace(c2w=np.eye(4, dtype=np.float32))], [3.0])
    with pytest.raises(ValueError, match='Capture'):
        data.rotate_captures([np.zeros((4, 5), np.float32)], [3.0])
    # a CPU tensor is not a device tensor: no fallback, whatever the angle
    for angle in (3.0, 0.0):
        with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
            data.rotate_captures([_cap()._replace(depth=torch.zeros(4, 5))], [angle])
        with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
            data.rotate_captures([_cap()._replace(image=torch.zeros(4, 5, 3, dtype=torch.uint8))], [angle])
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        data.rotate_image(torch.zeros(4, 5, 3, dtype=torch.uint8), 3.0)
    with pytest.raises(ValueError, match=r'uint8 \[H, W, 3\]'):
        data.rotate_image(np.zeros((4, 5), np.uint8), 3.0)
    with pytest.raises(ValueError, match=r'uint8 \[H, W, 3\]'):
        data.rotate_image(np.zeros((4, 5, 3), np.float32), 3.0)
    with pytest.raises(ValueError, match=r'float32 \[H, W\]'):
        data.rotate_image(np.zeros((4, 5, 3), np.uint8), 3.0, nearest=True)
    with pytest.raises(ValueError, match=r'float32 \[H, W\]'):
        data.rotate_image(np.zeros((4, 5), np.float64), 3.0, nearest=True)
    with pytest.raises(ValueError, match='16384'):
        data.rotate_image(np.zeros((1, 16385), np.float32), 3.0, nearest=True)
    with pytest.raises(ValueError, match='finite'):
        data.rotate_image(np.zeros((4, 5), np.float32), np.inf, nearest=True)
    with pytest.raises(ValueError, match='numpy array or a device tensor'):
        data.rotate_image([[1.0]], 3.0, nearest=True)
    with pytest.raises(ValueError, match='16384'):
        data.rotation_matrix((0, 5), 3.0)
    with pytest.raises(ValueError, match='16384'):
        data.rotation_matrix((5, 16385), 3.0)
    with pytest.raises(ValueError, match='finite'):
        data.rotation_matrix((4, 5), np.nan)
    with pytest.raises(ValueError, match='4 x 4'):
        data.rotated_c2w(np.eye(3), 3.0)
    with pytest.raises(ValueError, match='4 x 4'):
        data.rotated_c2w(np.eye(4) * np.nan, 3.0)
    with pytest.raises(ValueError, match='finite'):
        data.rotated_c2w(np.eye(4), np.inf)
    # the batch builders check `rotations` before any upload
    caps = [_cap(256, 256), _cap(256, 256)]
    for bad in (np.zeros((2, 3)), np.zeros(2), np.zeros((1, 2)), np.full((2, 2), np.nan), [[0.0, 'x'], [0.0, 0.0]]):
        with pytest.raises(ValueError, match=r'rotations \[B, 2\]'):
            data.make_batch(caps, caps, 10, rotations=bad)
        with pytest.raises(ValueError, match=r'rotations \[B, 2\]'):
            data.make_zoom_batch(caps, caps, 10, [1.0], 0.1, rotations=bad)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    assert 'cotr_rotate_captures' in declared_symbols() and 'cotr_rotate_captures' in _lib.EXPORTED_SYMBOLS
    lib = _lib.load_library()
    assert lib.cotr_abi_version() == 2 and callable(lib.cotr_rotate_captures)
    from cotr_amd import build
    assert 'rotate.hip' in build.SOURCES and build.EXTRA_FLAGS['rotate.hip'] == ['-ffp-contract=off'] and 'warp_taps.h' in build.HEADERS
    # one tap body: warp.hip and rotate.hip include it, neither restates it
    for f in ('warp.hip', 'rotate.hip'):
        src = open(os.path.join(build.CSRC, f)).read()
        assert '#include "warp_taps.h"' in src and 'bool sample(' not in src


def test_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    P, Q, R = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 31)   # never dereferenced

    def call(ptrs=P, shapes=Q, mats=R, n=1, max_h=8, max_w=8):
        return lib.cotr_rotate_captures(ptrs, shapes, mats, n, max_h, max_w, None)
    cases = [(dict(ptrs=None), b'NULL'), (dict(shapes=None), b'NULL'), (dict(mats=None), b'NULL'),
             (dict(n=0), b'[1, 65535]'), (dict(n=-1), b'[1, 65535]'), (dict(n=65536), b'[1, 65535]'),
             (dict(max_h=0), b'[1, 16384]'), (dict(max_w=0), b'[1, 16384]'), (dict(max_h=16385), b'[1, 16384]'),
             (dict(max_w=16385), b'[1, 16384]'), (dict(max_h=-5), b'[1, 16384]'),
             (dict(ptrs=ctypes.c_void_p((1 << 20) + 4)), b'aligned'), (dict(mats=ctypes.c_void_p((1 << 31) + 4)), b'aligned'),
             (dict(shapes=ctypes.c_void_p((1 << 30) + 2)), b'aligned')]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())
