"""detect_keypoints without a device: the numpy restatement of the rule (tests/keypoints_oracle.py) against scipy, against
brute-force Python and against Python's big integers, the properties the rule promises (translation, ground truth), and the
wrapper's host logic."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

from cotr_amd import _lib
from cotr_amd.inference import ZoomEngine, detect_keypoints, detect_keypoints_tensors
from cotr_amd.inference import keypoints as kpmod
from tests import keypoints_oracle as ko


# ---- against scipy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(17, 23), (40, 33)])
def test_sobel_and_box_sums_equal_scipy_correlate(H, W):
    img = ko.noise(1, H, W, seed=H)[0]
    I = img.astype(np.int64)
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.int64)
    Ix, Iy = ko.sobel(img)
    assert np.array_equal(Ix[1:-1, 1:-1], ndimage.correlate(I, kx, mode='constant')[1:-1, 1:-1])
    assert np.array_equal(Iy[1:-1, 1:-1], ndimage.correlate(I, kx.T, mode='constant')[1:-1, 1:-1])
    assert not Ix[0].any() and not Ix[:, 0].any() and not Iy[-1].any() and not Iy[:, -1].any()
    for r in (1, 2, 3, 4):
        for v in (Ix * Ix, Ix * Iy, Iy * Iy):
            assert np.array_equal(ko.box_sum(v, r), ndimage.correlate(v, np.ones((2 * r + 1, 2 * r + 1), np.int64), mode='constant'))


@pytest.mark.parametrize('score', ko.SCORES)
@pytest.mark.parametrize('R', [1, 4, 8])
def test_candidates_equal_scipy_maximum_filter_without_ties(score, R):
    img = ko.noise(1, 60, 75, seed=R)[0]
    key, S = ko.keys_of(img, None, score, 2, 0)
    positive = key[key > 0]
    assert positive.size > 1000 and np.unique(positive).size == positive.size            # no ties: the rule is the plain maximum
    rank = np.unique(key, return_inverse=True)[1].reshape(key.shape)                     # order-preserving and small: scipy filters in double
    want = (key > 0) & (rank == ndimage.maximum_filter(rank, size=2 * R + 1, mode='constant', cval=0))
    assert np.array_equal(ko.candidates(key, S, R, 0.0), want) and want.sum() > 5
    ys, xs = np.nonzero(want)                                                            # no two within Chebyshev distance R
    d = np.maximum(np.abs(ys[:, None] - ys[None]), np.abs(xs[:, None] - xs[None]))
    assert (d[~np.eye(len(ys), dtype=bool)] > R).all()
    assert want.sum() <= -(-60 // (R + 1)) * -(-75 // (R + 1))


# ---- against brute force, for the tie rule ------------------------------------------------------------------------------------
def _brute(img, score, r, R, border, quality, min_score):
    """every step in Python integers and floats, pixel by pixel -> [(pixel, S)] in the rule's order"""
    H, W = img.shape
    px = [[int(v) for v in row] for row in img]
    m = max(border, r + 1)
    key, S = {}, {}
    for y in range(H):
        for x in range(W):
            key[y, x], S[y, x] = 0, 0.0
            if not (m <= y < H - m and m <= x < W - m):
                continue
            a = b = c = 0
            for v in range(y - r, y + r + 1):
                for u in range(x - r, x + r + 1):
                    ix = (px[v - 1][u + 1] + 2 * px[v][u + 1] + px[v + 1][u + 1]) - (px[v - 1][u - 1] + 2 * px[v][u - 1] + px[v + 1][u - 1])
                    iy = (px[v + 1][u - 1] + 2 * px[v + 1][u] + px[v + 1][u + 1]) - (px[v - 1][u - 1] + 2 * px[v - 1][u] + px[v - 1][u + 1])
                    a, b, c = a + ix * ix, b + ix * iy, c + iy * iy
            if score == 'harris':
                k = 64 * (a * c - b * b) - 3 * (a + c) ** 2
                s = float(k)
            else:
                s = float(a + c) - math.sqrt(float((a - c) ** 2 + 4 * b * b))
                k = int(np.float64(s).view(np.int64))
            if s > 0:
                key[y, x], S[y, x] = k, s
    cands = []
    for y in range(H):
        for x in range(W):
            if key[y, x] <= 0 or S[y, x] < min_score:
                continue
            best = True
            for v in range(y - R, y + R + 1):
                for u in range(x - R, x + R + 1):
                    if (v, u) == (y, x):
                        continue
                    q = key.get((v, u), 0)
                    if not (q < key[y, x] or (q == key[y, x] and v * W + u > y * W + x)):
                        best = False
            if best:
                cands.append((y * W + x, key[y, x], S[y, x]))
    if not cands:
        return [], 0
    smax = max(s for _, _, s in cands)
    alive = sorted((c for c in cands if c[2] >= quality * smax), key=lambda c: (-c[1], c[0]))
    return [(p, s) for p, _, s in alive], len(cands)


@pytest.mark.parametrize('score', ko.SCORES)
@pytest.mark.parametrize('R', [1, 2, 8])
def test_an_8_by_9_image_with_ties_equals_brute_force(score, R):
    half = ko.noise(1, 8, 5, seed=11)[0]
    img = np.concatenate([half, half[:, 3::-1]], axis=1)          # mirrored about column 4: keys come in equal pairs
    assert img.shape == (8, 9)
    key, _ = ko.keys_of(img, None, score, 1, 0)
    assert np.array_equal(key, key[:, ::-1]) and (key > 0).sum() >= 4
    for quality in (0.0, 0.5):
        want, n_cand = _brute(img, score, 1, R, 0, quality, 0.0)
        xy, s, pixel, info = ko.detect_one(img, None, score, 1, R, 0, quality, 0.0, 16)
        assert info.tolist() == [n_cand, len(want), len(want), 0] and n_cand >= 1
        assert pixel[:len(want)].tolist() == [p for p, _ in want] and s[:len(want)].tolist() == [v for _, v in want]
    if R == 8:                                                    # one window holds the image: of two equal maxima the first in raster order
        best = key.max()
        ys, xs = np.nonzero(key == best)
        assert len(ys) >= 2 and pixel[0] == (ys * 9 + xs).min() and info[0] == 1


# ---- the integers stay inside int64 ------------------------------------------------------------------------------------------
def _exact(img, r, y, x):
    """a, b, c and the harris key at one pixel in Python integers"""
    px = img.astype(object)
    a = b = c = 0
    for v in range(y - r, y + r + 1):
        for u in range(x - r, x + r + 1):
            ix = (px[v - 1, u + 1] + 2 * px[v, u + 1] + px[v + 1, u + 1]) - (px[v - 1, u - 1] + 2 * px[v, u - 1] + px[v + 1, u - 1])
            iy = (px[v + 1, u - 1] + 2 * px[v + 1, u] + px[v + 1, u + 1]) - (px[v - 1, u - 1] + 2 * px[v - 1, u] + px[v - 1, u + 1])
            a, b, c = a + ix * ix, b + ix * iy, c + iy * iy
    return int(a), int(b), int(c), int(64 * (a * c - b * b) - 3 * (a + c) ** 2)


def test_integer_bounds_at_window_radius_4():
    bound = 81 * 1020 ** 2
    assert bound < 2 ** 31 and 5 * bound ** 2 < 2 ** 63 and 64 * bound ** 2 + 3 * (2 * bound) ** 2 < 2 ** 63    # every term of both keys
    H, W, r = 24, 26, 4
    y, x = np.mgrid[:H, :W]
    images = {'columns': np.where(x % 2 == 0, 0, 255).astype(np.uint8), 'checkerboard': ko.checkerboard(H, W, 1),
              'squares': ko.checkerboard(H, W, 2), 'binary noise': (ko.noise(1, H, W, seed=3)[0] > 127).astype(np.uint8) * 255}
    for name, img in images.items():
        a, b, c = ko.tensor(img, r)
        assert 0 <= a.min() and a.max() <= bound and 0 <= c.min() and c.max() <= bound and np.abs(b).max() <= bound, name
        key, S = ko.keys_of(img, None, 'harris', r, 0)
        for (py, px) in [(5, 5), (5, 20), (12, 13), (18, 6), (18, 20), (11, 7)]:
            ea, eb, ec, ek = _exact(img, r, py, px)
            assert (a[py, px], b[py, px], c[py, px]) == (ea, eb, ec), name
            assert key[py, px] == max(ek, 0) and abs(ek) < 2 ** 63, name
        ko.detect_one(img, None, 'min_eig', r, 4, 0, 0.01, 0.0, 64)                      # runs; S stays finite
        assert np.isfinite(ko.keys_of(img, None, 'min_eig', r, 0)[1]).all()
    assert ko.tensor(images['squares'], r)[0].max() > 2 ** 24                             # the int32 row sums are needed


# ---- translation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('score', ko.SCORES)
def test_whole_pixel_shifts_move_keypoints_exactly(score):
    r, R = 2, 4
    canvas = ko.textured(1, 90, 110, seed=5)[0]
    H, W, reach = 64, 80, R + r + 1
    a = ko.detect_one(canvas[10:10 + H, 12:12 + W], None, score, r, R, 0, 0.0, 0.0, 4096)
    checked = 0
    for dy, dx in [(3, 0), (0, -5), (-7, 9)]:                     # the window moves by (-dy, -dx): the scene moves by (dy, dx) in it
        b = ko.detect_one(canvas[10 - dy:10 - dy + H, 12 - dx:12 - dx + W], None, score, r, R, 0, 0.0, 0.0, 4096)
        assert a[3][1] < 4096 and b[3][1] < 4096
        there = {int(p): (b[0][i], b[1][i]) for i, p in enumerate(b[2][:b[3][2]])}
        for i in range(a[3][2]):
            y, x = divmod(int(a[2][i]), W)
            inside = lambda v, u: reach < v < H - 1 - reach and reach < u < W - 1 - reach   # noqa: E731
            if inside(y, x) and inside(y + dy, x + dx):
                xy, s = there[(y + dy) * W + x + dx]
                # the pixel (the dictionary's key) and the score exactly; x + off is rounded once on either side, at coordinates
                # below 128, whose half ulp is 2^-47 each
                assert s == a[1][i] and (np.abs(xy - (a[0][i] + [dx, dy])) <= 2.0 ** -45).all()
                checked += 1
    assert checked > 30


# ---- ground truth -------------------------------------------------------------------------------------------------------------
GROUND_TRUTH_QUALITY = {'min_eig': 0.02, 'harris': 0.0005}


@pytest.mark.parametrize('score', ko.SCORES)
@pytest.mark.parametrize('r', [1, 2, 3])
def test_every_rectangle_corner_and_nothing_else(score, r):
    """Seeds 0 to 4 of keypoints_oracle.rectangles (a corner is the rectangle's corner pixel): 240 of 240 corners, no extras;
    worst distances 0.27 / 1.21 / 2.46 px for min_eig and 0.41 / 1.32 / 2.55 px for harris at r = 1 / 2 / 3."""
    for seed in range(5):
        img, corners = ko.rectangles(seed)
        xy, _, _, info = ko.detect_one(img, None, score, r, 4, 0, GROUND_TRUTH_QUALITY[score], 0.0, 2048)
        to_keypoint, to_corner = ko.corner_report(xy[:info[2]], corners)
        assert corners.shape == (48, 2) and (to_keypoint <= r + 1).all() and (to_corner <= r + 1).all(), (seed, to_keypoint.max(), to_corner.max())


# ---- the wrapper on the host --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw,word', [(dict(score='fast'), 'score'), (dict(max_keypoints=0), 'max_keypoints'), (dict(max_keypoints=65537), 'max_keypoints'),
                                     (dict(window_radius=0), 'window_radius'), (dict(window_radius=5), 'window_radius'),
                                     (dict(nms_radius=0), 'nms_radius'), (dict(nms_radius=9), 'nms_radius'), (dict(nms_radius=2.5), 'nms_radius'),
                                     (dict(border=-1), 'border'), (dict(quality=1.5), 'quality'), (dict(quality=-0.1), 'quality'),
                                     (dict(quality=float('nan')), 'quality'), (dict(min_score=float('nan')), 'min_score')])
def test_argument_errors_come_before_any_device_work(kw, word):
    with pytest.raises(ValueError, match=word):
        detect_keypoints_tensors(np.zeros((16, 16), np.uint8), **kw)


def test_shape_rules_and_cpu_tensors():
    with pytest.raises(ValueError, match='at least 2 max'):
        kpmod._check_shape(1, 6, 40, 2, 0)
    with pytest.raises(ValueError, match='at least 2 max'):
        kpmod._check_shape(1, 40, 14, 1, 7)
    kpmod._check_shape(1, 7, 7, 2, 0)
    kpmod._check_shape(64, 15, 15, 1, 7)
    with pytest.raises(ValueError, match='images in one call'):
        kpmod._check_shape(65, 40, 40, 2, 0)
    with pytest.raises(ValueError, match='2\\^28'):
        kpmod._check_shape(2, 1 << 14, 1 << 14, 2, 0)
    with pytest.raises(ValueError, match='2\\^20'):
        kpmod._check_shape(1, (1 << 20) + 1, 7, 2, 0)
    kpmod._check_shape(1, 1 << 20, 7, 2, 0)
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        detect_keypoints_tensors(torch.zeros((16, 16), dtype=torch.uint8))
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        detect_keypoints_tensors(np.zeros((16, 16), np.uint8), mask=torch.ones((16, 16), dtype=torch.uint8))
    with pytest.raises(ValueError, match='at least one image'):
        detect_keypoints([])
    with pytest.raises(ValueError, match='every image'):
        detect_keypoints([np.zeros((4, 16, 16, 3), np.uint8)])
    with pytest.raises(ValueError, match='one mask per image'):
        detect_keypoints([np.zeros((16, 16), np.uint8)] * 2, mask=[np.ones((16, 16), np.uint8)])


def test_host_form_groups_by_size_and_keeps_input_order(monkeypatch):
    calls = []

    def fake(images, mask=None, **kw):
        n, H, W = images.shape[:3]
        calls.append((n, H, W, images.shape[3:], None if mask is None else tuple(mask.shape), kw))
        xy = torch.full((n, 5, 2), float('nan'), dtype=torch.float64)
        info = torch.zeros((n, 4), dtype=torch.int32)
        for i in range(n):                                        # image i, tagged t in its first pixel, has t % 5 keypoints (t, H)
            t = int(np.asarray(images[i]).reshape(-1)[0])
            xy[i, :t % 5] = torch.tensor([float(t), float(H)], dtype=torch.float64)
            info[i, 2] = t % 5
        return dict(keypoints=xy, info=info)
    monkeypatch.setattr(kpmod, 'detect_keypoints_tensors', fake)
    shapes = [(20, 30), (16, 16), (20, 30), (20, 30, 3), (16, 16), (20, 30)]
    imgs = [np.full(s, 10 + i, np.uint8) for i, s in enumerate(shapes)]
    out = detect_keypoints(imgs, nms_radius=3)
    assert [c[:4] for c in calls] == [(3, 20, 30, ()), (2, 16, 16, ()), (1, 20, 30, (3,))] and all(c[5] == dict(nms_radius=3) for c in calls)
    for i, (o, s) in enumerate(zip(out, shapes)):
        assert o.dtype == np.float64 and o.shape == ((10 + i) % 5, 2) and (o == [10 + i, s[0]]).all()
    assert kpmod.group_by_size(shapes) == {(20, 30): [0, 2, 5], (16, 16): [1, 4], (20, 30, 3): [3]}
    calls.clear()
    one = detect_keypoints(imgs[3], mask=np.ones((20, 30), np.uint8))        # one image in, one array out; its mask stacked with it
    assert one.shape == (3, 2) and calls[0][:5] == (1, 20, 30, (3,), (1, 20, 30))
    calls.clear()
    batch = detect_keypoints(np.stack([imgs[0], imgs[2]]))                   # a batch is a list of its images
    assert len(batch) == 2 and calls[0][:3] == (2, 20, 30)
    calls.clear()
    assert len(detect_keypoints([imgs[1]] * 70)) == 70 and [c[0] for c in calls] == [64, 6]


def test_engine_methods_detect_when_no_keypoints_are_given(monkeypatch):
    seen = []

    def fake_detect(image_or_list, **kw):
        seen.append((len(image_or_list) if isinstance(image_or_list, list) else 1, kw))
        return [np.array([[1.0, 2.0], [3.0, 4.0]]) + i for i in range(len(image_or_list))]
    monkeypatch.setattr(kpmod, 'detect_keypoints', fake_detect)
    eng = ZoomEngine.__new__(ZoomEngine)
    imgs = [np.zeros((32, 32, 3), np.uint8)] * 3
    assert len(eng.detect_keypoints(imgs, nms_radius=2)) == 3 and seen[-1] == (3, dict(nms_radius=2))
    got = {}

    def fake_corr(self, img_a, img_b, zoom_ins=(1.0,), converge_iters=1, max_corrs=1000, queries_a=None, force=False, **kw):
        got.setdefault('queries', []).append(np.asarray(queries_a))
        return np.concatenate([queries_a, queries_a], axis=1)
    monkeypatch.setattr(ZoomEngine, 'cotr_corr_multiscale', fake_corr)
    import cotr_amd.inference.guided as guided
    monkeypatch.setattr(guided, 'mutual_matches', lambda ab, ba, ka, kb: np.array([[0, 0], [1, 1]]))
    with pytest.raises(ValueError, match='5 matches'):            # two keypoints a view: the downstream call's own refusal
        eng.reconstruct_keypoints(imgs, np.eye(3), detect_kw=dict(quality=0.5))
    assert seen[-1] == (3, dict(quality=0.5)) and np.array_equal(got['queries'][0], [[1.0, 2.0], [3.0, 4.0]])
    got.clear()
    monkeypatch.setattr(guided, 'filter_guided_matches', lambda ab, ba, ka, kb, **kw: (ka, kb, kw))
    ka, kb, kw = eng.guided_match(imgs[0], imgs[1], detect_kw=dict(border=4), seed=2)
    assert seen[-1] == (2, dict(border=4)) and np.array_equal(ka, [[1.0, 2.0], [3.0, 4.0]]) and np.array_equal(kb, [[2.0, 3.0], [4.0, 5.0]]) and kw == dict(seed=2)
    ka, kb, _ = eng.guided_match(imgs[0], imgs[1], np.zeros((4, 2)), None)   # only the missing set is detected
    assert seen[-1][0] == 1 and ka.shape == (4, 2) and kb.shape == (2, 2)
