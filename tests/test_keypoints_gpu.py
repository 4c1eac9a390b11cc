"""cotr_detect_keypoints on the device against tests/keypoints_oracle.py: bit for bit at every edge of the kernel's widths,
ties, tile borders, repeatability, guard bands, and the chain it starts."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import ZoomEngine, detect_keypoints, detect_keypoints_tensors
from tests import keypoints_oracle as ko
from tests import structure_oracle as so
from tests.guard_arena import Arena, GuardError

pytestmark = pytest.mark.gpu

OUTPUTS = ('keypoints', 'scores', 'pixel', 'info')


def host(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def agree(got, want, what=''):
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, what)
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, what, got['info'].tolist(), want['info'].tolist())


def both(images, mask=None, score='min_eig', r=2, R=4, border=0, quality=0.01, min_score=0.0, K=64):
    got = host(detect_keypoints_tensors(images, mask=mask, max_keypoints=K, score=score, window_radius=r, nms_radius=R, border=border,
                                        quality=quality, min_score=min_score))
    return got, ko.detect(images, mask, score, r, R, border, quality, min_score, K)


# ---- exact equality at the width edges ----------------------------------------------------------------------------------------
# the tile is 32 x 32: one below, at and one above one and two tiles, in both axes and mixed; 'smallest' is 2 max(border, r+1) + 1
SIZES = [(31, 65), (32, 64), (33, 63), (63, 33), (64, 32), (65, 31), 'smallest']


@pytest.mark.parametrize('score', ko.SCORES)
@pytest.mark.parametrize('size', SIZES, ids=str)
def test_equals_the_oracle_bit_for_bit(size, score):
    """H, W in {31, 32, 33, 63, 64, 65} around the 32-pixel tile and the smallest legal size (5, 11 or 15 pixels square); r in
    {1, 4}; R in {1, 4, 8}; n in {1, 3}; border in {0, 7}; with and without a mask; quality in {0, 0.01, 1}; K one below, at and
    one above the survivor count."""
    calls = cut = 0
    for r in (1, 4):
        for border in (0, 7):
            H, W = (2 * max(border, r + 1) + 1,) * 2 if size == 'smallest' else size
            for n in (1, 3):
                images = ko.textured(n, H, W, seed=H * 131 + W + n)
                for with_mask in (False, True):
                    mask = ko.random_mask(n, H, W, seed=W) if with_mask else None
                    for R in (1, 4, 8):
                        for quality in (0.0, 0.01, 1.0):
                            kw = dict(mask=mask, score=score, r=r, R=R, border=border, quality=quality)
                            got, want = both(images, K=64, **kw)
                            agree(got, want, (H, W, kw))
                            if quality == 0.01:
                                s = int(want['info'][:, 1].max())
                                for K in sorted({max(1, s - 1), max(1, s), s + 1}):
                                    got, want = both(images, K=K, **kw)
                                    agree(got, want, (H, W, K, kw))
                                    cut += int((want['info'][:, 1] > K).any())
                                    calls += 1
                            calls += 1
    assert calls > 200 and (cut > 0 or size == 'smallest')


def test_min_score_and_large_k():
    images = ko.textured(2, 70, 90, seed=2)
    base = ko.detect(images, None, 'min_eig', 2, 2, 0, 0.0, 0.0, 4096)
    floor = float(np.nanmedian(base['scores']))
    for min_score in (floor, np.nextafter(floor, np.inf), -np.inf, np.inf):
        got, want = both(images, R=2, quality=0.0, min_score=min_score, K=4096)
        agree(got, want, min_score)
    assert want['info'][:, 0].tolist() == [0, 0] and base['info'][0, 2] > 50


# ---- ties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('score', ko.SCORES)
def test_ties(score):
    flat = np.full((1, 40, 50), 93, np.uint8)                     # a constant image: no keypoints
    got, want = both(flat, score=score, quality=0.0)
    agree(got, want)
    assert not got['info'].any() and np.isnan(got['keypoints']).all() and (got['pixel'] == -1).all()
    board = ko.checkerboard(70, 90, 8)[None]                      # many identical keys: equal scores come in raster order
    for R in (1, 4):
        got, want = both(board, score=score, R=R, quality=0.0, K=256)
        agree(got, want, R)
        k = int(got['info'][0, 2])
        s, p = got['scores'][0, :k], got['pixel'][0, :k]
        assert k > 40 and np.unique(s).size < k // 4 and (np.diff(s) <= 0).all() and (np.diff(p)[np.diff(s) == 0] > 0).all()
    twins = np.full((1, 40, 48), 40, np.uint8)                    # two 3 x 3 blobs: six equal maxima in one row, inside one window
    twins[0, 19:22, 14:17] = twins[0, 19:22, 19:22] = 220
    key, _ = ko.keys_of(twins[0], None, score, 2, 0)
    ys, xs = np.nonzero(key == key.max())
    assert len(ys) == 6 and (ys == 20).all() and xs.tolist() == [15, 16, 17, 18, 19, 20]
    got, want = both(twins, score=score, R=8, quality=0.0)
    agree(got, want)
    assert got['info'][0].tolist() == [1, 1, 1, 0] and got['pixel'][0, 0] == 20 * 48 + 15


def test_maxima_on_tile_borders_and_corners():
    centres = [(31, 50), (32, 50), (50, 31), (50, 32), (31, 31), (31, 32), (32, 31), (32, 32), (63, 64), (64, 63), (63, 31), (32, 64)]
    images = np.full((len(centres), 96, 96), 40, np.uint8)
    for i, (cy, cx) in enumerate(centres):
        images[i, cy - 1:cy + 2, cx - 1:cx + 2] = 220
    for score in ko.SCORES:
        for r, R in ((1, 1), (2, 4), (2, 8), (4, 8)):
            got, want = both(images, score=score, r=r, R=R)
            agree(got, want, (score, r, R))
            d = max(0, r - 2)                                     # a box wider than the blob sees all of it from a plateau: its first pixel wins
            assert got['pixel'][:, 0].tolist() == [(cy - d) * 96 + cx - d for cy, cx in centres] and got['info'][:, 2].tolist() == [1] * len(centres)
    many = np.full((1, 96, 96), 40, np.uint8)                     # all of them in one image, 16 pixels apart or more
    for cy, cx in [(31, 31), (31, 48), (32, 64), (48, 32), (63, 63), (64, 31), (64, 80), (80, 64)]:
        many[0, cy - 1:cy + 2, cx - 1:cx + 2] = 220
    got, want = both(many, R=4)
    agree(got, want)
    assert got['info'][0, 2] == 8


# ---- repeatability and the raw ABI --------------------------------------------------------------------------------------------
def _work_bytes(lib, n, H, W, R):
    count = ctypes.c_size_t()
    assert lib.cotr_detect_keypoints_work_bytes(n, H, W, R, ctypes.byref(count)) == 0, lib.cotr_raster_last_error()
    return count.value


def test_same_bytes_across_calls_and_graph_replays():
    lib = _lib.load_library()
    n, H, W, K, R = 3, 150, 170, 300, 2
    images = torch.from_numpy(ko.textured(n, H, W, seed=77)).cuda()
    first = host(detect_keypoints_tensors(images, max_keypoints=K, nms_radius=R, quality=0.0))
    again = host(detect_keypoints_tensors(images, max_keypoints=K, nms_radius=R, quality=0.0))
    assert (first['info'][:, 1] > K).all()
    for k in OUTPUTS:
        assert first[k].tobytes() == again[k].tobytes(), k
    spec = dict(keypoints=((n, K, 2), torch.float64), scores=((n, K), torch.float64), pixel=((n, K), torch.int32), info=((n, 4), torch.int32))
    out = {k: torch.full(shape, -7, dtype=dt, device='cuda') for k, (shape, dt) in spec.items()}
    work = torch.full((_work_bytes(lib, n, H, W, R),), 0xA5, dtype=torch.uint8, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.cotr_detect_keypoints(p(images), None, n, H, W, 0, 2, R, 0, 0.0, 0.0, K, p(out['keypoints']), p(out['scores']), p(out['pixel']),
                                       p(out['info']), p(work), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.cotr_raster_last_error()
    for _ in range(2):
        for t in out.values():
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for k in OUTPUTS:
            assert out[k].cpu().numpy().tobytes() == first[k].tobytes(), k


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load_library()
    t = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    a = ctypes.c_void_p(t.data_ptr())
    good = dict(n=1, H=16, W=16, score=0, r=2, R=4, border=0, quality=0.01, min_score=0.0, K=8)
    for change, word in [(dict(n=0), 'n must'), (dict(n=65), 'n must'), (dict(score=2), 'score'), (dict(r=0), 'window_radius'), (dict(r=5), 'window_radius'),
                         (dict(R=0), 'nms_radius'), (dict(R=9), 'nms_radius'), (dict(border=-1), 'border'), (dict(H=6), 'at least'), (dict(W=14, border=7), 'at least'),
                         (dict(quality=1.5), 'quality'), (dict(quality=float('nan')), 'quality'), (dict(min_score=float('nan')), 'min_score'),
                         (dict(K=0), 'max_keypoints'), (dict(K=65537), 'max_keypoints'), (dict(n=64, H=2048, W=2049), '2\\^28'), (dict(H=(1 << 20) + 1, W=16), '2\\^20'), (dict(H=16, W=(1 << 20) + 1), '2\\^20')]:
        g = dict(good, **change)
        rc = lib.cotr_detect_keypoints(a, None, g['n'], g['H'], g['W'], g['score'], g['r'], g['R'], g['border'], g['quality'], g['min_score'], g['K'],
                                       a, a, a, a, a, None)
        assert rc == -1 and word.replace('\\', '') in lib.cotr_raster_last_error().decode(), (change, lib.cotr_raster_last_error())
    odd = ctypes.c_void_p(t.data_ptr() + 4)
    assert lib.cotr_detect_keypoints(a, None, 1, 16, 16, 0, 2, 4, 0, 0.01, 0.0, 8, a, a, a, a, odd, None) == -1
    assert lib.cotr_detect_keypoints(a, None, 1, 16, 16, 0, 2, 4, 0, 0.01, 0.0, 8, a, a, a, a, None, None) == -1
    assert lib.cotr_detect_keypoints_work_bytes(1, 16, 16, 9, ctypes.byref(ctypes.c_size_t())) == -1
    torch.cuda.synchronize()
    assert not t.any()


# ---- guard bands --------------------------------------------------------------------------------------------------------------
def _guarded(lib, images, mask, score, r, R, border, quality, K, fill, early=0):
    n, H, W = images.shape
    a = Arena('cuda', fill)
    a.add_input('images', images)
    if mask is not None:
        a.add_input('mask', mask)
    a.add_output('keypoints', np.float64, (n, K, 2)).add_output('scores', np.float64, (n, K)).add_output('pixel', np.int32, (n, K))
    a.add_output('info', np.int32, (n, 4)).add('work', _work_bytes(lib, n, H, W, R), 'a8', early_rear_band=early)
    a.build()
    rc = lib.cotr_detect_keypoints(a.ptr('images'), a.ptr('mask') if mask is not None else None, n, H, W, ko.SCORES.index(score), r, R, border,
                                   quality, 0.0, K, a.ptr('keypoints'), a.ptr('scores'), a.ptr('pixel'), a.ptr('info'), a.ptr('work'), None)
    assert rc == 0, lib.cotr_raster_last_error()
    torch.cuda.synchronize()
    a.check()
    return dict(keypoints=a.view('keypoints', np.float64, (n, K, 2)), scores=a.view('scores', np.float64, (n, K)),
                pixel=a.view('pixel', np.int32, (n, K)), info=a.view('info', np.int32, (n, 4)))


@pytest.mark.parametrize('n,H,W,r', [(1, 5, 5, 1), (1, 11, 11, 4), (1, 65, 33, 2), (3, 65, 33, 2), (3, 33, 65, 4)])
def test_between_guard_bands(n, H, W, r):
    """every buffer at its documented minimum alignment (images and mask at odd addresses, work_out at 8 mod 16 and exactly
    cotr_detect_keypoints_work_bytes long): no band byte and no input byte changes, and the outputs are the oracle's"""
    lib = _lib.load_library()
    images, mask = ko.textured(n, H, W, seed=H + W + n), ko.random_mask(n, H, W, seed=5)
    for fill in (0xA5, 0x00):
        for R in (1, 8):
            for score in ko.SCORES:
                for m in (None, mask):
                    want = ko.detect(images, m, score, r, R, 0, 0.01, 0.0, 7)
                    agree(_guarded(lib, images, m, score, r, R, 0, 0.01, 7, fill), want, (fill, R, score, m is not None))


def test_the_guard_trips_when_the_work_band_starts_early():
    """the control: the rear band of work_out begins 256 bytes early, on the last region (the largest keys), which the first
    launch clears"""
    lib = _lib.load_library()
    images = ko.textured(3, 65, 33, seed=1)
    _guarded(lib, images, None, 'min_eig', 2, 4, 0, 0.01, 7, 0xA5)
    with pytest.raises(GuardError, match="rear band of 'work'"):
        _guarded(lib, images, None, 'min_eig', 2, 4, 0, 0.01, 7, 0xA5, early=256)


# ---- the chain ----------------------------------------------------------------------------------------------------------------
GROUND_TRUTH_QUALITY = {'min_eig': 0.02, 'harris': 0.0005}


@pytest.mark.parametrize('score', ko.SCORES)
def test_every_rectangle_corner_and_nothing_else_on_the_device(score):
    """the conditions of tests/test_keypoints_cpu.py, seeds 0 to 4 as one batch, through the host form, grey and RGB"""
    scenes = [ko.rectangles(seed) for seed in range(5)]
    for r in (1, 2, 3):
        kw = dict(score=score, window_radius=r, nms_radius=4, quality=GROUND_TRUTH_QUALITY[score])
        found = detect_keypoints([img for img, _ in scenes], **kw)
        for (img, corners), xy in zip(scenes, found):
            to_keypoint, to_corner = ko.corner_report(xy, corners)
            assert xy.shape == (48, 2) and (to_keypoint <= r + 1).all() and (to_corner <= r + 1).all()
        rgb = detect_keypoints(np.repeat(scenes[0][0][:, :, None], 3, axis=2), **kw)      # R = G = B: to_grey gives the level back
        assert np.array_equal(rgb, found[0])


def test_host_form_with_sizes_mixed_equals_the_oracle():
    imgs = [ko.textured(1, *s, seed=i)[0] for i, s in enumerate([(40, 50), (33, 31), (40, 50), (64, 64)])]
    masks = [ko.random_mask(1, *im.shape, seed=9)[0] for im in imgs]
    out = detect_keypoints(imgs, mask=masks, max_keypoints=40, nms_radius=3)
    for im, m, xy in zip(imgs, masks, out):
        want = ko.detect_one(im, m, 'min_eig', 2, 3, 0, 0.01, 0.0, 40)
        assert np.array_equal(xy, want[0][:want[3][2]]) and len(xy) > 3


def test_zoom_engine_reconstruct_keypoints_detects_its_own(monkeypatch):
    """a posed scene drawn as 5 x 5 squares at its points; correspondences come from the scene (the network is not under test):
    the chain from photographs to poses runs with no keypoints given and returns the dict.  No accuracy is asserted."""
    V, N = 3, 80
    sc = so.scene(V, N, seed=757, noise=0.0)
    imgs = []
    for v in range(V):
        img = np.full((480, 640), 50, np.uint8)
        for x, y in np.rint(sc['points'][v]).astype(int):
            if 10 <= x < 630 and 10 <= y < 470:
                img[y - 2:y + 3, x - 2:x + 3] = 230
        imgs.append(np.repeat(img[:, :, None], 3, axis=2))
    tag = {id(im): v for v, im in enumerate(imgs)}
    queries = {}

    def fake(self, img_a, img_b, zoom_ins=(1.0,), converge_iters=1, max_corrs=1000, queries_a=None, force=False, **kw):
        a, b = tag[id(img_a)], tag[id(img_b)]
        queries[a] = np.asarray(queries_a)
        near = np.linalg.norm(queries_a[:, None, :] - sc['points'][a][None].astype(np.float64), axis=2).argmin(axis=1)
        return np.concatenate([queries_a, queries_a + (sc['points'][b][near] - sc['points'][a][near])], axis=1)
    monkeypatch.setattr(ZoomEngine, 'cotr_corr_multiscale', fake)
    eng = ZoomEngine.__new__(ZoomEngine)
    Ks = np.stack([so.camera_matrix(c) for c in sc['cams']])
    r = eng.reconstruct_keypoints(imgs, Ks, span=1, detect_kw=dict(max_keypoints=512), pose_kw=dict(threshold=2.0, max_iters=200, seed=3), bundle_rounds=1)
    want = eng.detect_keypoints(imgs, max_keypoints=512)
    assert all(np.array_equal(queries[v], want[v]) and len(want[v]) >= 40 for v in range(V))
    assert tuple(r['c2w'].shape) == (V, 4, 4) and 'tracks' in r and tuple(r['tracks']['info'].shape) == (8,)
