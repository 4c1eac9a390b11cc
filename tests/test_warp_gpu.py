"""cotr_warp_map / cotr_warp_perspective and their Python callers on the MI355X against the numpy restatement
(tests/warp_oracle.py): dst and cover IDENTICAL, at sizes that are and are not multiples of the 64 x 16 tile and of the four
pixels a lane writes."""
import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import (get_perspective_transform, paste_by_corners, triangulate_corr, warp_by_corr, warp_by_map,
                                warp_perspective)
from cotr_amd.inference.warp import invert_perspective, picture_corners
from tests import raster_oracle as ro
from tests import warp_oracle as wo

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (7, 13), (256, 512), (768, 1024)]
BIG = (3000, 4000)
# (source, destination): every size with itself, small source / large destination and the reverse
SIZE_PAIRS = [(s, s) for s in SMALL] + [((7, 13), (768, 1024)), ((768, 1024), (7, 13)), ((1, 1), (256, 512)), ((256, 512), (1, 1))]
BIG_PAIRS = [(BIG, BIG), ((7, 13), BIG), (BIG, (256, 512))]


def triangulated_map(Hd, Wd, Hs, Ws, seed):
    """a real triangulate_corr(as_tensor=True) output (float64, device): a jittered grid of correspondences over the middle
    of A, so that the map is 0 outside their hull"""
    verts, tris = ro.jittered_grid(9, 7, 0.4, seed, lo=0.15, hi=0.85)
    rng = np.random.default_rng(seed)
    pb = verts.astype(np.float64) * [0.8, 0.9] + 0.05 + rng.uniform(-0.01, 0.01, verts.shape)
    corr = np.hstack([verts.astype(np.float64) * [Wd, Hd], pb * [Ws, Hs]])
    return triangulate_corr(corr, (Hd, Wd), (Hs, Ws), simplices=tris, as_tensor=True)


def maps(Hd, Wd, Hs, Ws, dtype, seed):
    """name -> map [Hd, Wd, 2] (numpy, or a device tensor for the triangulate_corr output)"""
    rng = np.random.default_rng(seed)
    ident = wo.identity_map(Hd, Wd, dtype)
    out = {'identity': ident, 'integer shift': ident + dtype(3) * np.array([1, -2], dtype),
           'fractional shift': ident + np.array([0.37, -1.71], dtype),
           'smooth': wo.smooth_map(Hd, Wd, Hs, Ws, seed, dtype),
           'wholly outside': wo.smooth_map(Hd, Wd, Hs, Ws, seed + 1, dtype) + dtype(Ws + Hs + 5),
           'half outside': wo.smooth_map(Hd, Wd, Hs, Ws, seed + 2, dtype, margin=0.5),
           'k/64 ties': (rng.integers(-2 * 64, (Ws + 2) * 64, (Hd, Wd, 2)) // np.array([1, max(Ws // Hs, 1)]) / 64).astype(dtype)}
    bad = wo.smooth_map(Hd, Wd, Hs, Ws, seed + 3, dtype)
    r = rng.random((Hd, Wd))
    bad[r < 0.05] = np.nan
    bad[(r >= 0.05) & (r < 0.10), 0] = np.inf
    bad[(r >= 0.10) & (r < 0.15), 1] = -np.inf
    bad[(r >= 0.15) & (r < 0.20)] = dtype(1e30)
    bad[(r >= 0.20) & (r < 0.25), 0] = dtype(-2.0 ** 26)
    bad[(r >= 0.25) & (r < 0.30), 1] = dtype(2.0 ** 26 - 4)
    out['NaN, Inf and huge'] = bad
    if dtype == np.float64:
        out['triangulate_corr'] = triangulated_map(Hd, Wd, Hs, Ws, seed)
    return out


def check_map(img, m, bg, with_cover, what):
    m_np = m.cpu().numpy() if torch.is_tensor(m) else m
    want, want_cover = wo.remap(img, m_np, bg)
    got = warp_by_map(img, m, background=bg, return_cover=with_cover)
    got, cover = got if with_cover else (got, None)
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, int((got != want).sum()))
    if with_cover:
        assert cover.dtype == bool and np.array_equal(cover, want_cover), (what, int((cover != want_cover).sum()))
    return want_cover


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('src_size,dst_size', SIZE_PAIRS)
def test_warp_map_is_identical_to_the_restatement(src_size, dst_size, dtype, C):
    (Hs, Ws), (Hd, Wd) = src_size, dst_size
    img, bg = wo.image(Hs, Ws, C, 1), wo.image(Hd, Wd, C, 2)
    covers = {}
    for name, m in maps(Hd, Wd, Hs, Ws, dtype, seed=Hs + Wd + C).items():
        for background in (None, bg):
            for with_cover in (False, True):
                covers[name] = check_map(img, m, background, with_cover, (name, background is not None, with_cover))
    assert not covers['wholly outside'].any()
    if Hd * Wd >= 64:
        assert not covers['NaN, Inf and huge'].all()
        if min(Hs, Ws) >= 7:                                     # (a 1 x 1 source has no extent to be half outside of)
            assert covers['half outside'].any() and not covers['half outside'].all()
    if 'triangulate_corr' in covers and min(Hd, Wd) >= 7 and min(Hs, Ws) >= 7:
        assert covers['triangulate_corr'].all()                 # zeros outside the hull read img[0, 0]: covered


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('src_size,dst_size', BIG_PAIRS)
def test_warp_map_at_twelve_megapixels(src_size, dst_size, C):
    (Hs, Ws), (Hd, Wd) = src_size, dst_size
    img, bg = wo.image(Hs, Ws, C, 3), wo.image(Hd, Wd, C, 4)
    k = 0
    for dtype in (np.float32, np.float64):
        for name, m in maps(Hd, Wd, Hs, Ws, dtype, seed=C).items():
            if C != 3 and name not in ('smooth', 'half outside', 'NaN, Inf and huge', 'triangulate_corr'):
                continue                                         # every kind at C = 3; the gathering kinds at C = 1 and 4
            k += 1                                               # background and cover alternate, each pairing with each
            check_map(img, m, bg if k & 1 else None, bool(k & 2), (name, dtype.__name__))


def test_gray_image_without_channel_axis():
    img, bg = wo.image(100, 131, 1, 5)[..., 0], wo.image(77, 93, 1, 6)[..., 0]
    m = wo.smooth_map(77, 93, 100, 131, 1, margin=0.2)
    got, cover = warp_by_map(img, m, background=bg, return_cover=True)
    want, want_cover = wo.remap(img, m, bg)
    assert got.shape == (77, 93) and np.array_equal(got, want) and np.array_equal(cover, want_cover)


# ---- perspective -------------------------------------------------------------------------------------------------------------
def check_perspective(img, Minv, Hd, Wd, bg=None, what=''):
    want, want_cover = wo.warp_perspective(img, Minv, Hd, Wd, bg)
    got, cover = warp_perspective(img, Minv, (Wd, Hd), inverse_map=True, background=bg, return_cover=True)
    assert np.array_equal(got, want), (what, int((got != want).sum()))
    assert np.array_equal(cover, want_cover), (what, int((cover != want_cover).sum()))
    return got, cover


def rotation(Hs, Ws, deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    cx, cy = (Ws - 1) / 2, (Hs - 1) / 2
    return np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0, 0, 1]])


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('size', SMALL + [(1000, 1200)])
def test_warp_perspective_is_identical_to_the_restatement(size, C):
    Hs, Ws = size
    Hd, Wd = Hs + 3, Ws + 5
    img, bg = wo.image(Hs, Ws, C, 7), wo.image(Hd, Wd, C, 8)
    horizon = np.array([[1.0, 0.1, -3.0], [0.05, 1.2, 2.0], [1.0 / max(Wd, 2), 1.0 / max(Hd, 2), -1.0]])   # W = 0 crosses the canvas
    cases = {'identity': np.eye(3), 'integer translation': np.array([[1, 0, -4.0], [0, 1, 3.0], [0, 0, 1]]),
             'fractional translation': np.array([[1, 0, 0.37], [0, 1, -1.71], [0, 0, 1]]),
             'k/64 translation': np.array([[1, 0, 3 / 64], [0, 1, -5 / 64], [0, 0, 1]]),
             'rotation': rotation(Hs, Ws, 17.0), 'horizon': horizon,
             'perspective': invert_perspective(get_perspective_transform(picture_corners((Hs, Ws)), wo.demo_corners(Hd, Wd)))}
    for name, Minv in cases.items():
        got, cover = check_perspective(img, Minv, Hd, Wd, None, name)
        check_perspective(img, Minv, Hd, Wd, bg, name + ' + background')
        for scale in (2.0 ** -7, 2.0 ** 9):                      # a homogeneous power-of-two scale: the same bits
            g2, c2 = warp_perspective(img, Minv * scale, (Wd, Hd), inverse_map=True, return_cover=True)
            assert np.array_equal(g2, got) and np.array_equal(c2, cover), (name, scale)
    if min(size) >= 7:
        W = (horizon[2, 0] * np.arange(Wd)[None, :] + horizon[2, 1] * np.arange(Hd)[:, None]) + horizon[2, 2]
        assert (W > 0).any() and (W < 0).any()


def test_forward_matrix_is_inverted_on_the_host():
    img = wo.image(300, 400, 3, 9)
    M = get_perspective_transform(picture_corners(img.shape), wo.demo_corners(500, 600))
    got = warp_perspective(img, M, (600, 500))
    want, _ = wo.warp_perspective(img, np.linalg.inv(M), 500, 600)
    assert np.array_equal(got, want)


def test_paste_by_corners_is_the_demos_two_warps_and_composite():
    """demo_homography.py:46-49 at its own shape: a 1200 x 1000 picture into a 4000 x 3000 (H x W) photograph"""
    picture, img_b = wo.image(1200, 1000, 3, 10), wo.image(4000, 3000, 3, 11)
    corners = np.array([[932, 1025], [2469, 901], [908, 2927], [2436, 3080]], np.float64) + 0.3
    got = paste_by_corners(picture, corners, img_b)
    rep_coord = np.array([[0, 0], [1000, 0], [0, 1200], [1000, 1200]]).astype(np.float32)
    T = get_perspective_transform(rep_coord, corners.astype(np.float32))
    Tinv = np.linalg.inv(T)
    _, vmask = wo.warp_perspective(np.ones((1200, 1000), np.uint8), Tinv, 4000, 3000)      # warpPerspective(ones) > 0
    warped, cover = wo.warp_perspective(picture, Tinv, 4000, 3000)
    assert np.array_equal(vmask, cover) and 0.2 < cover.mean() < 0.5
    out = warped * vmask[..., None] + img_b * (~vmask[..., None])
    assert got.dtype == np.uint8 and np.array_equal(got, out)
    t = paste_by_corners(torch.from_numpy(picture).cuda(), corners, torch.from_numpy(img_b).cuda(), as_tensor=True)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), out)


# ---- warp_by_corr --------------------------------------------------------------------------------------------------------------
def test_warp_by_corr_is_the_demos_last_lines():
    Ha, Wa, Hb, Wb = 301, 457, 512, 333
    img_a, img_b = wo.image(Ha, Wa, 3, 12), wo.image(Hb, Wb, 3, 13)
    verts, tris = ro.jittered_grid(11, 9, 0.4, 5, lo=0.1, hi=0.9)
    pb = verts.astype(np.float64) * [0.7, 0.8] + 0.1
    corrs = np.hstack([verts.astype(np.float64) * [Wa, Ha], pb * [Wb, Hb]])
    overlay, warped = warp_by_corr(img_a, img_b, corrs, simplices=tris)
    dense, mask = triangulate_corr(corrs, img_a.shape, img_b.shape, simplices=tris, return_mask=True)
    assert dense.dtype == np.float64 and not mask.all()
    assert np.array_equal(warped, warp_by_map(img_b, dense))
    assert np.array_equal(warped, wo.remap(img_b, dense)[0])
    assert (warped[~mask] == img_b[0, 0]).all()                  # the zeros outside the hull read img_b at (0, 0), as in the demo
    demo = warped / 255 * 0.5 + img_a / 255 * 0.5                  # demo_single_pair.py:44, float64
    assert overlay.dtype == np.float32 and overlay.shape == (Ha, Wa, 3)
    assert (np.abs(overlay.astype(np.float64) - demo) <= np.spacing(demo.astype(np.float32)).astype(np.float64)).all()
    o2, w2 = warp_by_corr(torch.from_numpy(img_a).cuda(), torch.from_numpy(img_b).cuda(), corrs, alpha=0.25, as_tensor=True,
                          simplices=tris)
    assert o2.is_cuda and w2.is_cuda and np.array_equal(w2.cpu().numpy(), warped)
    demo = warped / 255 * 0.25 + img_a / 255 * 0.75
    assert (np.abs(o2.cpu().numpy().astype(np.float64) - demo) <= np.spacing(demo.astype(np.float32)).astype(np.float64)).all()


# ---- determinism, streams, graphs, inputs ----------------------------------------------------------------------------------------
def _device_case(C=3):
    Hs, Ws, Hd, Wd = 300, 401, 256, 509
    d = torch.device('cuda', 0)
    img = torch.from_numpy(wo.image(Hs, Ws, C, 14)).to(d)
    bg = torch.from_numpy(wo.image(Hd, Wd, C, 15)).to(d)
    m = torch.from_numpy(wo.smooth_map(Hd, Wd, Hs, Ws, 16, margin=0.3)).to(d)
    Minv = rotation(Hs, Ws, -23.0) @ np.diag([1.1, 0.9, 1.0])
    return img, bg, m, Minv, (Wd, Hd)


def _both(img, bg, m, Minv, dsize):
    a = warp_by_map(img, m, background=bg, return_cover=True, as_tensor=True)
    b = warp_perspective(img, Minv, dsize, inverse_map=True, background=bg, return_cover=True, as_tensor=True)
    return a + b


def test_run_to_run_side_stream_and_graph_replay_are_bit_identical():
    img, bg, m, Minv, dsize = _device_case()
    ref = _both(img, bg, m, Minv, dsize)
    torch.cuda.synchronize()
    want = wo.remap(img.cpu().numpy(), m.cpu().numpy(), bg.cpu().numpy())
    assert np.array_equal(ref[0].cpu().numpy(), want[0]) and np.array_equal(ref[1].cpu().numpy(), want[1])
    for _ in range(3):
        again = _both(img, bg, m, Minv, dsize)
        assert all(torch.equal(x, y) for x, y in zip(again, ref))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = _both(img, bg, m, Minv, dsize)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(s, ref))
    g = torch.cuda.CUDAGraph()                                    # one chain: the two launches follow each other on one stream
    with torch.cuda.graph(g):
        captured = _both(img, bg, m, Minv, dsize)
    for t in captured:
        t.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(captured, ref))
    m.copy_(torch.from_numpy(wo.smooth_map(256, 509, 300, 401, 17, margin=0.1)))   # a replay reads the buffers' current contents
    g.replay()
    torch.cuda.synchronize()
    fresh = _both(img, bg, m, Minv, dsize)
    assert all(torch.equal(x, y) for x, y in zip(captured, fresh))


@pytest.mark.parametrize('C', [1, 3, 4])
def test_numpy_and_device_inputs_give_the_same_bits(C):
    img, bg, m, Minv, dsize = _device_case(C)
    dev = _both(img, bg, m, Minv, dsize)
    host = (warp_by_map(img.cpu().numpy(), m.cpu().numpy(), background=bg.cpu().numpy(), return_cover=True) +
            warp_perspective(img.cpu().numpy(), Minv, dsize, inverse_map=True, background=bg.cpu().numpy(), return_cover=True))
    assert all(isinstance(h, np.ndarray) and np.array_equal(d.cpu().numpy(), h) for d, h in zip(dev, host))
    mixed = warp_by_map(img, m.cpu().numpy(), background=bg, as_tensor=True)
    assert torch.equal(mixed, dev[0])
    # views that are not contiguous, and a map whose address is not a multiple of 16
    wide = torch.zeros((300, 401 + 7, C), dtype=torch.uint8, device='cuda')
    wide[:, 3:404] = img
    assert torch.equal(warp_by_map(wide[:, 3:404], m, background=bg, as_tensor=True), dev[0])
    flat = torch.zeros(m.numel() + 2, dtype=torch.float32, device='cuda')
    flat[2:] = m.flatten()
    assert torch.equal(warp_by_map(img, flat[2:].view(m.shape), background=bg, as_tensor=True), dev[0])


def test_wrong_devices_and_dtypes_raise():
    img, bg, m, Minv, dsize = _device_case()
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        warp_by_map(img.cpu(), m)
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        warp_by_map(img, m, background=bg.cpu())
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        warp_perspective(img.cpu(), Minv, dsize)
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        paste_by_corners(img.cpu(), wo.demo_corners(256, 509), bg)
    with pytest.raises(ValueError, match='uint8'):
        warp_by_map(img.float(), m)
    with pytest.raises(ValueError, match='float32 or float64'):
        warp_by_map(img, m.half())
    with pytest.raises(ValueError, match='uint8'):
        warp_perspective(img.int(), Minv, dsize)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match='one device'):
            warp_by_map(img, m.to('cuda:1'))
