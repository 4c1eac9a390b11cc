"""cotr_delaunay / delaunay / triangulate_corr(simplices='device') on the MI355X against the rule's restatement
(tests/delaunay_oracle.py): the device triangles and the restatement's are the same ORDERED list in every case here
(only the comparisons with scipy are comparisons of sets), info[1] == 0 and every row past the count is -1."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import delaunay, triangulate_corr, warp_by_corr
from tests import delaunay_oracle as do
from tests.test_delaunay_cpu import large_lattice, lattice_with_duplicates, pixel_grid, two_rows_and_a_point

pytestmark = pytest.mark.gpu


def device_tris(P):
    """-> the triangles before the count, after checking the status and the rows past the count"""
    P = np.asarray(P, dtype=np.float32).reshape(-1, 2)
    tris, info = delaunay(P, as_tensor=True)
    torch.cuda.synchronize()
    tris, (count, status) = tris.cpu().numpy(), info.cpu().numpy()
    assert tris.shape == (2 * len(P), 3) and tris.dtype == np.int32
    assert status == 0
    assert 0 <= count <= len(tris) and (tris[count:] == -1).all()
    assert np.array_equal(delaunay(P), tris[:count])            # the host-array form reads the count back
    return tris[:count]


def check(P, form='int'):
    got = device_tris(P)
    want, status = do.triangulate(P, form)
    assert status == 0
    assert got.shape == want.shape and np.array_equal(got, want), f'{len(got)} device triangles, {len(want)} by the rule'
    return got


def f24(X):
    """integers below 2^24 -> the float32 points that snap onto exactly them"""
    X = np.asarray(X, dtype=np.int64)
    assert (np.abs(X) < 1 << 24).all()
    return (X / float(1 << 24)).astype(np.float32)


# ---- trivial sizes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,T', [(np.zeros((0, 2)), 0), ([[0.3, 0.4]], 0), ([[0.3, 0.4], [0.5, 0.1]], 0),
                                 ([[0.125, 0.125], [0.375, 0.25], [0.625, 0.375]], 0), ([[0.1, 0.1], [0.7, 0.2], [0.4, 0.9]], 1),
                                 (np.stack([np.arange(7) / 8, np.arange(7) / 16], -1), 0)],
                         ids=['n = 0', 'n = 1', 'n = 2', '3 collinear', '3 general', '7 collinear'])
def test_trivial_sizes(P, T):
    assert len(check(P)) == T


# ---- a cocircular quadruple ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', list(itertools.permutations(range(4))), ids=lambda o: ''.join(map(str, o)))
def test_square_corners_in_every_index_order(order):
    corners = np.array([[0.25, 0.25], [0.75, 0.25], [0.75, 0.75], [0.25, 0.75]], np.float32)
    got = check(corners[list(order)])
    assert len(got) == 2
    # the lowest index is lifted most, so the lower hull avoids it where it can: the diagonal is the one WITHOUT corner
    # order.index(...) == 0, i.e. point 0 has one triangle only
    assert (got == 0).sum() == 1


# ---- lane and wavefront edges; a point that keeps more triangles than the staging holds -------------------------------------
@pytest.mark.parametrize('n', [63, 64, 65, 129, 256, 257, 513])   # 256: the width of the scan's chunks
def test_random_points_around_the_wavefront_width(n):
    check(np.random.default_rng(n).uniform(0, 1, (n, 2)).astype(np.float32))


def test_a_hub_keeps_more_triangles_than_the_staging_holds():
    rng = np.random.default_rng(3)
    ang = (np.arange(40) + rng.uniform(-0.1, 0.1, 40)) * (2 * np.pi / 40)
    ring = 0.5 + (0.3 + rng.uniform(-0.002, 0.002, 40))[:, None] * np.stack([np.cos(ang), np.sin(ang)], -1)
    got = check(np.vstack([[[0.5, 0.5]], ring]).astype(np.float32))
    assert (got[:, 0] == 0).sum() == 40                         # (the write pass walks again for such a point)


# ---- exactness: full 24-bit coordinates -----------------------------------------------------------------------------------
def _exact_cases():
    rng = np.random.default_rng(11)
    k, c = 1000003, 8100000                                     # octagon (+-3k, +-4k), (+-4k, +-3k) about (c, c): radius 5k
    octagon = np.array([(3, 4), (4, 3), (4, -3), (3, -4), (-3, -4), (-4, -3), (-4, 3), (-3, 4)]) * k + c
    rects = np.array([[x, y] for x0, x1, y0, y1 in [(1234567, 15999999, 2345671, 14888883), (5000001, 11000003, 100003, 16000001)]
                      for x, y in [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]])
    filler = rng.integers(0, 1 << 24, (60, 2))
    near = octagon.copy()
    near[::2, 0] += 1                                           # one grid step off the circle
    near[1::2, 1] -= 1
    cases = {'octagon and rectangles': np.vstack([octagon[rng.permutation(8)], rects, filler]),
             'octagon alone': octagon, 'rectangles alone': rects[rng.permutation(8)],
             'one step off the circle': np.vstack([near, filler[:30]]),
             'octagon, centre and near points': np.vstack([filler[:20], octagon, [[c, c]], near[:3] + [[0, 2]] * 3]),
             'random 24-bit': rng.integers(0, 1 << 24, (128, 2))}
    return {name: f24(X) for name, X in cases.items()}


@pytest.mark.parametrize('name', list(_exact_cases()))
def test_full_24_bit_coordinates_need_the_128_bit_determinant(name):
    P = _exact_cases()[name]
    assert len(P) <= 128
    got = check(P)
    do.properties(P, got)
    if name in ('octagon alone', 'rectangles alone'):           # the determinant is 0 only in exact arithmetic
        assert not do.is_unique(P, got)


# ---- pixel grids ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [pixel_grid(16, 12, 640, 480), pixel_grid(9, 7, 37, 53), lattice_with_duplicates(),
                               two_rows_and_a_point()],
                         ids=['16x12 on 640x480', '9x7 on 37x53', '12x12 lattice with duplicates', 'two rows and a point'])
def test_pixel_grids(P):
    check(P)


# ---- invalid points -----------------------------------------------------------------------------------------------------------
def test_invalid_points_take_no_part():
    P = np.random.default_rng(1).uniform(0, 1, (100, 2)).astype(np.float32)
    P[3], P[9], P[17], P[64], P[70] = (np.nan, 0.5), (0.5, np.inf), (4.5, 0.5), (-np.inf, np.nan), (0.5, -4.01)
    P[20], P[30], P[99], P[65] = P[2], P[35], P[0], P[63]       # repeats at a higher (20, 99, 65) and at a lower index (30 before 35)
    invalid = {3, 9, 17, 64, 70, 20, 35, 99, 65}
    assert {i for i, s in enumerate(do.snap(P)) if s is None} == invalid
    got = check(P)
    assert not set(got.ravel()) & invalid
    assert set(got.ravel()) == set(range(100)) - invalid


# ---- larger inputs on the k/4096 lattice ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _large_reference(n):
    return do.triangulate(large_lattice(n), 'int64')


@pytest.mark.parametrize('n', [1000, 4096])
def test_large_lattice_inputs(n):
    P = large_lattice(n)
    want, status = _large_reference(n)
    got = device_tris(P)
    assert status == 0 and np.array_equal(got, want)
    if n == 1000:
        assert do.is_unique(P, want)                            # (tests/test_delaunay_cpu.py checks the seed)
    if do.is_unique(P, want):
        spatial = pytest.importorskip('scipy.spatial')
        assert do.as_set(got) == do.as_set(spatial.Delaunay(P.astype(np.float64)).simplices)      # a comparison of sets


# ---- determinism ------------------------------------------------------------------------------------------------------------
def _abi_call(verts, tris, info, scratch, nbytes=None, n=None, stream=None):
    lib = _lib.load_library()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    return lib.cotr_delaunay(p(verts), verts.shape[0] if n is None else n, p(tris), p(info), p(scratch),
                             scratch.numel() if nbytes is None else nbytes, stream if stream is not None else _lib.current_stream_ptr())


def _bytes(n):
    nb = ctypes.c_size_t()
    assert _lib.load_library().cotr_delaunay_scratch_bytes(n, ctypes.byref(nb)) == 0
    return nb.value


def _mixed_points(n, seed):
    rng = np.random.default_rng(seed)
    P = np.vstack([rng.uniform(0, 1, (n - 100, 2)), rng.integers(0, 10, (100, 2)) / 10]).astype(np.float32)   # ties and repeats
    return torch.from_numpy(P[rng.permutation(n)]).cuda()


def test_determinism_and_scratch_independence():
    v = _mixed_points(700, 1)
    nb = _bytes(700)
    results = []
    for fill in (0, 255, 17, 0):
        scratch = torch.full((nb + 512,), fill, dtype=torch.uint8, device='cuda')[256:256 + nb]
        tris = torch.full((1400, 3), 9, dtype=torch.int32, device='cuda')
        info = torch.full((2,), 9, dtype=torch.int32, device='cuda')
        assert _abi_call(v, tris, info, scratch) == 0
        torch.cuda.synchronize()
        results.append((tris.cpu().numpy().tobytes(), info.cpu().numpy().tobytes()))
    assert all(r == results[0] for r in results)
    count, status = np.frombuffer(results[0][1], np.int32)
    want, _ = do.triangulate(v.cpu().numpy())
    assert status == 0 and np.array_equal(np.frombuffer(results[0][0], np.int32).reshape(-1, 3)[:count], want)


def test_side_stream_and_graph_replay_match_the_default_stream():
    v = _mixed_points(500, 2)
    ref_tris, ref_info = delaunay(v, as_tensor=True)
    torch.cuda.synchronize()
    assert ref_info.tolist()[0] > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s_tris, s_info = delaunay(v, as_tensor=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(s_tris, ref_tris) and torch.equal(s_info, ref_info)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_tris, g_info = delaunay(v, as_tensor=True)
    for _ in range(2):
        g_tris.fill_(7), g_info.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_tris, ref_tris) and torch.equal(g_info, ref_info)
    v.copy_(_mixed_points(500, 3))                              # replays read the captured buffer's current contents
    g.replay()
    e_tris, e_info = delaunay(v, as_tensor=True)
    torch.cuda.synchronize()
    assert torch.equal(g_tris, e_tris) and torch.equal(g_info, e_info) and not torch.equal(g_tris, ref_tris)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refused_calls_launch_nothing():
    lib = _lib.load_library()
    v = _mixed_points(200, 4)
    nb = _bytes(200)
    scratch = torch.zeros(nb, dtype=torch.uint8, device='cuda')
    tris = torch.full((400, 3), 9, dtype=torch.int32, device='cuda')
    info = torch.full((2,), 9, dtype=torch.int32, device='cuda')
    for what, kw in {'n = -1': dict(n=-1), 'n = 65537': dict(n=65537), 'scratch one byte short': dict(nbytes=nb - 1)}.items():
        assert _abi_call(v, tris, info, scratch, **kw) == -1, what
        assert lib.cotr_raster_last_error(), what
    for what, args in {'null verts': (None, tris, info, scratch), 'null tris': (v, None, info, scratch),
                       'null info': (v, tris, None, scratch), 'null scratch': (v, tris, info, None)}.items():
        assert _abi_call(*args, nbytes=nb, n=200) == -1, what
        assert lib.cotr_raster_last_error(), what
    torch.cuda.synchronize()
    assert (tris == 9).all() and (info == 9).all() and (scratch == 0).all()
    with pytest.raises(ValueError):
        delaunay(torch.zeros((5, 3), device='cuda'))


# ---- the chain --------------------------------------------------------------------------------------------------------------
def _affine_corrs(n, shape_a, shape_b, seed):
    rng = np.random.default_rng(seed)
    pa = rng.uniform(0, 1, (n, 2)) * [shape_a[1], shape_a[0]]
    A = np.array([[1.1, 0.15], [-0.2, 1.3]])
    return np.hstack([pa, pa @ A.T + [3.0, 7.0]])


@pytest.mark.parametrize('n', [50, 500])
def test_triangulate_corr_on_the_device_equals_the_scipy_path(n):
    pytest.importorskip('scipy.spatial')
    shape_a, shape_b = (48, 64, 3), (96, 80, 3)
    corr = _affine_corrs(n, shape_a, shape_b, n)
    ref, ref_mask = triangulate_corr(corr, shape_a, shape_b, return_mask=True)
    out, mask = triangulate_corr(corr, shape_a, shape_b, simplices='device', return_mask=True)
    assert out.dtype == np.float64 and out.shape == (48, 64, 2) and mask.dtype == bool and mask.any()
    assert np.array_equal(mask, ref_mask)
    assert (out[~mask] == 0).all()
    assert np.abs(out - ref).max() <= 1e-3
    t_out, t_mask = triangulate_corr(torch.from_numpy(corr).cuda(), shape_a, shape_b, simplices='device', return_mask=True,
                                     as_tensor=True)
    assert t_out.is_cuda and t_out.dtype == torch.float64
    assert np.array_equal(t_out.cpu().numpy(), out) and np.array_equal(t_mask.cpu().numpy(), mask)


def test_warp_by_corr_on_the_device_under_graph_capture():
    rng = np.random.default_rng(5)
    shape_a, shape_b = (48, 64, 3), (96, 80, 3)
    img_a = torch.from_numpy(rng.integers(0, 256, shape_a, dtype=np.uint8)).cuda()
    img_b = torch.from_numpy(rng.integers(0, 256, shape_b, dtype=np.uint8)).cuda()
    corr = torch.from_numpy(_affine_corrs(300, shape_a, shape_b, 9)).cuda()
    e_overlay, e_warped = warp_by_corr(img_a, img_b, corr, as_tensor=True, simplices='device')
    torch.cuda.synchronize()
    assert e_warped.shape == shape_a and e_warped.float().std() > 10     # the warp shows image B, not a constant
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_overlay, g_warped = warp_by_corr(img_a, img_b, corr, as_tensor=True, simplices='device')
    for _ in range(2):
        g_overlay.fill_(7.0), g_warped.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_warped, e_warped) and torch.equal(g_overlay, e_overlay)
