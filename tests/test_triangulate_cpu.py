"""triangulate_corr without a GPU: the coverage rule of the numpy restatement (tests/raster_oracle.py), the argument checks
of the C ABI (they run before any HIP call), and the host logic of cotr_amd.inference.triangulate_corr with the raster call
answered by the restatement."""
import ctypes
import sys

import numpy as np
import pytest
import torch

from tests import raster_oracle as ro


def _on_pixel_centres(pts, H, W):
    return ((np.floor(pts * [W, H]) + 0.5) / [W, H]).astype(np.float32)


# ---- the coverage rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,nx,ny,jitter,seed', [(64, 64, 8, 8, 0.0, 0), (48, 80, 5, 7, 0.4, 1), (37, 53, 9, 4, 0.45, 2),
                                                   (16, 16, 16, 16, 0.0, 3)])
def test_jittered_grid_covers_every_sample_exactly_once(H, W, nx, ny, jitter, seed):
    verts, tris = ro.jittered_grid(nx, ny, jitter, seed)
    _, mask, _, count = ro.raster(verts, np.zeros_like(verts), tris, H, W)
    assert (count == 1).all() and mask.all()


@pytest.mark.parametrize('n,centres,seed', [(300, False, 0), (300, True, 1), (60, True, 2)])
def test_delaunay_mesh_covers_the_inside_of_the_hull_exactly_once(n, centres, seed):
    spatial = pytest.importorskip('scipy.spatial')
    H, W = 96, 128
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0.05, 0.95, (n, 2))
    if centres:                      # vertices on pixel centres: edges through samples, fans around a sample
        pts = _on_pixel_centres(pts, H, W)
        pts = np.unique(pts, axis=0)
    pts = pts.astype(np.float32)
    tri = spatial.Delaunay(pts.astype(np.float64))
    _, mask, _, count = ro.raster(pts, np.zeros_like(pts), tri.simplices, H, W)
    assert count.max() == 1
    yy, xx = np.mgrid[0:H, 0:W]
    c = np.stack([(xx + 0.5) / W, (yy + 0.5) / H, np.ones((H, W))], -1)
    hull = spatial.ConvexHull(pts.astype(np.float64))
    eps = 1.0 / (256 * min(H, W))          # snapping moves a vertex by at most 1/512 px
    assert mask[(c @ hull.equations.T < -eps).all(-1)].all()
    assert not mask[(c @ hull.equations.T > eps).any(-1)].any()


def test_tie_rule_shared_edge():
    # the diagonal of a 4x4 canvas passes through the samples (i, i): owned by the triangle whose edge runs with dy < 0
    verts = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], np.float32)
    for tris in ([[0, 1, 3], [0, 3, 2]], [[3, 1, 0], [2, 3, 0]]):       # either winding
        _, mask, ids, count = ro.raster(verts, np.zeros_like(verts), tris, 4, 4)
        assert (count == 1).all()
        assert (np.diag(ids) == 0).all()          # (0,1,3) traverses the diagonal from (1,1) to (0,0): dy < 0 -> inside
    # one triangle alone: its closed side of the diagonal is the one the rule gives it
    _, mask, _, _ = ro.raster(verts, np.zeros_like(verts), [[0, 3, 2]], 4, 4)
    assert not np.diag(mask).any() and mask[np.tril_indices(4, -1)].all()


def test_tie_rule_fan_around_a_sample():
    # eight triangles around a vertex at the centre of pixel (2, 2) of a 5x5 canvas: that sample is covered exactly once
    c = np.array([2.5 / 5, 2.5 / 5])
    ring = np.array([[0, 0], [0.5, 0], [1, 0], [1, 0.5], [1, 1], [0.5, 1], [0, 1], [0, 0.5]])
    verts = np.vstack([c, ring]).astype(np.float32)
    tris = [[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)]
    _, _, _, count = ro.raster(verts, np.zeros_like(verts), tris, 5, 5)
    assert (count == 1).all()


def test_tie_rule_hull_edges():
    # right triangle whose hypotenuse passes through the samples with i + j == 3 on a 4x4 canvas, both windings
    verts = np.array([[0, 0], [1, 0], [0, 1]], np.float32)
    for tris in ([[0, 1, 2]], [[0, 2, 1]]):
        _, mask, _, _ = ro.raster(verts, np.zeros_like(verts), tris, 4, 4)
        i, j = np.mgrid[0:4, 0:4]
        assert mask[i + j < 3].all() and not mask[i + j > 3].any()
        # the hypotenuse runs b=(1,0) -> c=(0,1) after orientation (dy > 0): excluded
        assert not mask[i + j == 3].any()
    # the mirrored triangle owns those samples: (1,0) (1,1) (0,1)
    _, mask, _, _ = ro.raster(np.array([[1, 0], [1, 1], [0, 1]], np.float32), np.zeros((3, 2)), [[0, 1, 2]], 4, 4)
    i, j = np.mgrid[0:4, 0:4]
    assert mask[i + j == 3].all()


def test_overlap_highest_index_wins_and_bad_triangles_cover_nothing():
    verts = np.array([[0, 0], [1, 0], [0, 1], [1, 1], [np.nan, 0.5], [0.2, 0.2]], np.float32)
    attrs = np.arange(12, dtype=np.float32).reshape(6, 2)
    tris = [[0, 1, 2], [0, 1, 3], [0, 4, 3], [0, 9, 3], [0, 5, 3]]      # 2: NaN vertex, 3: bad index, 4: zero area
    _, mask, ids, count = ro.raster(verts, attrs, tris, 8, 8)
    assert set(np.unique(ids[mask])) == {0, 1}
    both = (count == 2)
    assert both.any() and (ids[both] == 1).all()


def test_affine_attributes_are_reproduced():
    H, W = 40, 56
    rng = np.random.default_rng(5)
    px = rng.integers(-2000, 256 * 60, (30, 2)) / 256.0                 # on the 1/256 px grid: snapping moves nothing
    verts = (px / [W, H]).astype(np.float32)
    X, Y, _ = ro.snap(verts, H, W)
    assert np.array_equal(np.stack([X, Y], -1), px * 256)
    A = np.array([[0.75, -0.25], [0.125, 1.5]])
    attrs = (px @ A.T + [3.0, -1.0]).astype(np.float32)
    verts_g, tris = ro.jittered_grid(6, 5, 0.3, 7, lo=-0.1, hi=1.1)
    pxg = np.rint(verts_g.astype(np.float64) * [W, H] * 256) / 256
    verts_g = (pxg / [W, H]).astype(np.float32)
    cases = [(verts_g, (pxg @ A.T + [3.0, -1.0]).astype(np.float32), tris)]
    if _have_scipy():
        from scipy.spatial import Delaunay
        cases.append((verts, attrs, Delaunay(px).simplices))
    for v, a, t in cases:
        out, mask, _, _ = ro.raster(v, a, t, H, W)
        yy, xx = np.mgrid[0:H, 0:W]
        want = np.stack([xx + 0.5, yy + 0.5], -1) @ A.T + [3.0, -1.0]
        assert mask.any()
        err = np.abs(out - want)[mask].max()
        assert err < 1e-5, err       # float32 attributes at the vertices; the interpolation itself is exact


def _have_scipy():
    try:
        import scipy.spatial  # noqa: F401
        return True
    except ImportError:
        return False


# ---- the C ABI's argument checks (before any HIP call) ---------------------------------------------------------------
def test_abi_argument_errors_without_a_gpu():
    from cotr_amd import _lib
    from cotr_amd.build import build_library
    build_library()
    lib = _lib.load_library()
    nb = ctypes.c_size_t()
    P = ctypes.c_void_p(4096)                # never dereferenced: every case fails its host-side check
    assert lib.cotr_raster_mesh_scratch_bytes(10, 64, 64, ctypes.byref(nb)) == 0 and nb.value >= 64 * 64 * 4 + 10 * 64
    need = nb.value

    def call(verts=P, attrs=P, tris=P, n_tris=10, H=64, W=64, out=P, scratch=P, nbytes=need):
        return lib.cotr_raster_mesh(verts, 5, attrs, tris, n_tris, H, W, out, None, scratch, nbytes, None)

    cases = {'null verts': dict(verts=None), 'null attrs': dict(attrs=None), 'null tris': dict(tris=None),
             'null out': dict(out=None), 'null scratch': dict(scratch=None), 'H = 0': dict(H=0), 'W = 16385': dict(W=16385),
             'n_tris < 0': dict(n_tris=-1), 'too little scratch': dict(nbytes=need - 1)}
    for what, kw in cases.items():
        assert call(**kw) == -1, what
        assert lib.cotr_raster_last_error(), what
    assert b'scratch' in (call(nbytes=need - 1), lib.cotr_raster_last_error())[1]
    assert b'16384' in (call(W=16385), lib.cotr_raster_last_error())[1]
    assert lib.cotr_raster_mesh_scratch_bytes(1, 0, 5, ctypes.byref(nb)) == -1
    assert lib.cotr_raster_mesh_scratch_bytes(1, 5, 16385, ctypes.byref(nb)) == -1
    assert lib.cotr_raster_mesh_scratch_bytes(-1, 5, 5, ctypes.byref(nb)) == -1
    assert lib.cotr_raster_mesh_scratch_bytes(1, 5, 5, None) == -1
    # the scratch grows with the canvas and the triangle count
    sizes = []
    for args in ((0, 1, 1), (1000, 1, 1), (0, 1024, 768), (1000, 1024, 768)):
        assert lib.cotr_raster_mesh_scratch_bytes(*args, ctypes.byref(nb)) == 0
        sizes.append(nb.value)
    assert sizes[0] < sizes[1] < sizes[3] and sizes[2] < sizes[3]


# ---- host logic of triangulate_corr, the raster call answered by the restatement ---------------------------------------
@pytest.fixture
def oracle_raster(monkeypatch):
    from cotr_amd.inference import triangulate as tr
    calls = []

    def fake(verts, attrs, tris, H, W, device=None):
        calls.append((np.asarray(verts), np.asarray(attrs), np.asarray(tris), H, W))
        out, mask, _, _ = ro.raster(verts, attrs, tris, H, W)
        return torch.from_numpy(out.astype(np.float32)), torch.from_numpy(mask)
    monkeypatch.setattr(tr, 'raster_mesh', fake)
    return calls


def _corrs(n, shape_a, shape_b, seed):
    rng = np.random.default_rng(seed)
    (ha, wa), (hb, wb) = shape_a, shape_b
    pa = rng.uniform(0, 1, (n, 2)) * [wa, ha]
    pb = pa * [wb / wa, hb / ha] * 0.9 + rng.uniform(-3, 3, (n, 2))
    return np.hstack([pa, pb])


def test_triangulate_corr_output_and_normalised_triangulation(oracle_raster):
    spatial = pytest.importorskip('scipy.spatial')
    from cotr_amd.inference import triangulate_corr
    shape_a, shape_b = (96, 160, 3), (120, 90, 3)
    corr = _corrs(60, shape_a[:2], shape_b[:2], 0)
    render = triangulate_corr(corr, shape_a, shape_b)
    assert render.dtype == np.float64 and render.shape == (96, 160, 2)
    verts, attrs, tris, H, W = oracle_raster[0]
    assert (H, W) == (96, 160) and verts.dtype == np.float32
    norm = corr / [160, 96, 90, 120]
    assert np.array_equal(verts, norm[:, :2].astype(np.float32)) and np.array_equal(attrs, norm[:, 2:].astype(np.float32))
    t_norm = spatial.Delaunay(norm[:, :2]).simplices
    t_px = spatial.Delaunay(corr[:, :2]).simplices
    assert {tuple(sorted(t)) for t in t_norm} != {tuple(sorted(t)) for t in t_px}   # the case tells the two apart
    assert np.array_equal(tris, t_norm)
    out, mask, _, _ = ro.raster(norm[:, :2].astype(np.float32), norm[:, 2:].astype(np.float32), t_norm, 96, 160)
    assert np.array_equal(render, out.astype(np.float32) * np.array([90, 120]))
    assert (render[~mask] == 0).all() and mask.any() and not mask.all()
    render2, mask2 = triangulate_corr(corr, shape_a, shape_b, return_mask=True)
    assert np.array_equal(render2, render) and mask2.dtype == bool and np.array_equal(mask2, mask)


def test_triangulate_corr_simplices_skip_scipy_and_errors(oracle_raster, monkeypatch):
    from cotr_amd.inference import triangulate_corr
    corr = np.array([[0, 0, 0, 0], [40, 0, 20, 0], [0, 30, 0, 60], [40, 30, 20, 60]], np.float64)
    monkeypatch.setitem(sys.modules, 'scipy.spatial', None)          # scipy unavailable
    with pytest.raises(ImportError, match='scipy'):
        triangulate_corr(corr, (30, 40), (60, 20))
    render = triangulate_corr(corr, (30, 40), (60, 20), simplices=[[0, 1, 3], [0, 3, 2]])
    assert render.shape == (30, 40, 2) and render.dtype == np.float64
    yy, xx = np.mgrid[0:30, 0:40]
    assert np.allclose(render, np.stack([(xx + 0.5) / 2, (yy + 0.5) * 2], -1), atol=1e-4)
    for bad in ([[0, 1, 4]], [[-1, 1, 2]], [[0, 1]], [[0.0, 1.0, 2.0]]):
        with pytest.raises(ValueError):
            triangulate_corr(corr, (30, 40), (60, 20), simplices=bad)
    with pytest.raises(ValueError):
        triangulate_corr(corr[:, :3], (30, 40), (60, 20), simplices=[[0, 1, 2]])
    monkeypatch.delitem(sys.modules, 'scipy.spatial')
    spatial = pytest.importorskip('scipy.spatial')
    for pts in (corr[:2], np.array([[0, 0, 0, 0], [10, 10, 1, 1], [20, 20, 2, 2]], np.float64)):   # too few, collinear
        with pytest.raises(spatial.QhullError):
            triangulate_corr(pts, (30, 40), (60, 20))
