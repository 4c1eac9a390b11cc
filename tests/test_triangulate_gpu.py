"""cotr_raster_mesh / triangulate_corr on the MI355X against the numpy restatement (tests/raster_oracle.py): coverage and mask
identical, values within 1e-3 px in B's pixels, on canvases that are and are not multiples of the 16x16 tile."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import triangulate_corr
from cotr_amd.inference.triangulate import raster_mesh
from tests import raster_oracle as ro

pytestmark = pytest.mark.gpu

B_PX = np.array([2048.0, 2048.0])     # attributes are normalised B coordinates: errors are reported in pixels of a 2048^2 B


def gpu_raster(verts, attrs, tris, H, W):
    out, mask = raster_mesh(verts, attrs, tris, H, W)
    torch.cuda.synchronize()
    return out.cpu().numpy(), mask.cpu().numpy()


def check(verts, attrs, tris, H, W, scale=B_PX):
    out, mask = gpu_raster(verts, attrs, tris, H, W)
    ref, ref_mask, _, _ = ro.raster(verts, attrs, tris, H, W)
    assert np.array_equal(mask, ref_mask), f'{int((mask != ref_mask).sum())} samples differ in coverage'
    assert (out[~mask] == 0).all()
    err = np.abs(out.astype(np.float64) - ref)[mask] * scale if mask.any() else np.zeros(1)
    assert err.max() <= 1e-3, err.max()
    return out, mask


def grid_attrs(verts, seed):
    rng = np.random.default_rng(seed)
    return (verts * [0.8, 0.9] + 0.05 + rng.uniform(-0.01, 0.01, verts.shape)).astype(np.float32)


CANVASES = [(1, 1), (7, 13), (256, 512), (768, 1024), (2048, 2048)]


@pytest.mark.parametrize('H,W', CANVASES)
@pytest.mark.parametrize('nx,ny,jitter', [(1, 1, 0.0), (9, 7, 0.4), (64, 48, 0.45)])
def test_jittered_grid(H, W, nx, ny, jitter):
    verts, tris = ro.jittered_grid(nx, ny, jitter, seed=H + W + nx)
    out, mask = check(verts, grid_attrs(verts, nx), tris, H, W)
    assert mask.all()                                       # the grid covers [0,1]^2: every sample exactly once


@pytest.mark.parametrize('H,W', CANVASES)
def test_vertices_on_pixel_centres(H, W):
    # a grid whose vertices sit on pixel centres: edges and vertices pass through samples
    nx, ny = min(W, 12), min(H, 9)
    xs = (np.round(np.linspace(0, W - 1, nx + 1)) + 0.5) / W
    ys = (np.round(np.linspace(0, H - 1, ny + 1)) + 0.5) / H
    if len(np.unique(xs)) < nx + 1 or len(np.unique(ys)) < ny + 1:
        xs, ys = np.linspace(0.05, 0.95, nx + 1), np.linspace(0.05, 0.95, ny + 1)
    verts, tris = ro.jittered_grid(nx, ny, 0.0, 0)
    gx, gy = np.meshgrid(xs, ys)
    verts = np.stack([gx, gy], -1).reshape(-1, 2).astype(np.float32)
    check(verts, grid_attrs(verts, 1), tris, H, W)


@pytest.mark.parametrize('H,W', CANVASES)
def test_one_triangle_larger_than_the_canvas(H, W):
    verts = np.array([[-1.5, -1.2], [3.3, -0.7], [-0.4, 3.9]], np.float32)
    attrs = np.array([[0.1, 0.2], [0.9, 0.3], [0.4, 0.95]], np.float32)
    out, mask = check(verts, attrs, [[0, 1, 2]], H, W)
    assert mask.all()


@pytest.mark.parametrize('H,W', CANVASES)
def test_slivers_spanning_the_canvas(H, W):
    rng = np.random.default_rng(H * W)
    verts, tris = [], []
    for k in range(40):           # long thin triangles corner to corner, across and down
        a = rng.uniform(-0.1, 0.1, 2) + ([0, 0] if k % 3 == 0 else [0, rng.uniform(0, 1)] if k % 3 == 1 else [rng.uniform(0, 1), 0])
        b = rng.uniform(0.9, 1.1, 2) if k % 3 == 0 else np.array([1.05, a[1] + rng.uniform(-0.05, 0.05)]) if k % 3 == 1 else \
            np.array([a[0] + rng.uniform(-0.05, 0.05), 1.05])
        c = b + rng.uniform(-3, 3, 2) / [W, H]
        verts += [a, b, c]
        tris.append([3 * k, 3 * k + 1, 3 * k + 2])
    verts = np.array(verts, np.float32)
    check(verts, rng.uniform(0, 1, verts.shape).astype(np.float32), tris, H, W)


@pytest.mark.parametrize('H,W', [(7, 13), (256, 512), (768, 1024)])
@pytest.mark.parametrize('lo,hi', [(-0.5, 1.5), (-2.0, 0.3), (1.2, 2.5), (-3.0, -1.0)])
def test_vertices_partly_or_wholly_outside(H, W, lo, hi):
    verts, tris = ro.jittered_grid(17, 13, 0.4, seed=3, lo=lo, hi=hi)
    out, mask = check(verts, grid_attrs(verts, 2), tris, H, W)
    if hi < 0 or lo > 1:
        assert not mask.any()


def test_ten_thousand_points_grid_and_delaunay():
    verts, tris = ro.jittered_grid(99, 100, 0.45, seed=11)
    assert len(verts) >= 10000
    check(verts, grid_attrs(verts, 3), tris, 2048, 2048)
    spatial = pytest.importorskip('scipy.spatial')
    rng = np.random.default_rng(12)
    pts = rng.uniform(0, 1, (10000, 2))
    tri = spatial.Delaunay(pts)
    v = pts.astype(np.float32)
    check(v, grid_attrs(v, 4), tri.simplices, 2048, 2048)
    check(v, grid_attrs(v, 4), tri.simplices, 768, 1024)


def test_more_block_totals_than_the_scan_takes_in_one_chunk():
    # a workgroup of the setup pass holds 256 triangles and the scan of their totals walks chunks of 256: one chunk plus three
    verts, tris = ro.jittered_grid(182, 182, 0.45, seed=14)
    assert len(tris) == 66248 and (len(tris) + 255) // 256 > 256
    out, mask = check(verts, grid_attrs(verts, 5), tris, 256, 512)
    assert mask.all()


@pytest.mark.parametrize('H,W', [(7, 13), (768, 1024)])
def test_scipy_meshes_with_vertices_on_pixel_centres(H, W):
    spatial = pytest.importorskip('scipy.spatial')
    rng = np.random.default_rng(W)
    pts = np.unique(((np.floor(rng.uniform(0, 1, (min(H * W // 2, 3000), 2)) * [W, H]) + 0.5) / [W, H]), axis=0)
    pts = np.vstack([pts, [[0, 0], [1, 0], [0, 1], [1, 1]]]).astype(np.float32)
    tri = spatial.Delaunay(pts.astype(np.float64))
    check(pts, grid_attrs(pts, 5), tri.simplices, H, W)


@pytest.mark.parametrize('H,W', [(7, 13), (256, 512), (2048, 2048)])
def test_affine_attributes_are_reproduced(H, W):
    rng = np.random.default_rng(W + 1)
    verts_g, tris = ro.jittered_grid(23, 19, 0.4, seed=6, lo=-0.05, hi=1.05)
    px = np.rint(verts_g.astype(np.float64) * [W, H] * 256) / 256          # on the snapping grid
    verts = (px / [W, H]).astype(np.float32)
    A = np.array([[0.75, -0.25], [0.125, 0.5]]) / max(H, W)
    attrs = (px @ A.T + [0.25, 0.125]).astype(np.float32)
    out, mask = gpu_raster(verts, attrs, tris, H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    want = np.stack([xx + 0.5, yy + 0.5], -1) @ A.T + [0.25, 0.125]
    assert mask.all()
    assert (np.abs(out - want) * B_PX).max() <= 1e-3


def test_overlap_highest_index_wins():
    rng = np.random.default_rng(8)
    H, W, T = 256, 512, 300
    verts = rng.uniform(-0.2, 1.2, (3 * T, 2)).astype(np.float32)
    attrs = np.repeat(np.arange(T, dtype=np.float32), 3)[:, None].repeat(2, 1) / 1024   # constant per triangle: its index
    tris = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    out, mask = check(verts, attrs, tris, H, W)
    _, _, ids, count = ro.raster(verts, attrs, tris, H, W)
    assert count.max() > 5
    assert np.array_equal(np.rint(out[..., 0] * 1024).astype(np.int64)[mask], ids[mask])


def test_bad_triangles_are_skipped():
    H, W = 256, 512
    verts, tris = ro.jittered_grid(13, 11, 0.4, seed=9)
    attrs = grid_attrs(verts, 6)
    good, good_mask = gpu_raster(verts, attrs, tris, H, W)
    n = len(verts)
    extra_v = np.array([[np.nan, 0.5], [0.5, np.inf], [0.1, 0.1], [0.1, 0.1], [0.9, 0.9], [20000.0, 0.5], [0.2, 0.7]], np.float32)
    v2 = np.vstack([verts, extra_v])
    a2 = np.vstack([attrs, np.full((7, 2), 7.0, np.float32)])
    bad = np.array([[0, n, 1], [0, 1, n + 1], [n + 2, n + 3, n + 4],       # NaN, inf, zero area
                    [0, 1, n + 7], [-1, 2, 3], [n + 100000, 1, 2],        # indices out of range
                    [0, n + 5, n + 6]], np.int32)                          # beyond 2^22 px
    for where in ('first', 'middle', 'last'):
        t2 = {'first': np.vstack([bad, tris]), 'last': np.vstack([tris, bad]),
              'middle': np.vstack([tris[:50], bad, tris[50:]])}[where]
        out, mask = check(v2, a2, t2, H, W)
        assert np.array_equal(mask, good_mask) and np.array_equal(out, good), where


def test_empty_mesh_writes_zeros():
    out, mask = gpu_raster(np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros((0, 3), np.int32), 37, 53)
    assert not mask.any() and (out == 0).all()


def _abi_call(verts, attrs, tris, H, W, scratch, out, mask, stream=None):
    lib = _lib.load_library()
    rc = lib.cotr_raster_mesh(ctypes.c_void_p(verts.data_ptr()), verts.shape[0], ctypes.c_void_p(attrs.data_ptr()),
                              ctypes.c_void_p(tris.data_ptr()), tris.shape[0], H, W, ctypes.c_void_p(out.data_ptr()),
                              ctypes.c_void_p(mask.data_ptr()), ctypes.c_void_p(scratch.data_ptr()), scratch.numel(),
                              stream if stream is not None else _lib.current_stream_ptr())
    assert rc == 0, lib.cotr_raster_last_error()


def _device_mesh(H, W, seed):
    verts, tris = ro.jittered_grid(40, 30, 0.45, seed=seed, lo=-0.1, hi=1.1)
    over = np.random.default_rng(seed).uniform(0, 1, (60, 2)).astype(np.float32)   # overlapping extras: ties by index
    verts = np.vstack([verts, over])
    tris = np.vstack([tris, len(verts) - 60 + np.arange(60).reshape(20, 3)]).astype(np.int32)
    d = torch.device('cuda', 0)
    return (torch.from_numpy(verts).to(d), torch.from_numpy(grid_attrs(verts, seed)).to(d), torch.from_numpy(tris).to(d))


def _bytes(T, H, W):
    nb = ctypes.c_size_t()
    assert _lib.load_library().cotr_raster_mesh_scratch_bytes(T, H, W, ctypes.byref(nb)) == 0
    return nb.value


def test_determinism_and_scratch_independence():
    H, W = 768, 1024
    v, a, t = _device_mesh(H, W, 1)
    nb = _bytes(t.shape[0], H, W)
    results = []
    for fill in (0, 255, 17, 0):
        scratch = torch.full((nb + 512,), fill, dtype=torch.uint8, device='cuda')[256:256 + nb]
        out = torch.full((H, W, 2), float('nan'), device='cuda')
        mask = torch.full((H, W), 9, dtype=torch.uint8, device='cuda')
        _abi_call(v, a, t, H, W, scratch, out, mask)
        torch.cuda.synchronize()
        results.append((out.cpu().numpy().tobytes(), mask.cpu().numpy().tobytes()))
    assert all(r == results[0] for r in results)


def test_side_stream_and_graph_replay_match_the_default_stream():
    H, W = 256, 512
    v, a, t = _device_mesh(H, W, 2)
    ref_out, ref_mask = raster_mesh(v, a, t, H, W)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s_out, s_mask = raster_mesh(v, a, t, H, W)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(s_out, ref_out) and torch.equal(s_mask, ref_mask)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_out, g_mask = raster_mesh(v, a, t, H, W)
    g_out.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_out, ref_out) and torch.equal(g_mask, ref_mask)
    v2, a2, t2 = _device_mesh(H, W, 3)                      # replays read the captured buffers' current contents
    v.copy_(v2), a.copy_(a2)
    g.replay()
    e_out, e_mask = raster_mesh(v, a, t, H, W)
    torch.cuda.synchronize()
    assert torch.equal(g_out, e_out) and torch.equal(g_mask, e_mask)


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _oracle_triangulate(corr, shape_a, shape_b):
    spatial = pytest.importorskip('scipy.spatial')
    norm = corr / np.concatenate([shape_a[:2][::-1], shape_b[:2][::-1]])
    simp = spatial.Delaunay(norm[:, :2]).simplices
    out, mask, _, _ = ro.raster(norm[:, :2].astype(np.float32), norm[:, 2:].astype(np.float32), simp, *shape_a[:2])
    return out * np.array(shape_b[:2][::-1]), mask


@pytest.mark.parametrize('shape_a,shape_b,n', [((768, 1024, 3), (600, 800, 3), 1000), ((301, 457, 3), (512, 333, 3), 200)])
def test_triangulate_corr_on_a_homography(shape_a, shape_b, n):
    pytest.importorskip('scipy.spatial')
    rng = np.random.default_rng(n)
    Hm = np.array([[0.7, 0.05, 20.0], [-0.03, 0.75, 15.0], [1e-5, -2e-5, 1.0]])
    pa = rng.uniform(0, 1, (n, 2)) * [shape_a[1], shape_a[0]]
    q = np.hstack([pa, np.ones((n, 1))]) @ Hm.T
    corr = np.hstack([pa, q[:, :2] / q[:, 2:]])
    render, mask = triangulate_corr(corr, shape_a, shape_b, return_mask=True)
    assert render.dtype == np.float64 and render.shape == shape_a[:2] + (2,) and mask.dtype == bool
    ref, ref_mask = _oracle_triangulate(corr, shape_a, shape_b)
    assert np.array_equal(mask, ref_mask)
    assert (render[~mask] == 0).all()
    assert np.abs(render - ref)[mask].max() <= 1e-3
    t_render, t_mask = triangulate_corr(corr, shape_a, shape_b, return_mask=True, as_tensor=True)
    assert t_render.is_cuda and t_render.dtype == torch.float64
    assert np.array_equal(t_render.cpu().numpy(), render) and np.array_equal(t_mask.cpu().numpy(), mask)


def test_demo_chain_sparse_engine_then_triangulate():
    """demo_single_pair.py's chain with seeded weights: FasterSparseEngine.cotr_corr_multiscale(force=True) -> triangulate_corr."""
    pytest.importorskip('scipy.spatial')
    import cotr_amd
    from cotr_amd.inference import FasterSparseEngine
    from cotr_amd.models import build_model
    from cotr_amd.utils.synth import synth_state_dict
    from tests.engine_fixtures import synthetic_pair
    model = build_model(cotr_amd.default_args()).cuda().eval()
    model.load_state_dict(synth_state_dict(0))
    img_a, img_b = synthetic_pair(3)
    eng = FasterSparseEngine(model, 32, mode='tile')
    np.random.seed(0)
    corrs = eng.cotr_corr_multiscale(img_a, img_b, np.linspace(0.5, 0.0625, 4), 1, max_corrs=100, queries_a=None, force=True)
    assert corrs.shape[1] == 4 and len(corrs) >= 3
    render, mask = triangulate_corr(corrs, img_a.shape, img_b.shape, return_mask=True)
    assert render.shape == img_a.shape[:2] + (2,) and np.isfinite(render).all()
    ref, ref_mask = _oracle_triangulate(corrs, img_a.shape, img_b.shape)
    assert np.array_equal(mask, ref_mask) and mask.any()
    assert np.abs(render - ref)[mask].max() <= 1e-3
