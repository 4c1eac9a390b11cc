"""cotr_delaunay without a GPU: the rule's restatement (tests/delaunay_oracle.py) against scipy where the triangulation is
unique and against the rule's properties where it is not, the two forms of the restatement against each other, and the
argument checks of the C ABI (before any HIP call) and of the Python layer."""
import ctypes

import numpy as np
import pytest

from tests import delaunay_oracle as do


def pixel_grid(nx, ny, W, H):
    """an nx x ny grid of integer pixel positions of a W x H image, normalised the way triangulate_corr normalises"""
    gx, gy = np.meshgrid(np.round(np.linspace(0, W - 1, nx)), np.round(np.linspace(0, H - 1, ny)))
    return (np.stack([gx, gy], -1).reshape(-1, 2) / [W, H]).astype(np.float32)


def lattice_with_duplicates(n=200, side=12, seed=5):
    return (np.random.default_rng(seed).integers(0, side, (n, 2)) / side).astype(np.float32)


def two_rows_and_a_point():
    xs = np.arange(9) / 10
    return np.vstack([np.stack([xs, 0 * xs + 0.25], -1), np.stack([xs, 0 * xs + 0.5], -1), [[0.375, 0.875]]]).astype(np.float32)


DEGENERATE = {'grid 16x12 on 640x480': lambda: pixel_grid(16, 12, 640, 480), 'grid 9x7 on 37x53': lambda: pixel_grid(9, 7, 37, 53),
              'grid 16x16 on 256x256': lambda: pixel_grid(16, 16, 256, 256), 'lattice with duplicates': lattice_with_duplicates,
              'two rows and a point': two_rows_and_a_point}


@pytest.mark.parametrize('n', [3, 4, 37, 102])
def test_the_rule_gives_scipys_triangles_where_they_are_unique(n):
    spatial = pytest.importorskip('scipy.spatial')
    P = np.random.default_rng(n).uniform(0, 1, (n, 2)).astype(np.float32)
    tris, status = do.triangulate(P)
    assert status == 0 and do.is_unique(P, tris)
    do.properties(P, tris)
    assert do.as_set(tris) == do.as_set(spatial.Delaunay(P.astype(np.float64)).simplices)


@pytest.mark.parametrize('name', list(DEGENERATE))
def test_the_rule_triangulates_degenerate_inputs_properly(name):
    P = DEGENERATE[name]()
    tris, status = do.triangulate(P)
    assert status == 0 and len(tris) > 0
    do.properties(P, tris)
    assert not do.is_unique(P, tris)                      # every one of these has cocircular quadruples: the tie-break decides


def test_collinear_points_give_no_triangle():
    P = np.stack([np.arange(7) / 8, np.arange(7) / 16], -1).astype(np.float32)
    tris, status = do.triangulate(P)
    assert status == 0 and len(tris) == 0
    do.properties(P, tris)


def test_invalid_points_take_no_part():
    P = np.random.default_rng(1).uniform(0, 1, (40, 2)).astype(np.float32)
    P[3], P[9], P[17], P[20], P[30] = (np.nan, 0.5), (0.5, np.inf), (4.5, 0.5), P[2], P[35]
    S = do.snap(P)
    assert [i for i, s in enumerate(S) if s is None] == [3, 9, 17, 20, 35]      # 35 repeats 30: the lower index is the valid one
    tris, status = do.triangulate(P)
    do.properties(P, tris)
    assert not set(tris.ravel()) & {3, 9, 17, 20, 35}


@pytest.mark.parametrize('P', [pixel_grid(16, 16, 256, 256), lattice_with_duplicates(200, 16, 6),
                               (np.random.default_rng(2).integers(0, 4096, (150, 2)) / 4096).astype(np.float32)],
                         ids=['grid 16x16 on 256x256', 'k/16 lattice with duplicates', 'random k/4096'])
def test_the_int64_form_equals_the_python_int_form(P):
    a, b = do.triangulate(P, 'int64'), do.triangulate(P, 'int')
    assert len(a[0]) > 0 and np.array_equal(a[0], b[0]) and a[1] == b[1] == 0


def large_lattice(n):
    """n distinct random points of the k/4096 lattice; the seed makes the triangulation unique at n = 1000"""
    rng = np.random.default_rng(7)
    k = rng.choice(4096 * 4096, n, replace=False)
    return (np.stack([k % 4096, k // 4096], -1) / 4096).astype(np.float32)


def test_the_large_case_is_unique_and_equals_scipys():
    spatial = pytest.importorskip('scipy.spatial')
    P = large_lattice(1000)
    tris, status = do.triangulate(P, 'int64')
    assert status == 0 and do.is_unique(P, tris)
    do.properties(P, tris)
    assert do.as_set(tris) == do.as_set(spatial.Delaunay(P.astype(np.float64)).simplices)


# ---- argument checks ----------------------------------------------------------------------------------------------------
def test_python_argument_checks():
    from cotr_amd.inference import delaunay, triangulate_corr
    for bad in (np.zeros((5, 3), np.float32), np.zeros(6, np.float32), np.zeros((2, 2, 2), np.float32), np.zeros((65537, 2), np.float32)):
        with pytest.raises(ValueError):
            delaunay(bad)
    corr = np.zeros((5, 4))
    for bad in ('host', 'scipy', ''):
        with pytest.raises(ValueError, match='device'):
            triangulate_corr(corr, (8, 8), (8, 8), simplices=bad)
    with pytest.raises(ValueError, match=r'\[N, 4\]'):
        triangulate_corr(np.zeros((5, 3)), (8, 8), (8, 8), simplices='device')


def test_abi_argument_errors_without_a_gpu():
    from cotr_amd import _lib
    from cotr_amd.build import build_library
    build_library()
    lib = _lib.load_library()
    nb = ctypes.c_size_t()
    P = ctypes.c_void_p(4096)                # never dereferenced: every case fails its host-side check
    assert lib.cotr_delaunay_scratch_bytes(100, ctypes.byref(nb)) == 0 and nb.value >= 100 * 8
    need = nb.value

    def call(verts=P, n=100, tris=P, info=P, scratch=P, nbytes=need):
        return lib.cotr_delaunay(verts, n, tris, info, scratch, nbytes, None)

    cases = {'n = -1': dict(n=-1), 'n = 65537': dict(n=65537), 'null verts': dict(verts=None), 'null tris': dict(tris=None),
             'null info': dict(info=None), 'null scratch': dict(scratch=None), 'too little scratch': dict(nbytes=need - 1),
             'misaligned scratch': dict(scratch=ctypes.c_void_p(4096 + 8))}
    for what, kw in cases.items():
        assert call(**kw) == -1, what
        assert lib.cotr_raster_last_error(), what
    assert b'65536' in (call(n=65537), lib.cotr_raster_last_error())[1]
    assert b'scratch' in (call(nbytes=need - 1), lib.cotr_raster_last_error())[1]
    assert lib.cotr_delaunay_scratch_bytes(-1, ctypes.byref(nb)) == -1
    assert lib.cotr_delaunay_scratch_bytes(65537, ctypes.byref(nb)) == -1
    assert lib.cotr_delaunay_scratch_bytes(5, None) == -1
    assert [lib.cotr_delaunay_max_tris(n) for n in (0, 1, 1000, 65536)] == [0, 2, 2000, 131072]
    assert lib.cotr_delaunay_max_tris(-1) == -1 and lib.cotr_delaunay_max_tris(65537) == -1
    sizes = []
    for n in (0, 1, 1000, 65536):
        assert lib.cotr_delaunay_scratch_bytes(n, ctypes.byref(nb)) == 0
        sizes.append(nb.value)
    assert sizes[0] == 0 and sizes == sorted(sizes)
