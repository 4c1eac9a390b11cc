"""The mesh of a TSDF volume without a GPU: the numpy restatement (tests/mesh_oracle.py) against a scalar per-cell loop and
against volumes whose surface is known - spheres (closed, oriented, Euler characteristic 2, every vertex within the bound of
linear interpolation), planes between and through lattice points, an unobserved slab - the coverage of all 96 (tetrahedron, sign
pattern) cases, and the argument checks of the C ABI (they run before any HIP call), of ``extract_mesh`` and of ``write_ply``."""
import ctypes
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.build import declared_symbols
from cotr_amd.inference import TsdfVolume, extract_mesh, write_ply
from tests import mesh_oracle as mo

NAMES = ['cotr_tsdf_mesh', 'cotr_tsdf_mesh_scratch_bytes']
SPHERES = ((9, 2.7), (12, 4.0), (17, 6.3))
ORIGIN, VOXEL = (0.31, -1.27, 2.05), 0.05


# ---- the restatement against a scalar loop ----------------------------------------------------------------------------------
# The four rows of the rule's table written out by hand for each set of inside vertices, not taken from the restatement: the
# vertex E_ab as the two digits ab.  One inside {a} and three inside with {a} outside give (E_ab, E_ac, E_ad); two inside {a, b}
# with {c, d} outside give (E_ac, E_ad, E_bd), then (E_ac, E_bd, E_bc).
ONE = {0: ('01', '02', '03'), 1: ('01', '12', '13'), 2: ('02', '12', '23'), 3: ('03', '13', '23')}
TWO = {(0, 1): (('02', '03', '13'), ('02', '13', '12')), (0, 2): (('01', '03', '23'), ('01', '23', '12')),
       (0, 3): (('01', '02', '23'), ('01', '23', '13')), (1, 2): (('01', '13', '23'), ('01', '23', '02')),
       (1, 3): (('01', '12', '23'), ('01', '23', '03')), (2, 3): (('02', '12', '13'), ('02', '13', '03'))}


def table_rows(S):
    inside = tuple(a for a in range(4) if S >> a & 1)
    if len(inside) in (0, 4):
        return ()
    if len(inside) == 2:
        return TWO[inside]
    return (ONE[inside[0] if len(inside) == 1 else (set(range(4)) - set(inside)).pop()],)


def test_the_table_written_out_is_the_restatements():
    for S in range(16):
        assert [tuple((int(e[0]), int(e[1])) for e in tri) for tri in table_rows(S)] == mo.pattern_triangles(S), S


def scalar_mesh(tsdf, weight, origin, voxel):
    """the rule cell by cell and edge by edge, as it reads; the winding from the positions themselves: a triangle is turned over
    iff its normal points against the gradient of the tetrahedron's linear interpolant (no triangle here has zero area)"""
    Nz, Ny, Nx = tsdf.shape
    inside = lambda p: bool(tsdf[p[2], p[1], p[0]] <= 0)   # noqa: E731
    cells = [(i, j, k) for k in range(Nz - 1) for j in range(Ny - 1) for i in range(Nx - 1)
             if all(weight[k + c, j + b, i + a] > 0 for a in (0, 1) for b in (0, 1) for c in (0, 1))]
    perms = list(itertools.permutations(range(3)))
    e = np.eye(3, dtype=int)
    edges = set()
    for c in cells:
        for p in perms:
            q = [np.array(c), np.array(c) + e[p[0]], np.array(c) + e[p[0]] + e[p[1]], np.array(c) + 1]
            for a in range(4):
                for b in range(a + 1, 4):
                    if inside(q[a]) != inside(q[b]):
                        d = q[b] - q[a]
                        edges.add(((q[a][2] * Ny + q[a][1]) * Nx + q[a][0], int(d[0] + 2 * d[1] + 4 * d[2])))
    edges = sorted(edges)
    number = {key: n for n, key in enumerate(edges)}
    verts = []
    for v, dcode in edges:
        p = np.array([v % Nx, v // Nx % Ny, v // (Nx * Ny)])
        d = np.array([dcode & 1, dcode >> 1 & 1, dcode >> 2])
        fa, fb = float(tsdf[p[2], p[1], p[0]]), float(tsdf[p[2] + d[2], p[1] + d[1], p[0] + d[0]])
        t = fa / (fa - fb)
        verts.append([float(origin[a]) + voxel * ((float(p[a]) + t) if d[a] else float(p[a])) for a in range(3)])
    verts = np.array(verts).reshape(-1, 3)
    tris = []
    for c in cells:
        for p in perms:
            q = [np.array(c), np.array(c) + e[p[0]], np.array(c) + e[p[0]] + e[p[1]], np.array(c) + 1]
            f = np.array([float(tsdf[x[2], x[1], x[0]]) for x in q])
            S = sum(int(inside(q[a])) << a for a in range(4))
            E = lambda a, b: number[((q[a][2] * Ny + q[a][1]) * Nx + q[a][0], int((q[b] - q[a]) @ (1, 2, 4)))]   # noqa: E731
            grad = np.linalg.solve(np.array([q[a] - q[0] for a in (1, 2, 3)], float), f[1:] - f[0])
            for tri in table_rows(S):
                A, B, C = (E(int(e[0]), int(e[1])) for e in tri)
                if np.cross(verts[B] - verts[A], verts[C] - verts[A]) @ grad < 0:
                    B, C = C, B
                tris.append((A, B, C))
    return verts, np.array(tris, np.int32).reshape(-1, 3), len(cells)


@pytest.mark.parametrize('dims, holes', [((4, 4, 4), 0.0), ((4, 4, 4), 0.1), ((3, 5, 7), 0.0), ((3, 5, 7), 0.15)], ids=['4x4x4', '4x4x4-holes', '3x5x7', '3x5x7-holes'])
def test_restatement_against_a_scalar_loop(dims, holes):
    tsdf, weight = mo.random_volume(dims, 5, holes)
    o = mo.mesh(tsdf, weight, ORIGIN, VOXEL)
    verts, tris, cells = scalar_mesh(tsdf, weight, ORIGIN, VOXEL)
    assert o['info'].tolist() == [1, len(verts), len(tris), cells] and len(tris) > 50
    assert np.array_equal(o['verts'], verts) and np.array_equal(o['tris'], tris)


def test_the_winding_table_is_one_word_for_the_even_and_one_for_the_odd_permutations():
    w = mo.winding_table()
    assert np.array_equal(w[0], w[3]) and np.array_equal(w[0], w[4]) and np.array_equal(w[1], w[2]) and np.array_equal(w[1], w[5])
    used = np.array([[n < len(mo.pattern_triangles(S)) for n in (0, 1)] for S in range(16)])
    assert np.array_equal(w[0][used], ~w[1][used]) and not w[:, ~used].any()


# ---- spheres --------------------------------------------------------------------------------------------------------------
_SPHERES = {}


def sphere_mesh(N, r):
    if (N, r) not in _SPHERES:
        tsdf, weight, centre = mo.sphere(N, r)
        _SPHERES[N, r] = (tsdf, weight, centre, mo.mesh(tsdf, weight, (0.0, 0.0, 0.0), 1.0, normals=True))
    return _SPHERES[N, r]


def directed_edges(tris):
    """-> (the directed edges as a * 2^32 + b, sorted; True where an edge's reverse is present)"""
    t = tris.astype(np.int64)
    a, b = np.concatenate([t[:, 0], t[:, 1], t[:, 2]]), np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    fwd, rev = a << 32 | b, b << 32 | a
    return fwd, np.isin(fwd, rev)


def tet_gradients(tsdf, o):
    """the gradient of the linear interpolant of the tetrahedron each triangle comes from, [T, 3]"""
    Nz, Ny, Nx = tsdf.shape
    c = o['tri_cell']
    base = np.stack([c % Nx, c // Nx % Ny, c // (Nx * Ny)], -1)
    q = base[:, None, :] + mo.tetrahedra()[o['tri_tet']]   # [T, 4, 3]
    f = tsdf[q[..., 2], q[..., 1], q[..., 0]].astype(np.float64)
    return np.linalg.solve((q[:, 1:] - q[:, :1]).astype(np.float64), (f[:, 1:] - f[:, :1])[..., None])[..., 0]


@pytest.mark.parametrize('N, r', SPHERES, ids=lambda v: str(v))
def test_a_sphere_is_closed_oriented_and_of_genus_0(N, r):
    tsdf, weight, centre, o = sphere_mesh(N, r)
    V, T = int(o['info'][1]), int(o['info'][2])
    fwd, has_reverse = directed_edges(o['tris'])
    assert len(np.unique(fwd)) == len(fwd) and has_reverse.all()   # every directed edge once, and its reverse once
    E = len(fwd) // 2
    assert V - E + T == 2, (V, E, T)
    A, B, C = (o['verts'][o['tris'][:, n]] for n in range(3))
    volume = (A * np.cross(B, C)).sum() / 6
    assert volume > 0 and abs(volume - 4 / 3 * np.pi * r ** 3) < 0.1 * volume
    normal = np.cross(B - A, C - A)
    proper = np.linalg.norm(normal, axis=1) > 0
    dots = (normal * tet_gradients(tsdf, o)).sum(1)
    print(f'sphere r = {r} in {N}^3: {V} vertices, {T} triangles, {E} edges, volume {volume:.3f}, {int((~proper).sum())} triangles of no area')
    assert proper.sum() > T // 2 and (dots[proper] > 0).all()
    # the normals: all there (the sphere lies inside the observed volume), and outwards within the error of a central difference
    away = (o['verts'] - centre) / np.linalg.norm(o['verts'] - centre, axis=1, keepdims=True)
    assert not np.isnan(o['normals']).any() and ((o['normals'] * away).sum(1) > 0.95).all()


@pytest.mark.parametrize('N, r', SPHERES, ids=lambda v: str(v))
def test_every_vertex_of_a_sphere_lies_within_the_bound_of_linear_interpolation(N, r):
    # along an edge of length L <= sqrt 3 the distance has second derivative <= 1 / (r - L): the linear interpolant is off by at most
    # L^2 / 8 of that, and the samples by their float32 rounding
    tsdf, weight, centre, o = sphere_mesh(N, r)
    bound = 3 / (8 * (r - np.sqrt(3))) + 2.0 ** -20 * r
    err = np.abs(np.linalg.norm(o['verts'] - centre, axis=1) - r).max()
    print(f'sphere r = {r}: vertices within {err:.3f} voxels of it (bound {bound:.3f})')
    assert err <= bound


# ---- planes and holes -----------------------------------------------------------------------------------------------------
def test_a_plane_between_lattice_planes_carries_every_vertex():
    z0 = 3.375   # k - z0 is exact in float32, so t = z0 - k exactly and only the two roundings of origin + voxel * g remain
    tsdf, weight = mo.plane_volume((5, 4, 8), z0)
    o = mo.mesh(tsdf, weight, ORIGIN, VOXEL, normals=True)
    exact = Fraction(ORIGIN[2]) + Fraction(VOXEL) * Fraction(z0)
    err = max(abs(Fraction(z) - exact) for z in o['verts'][:, 2])
    # the edges that rise from the 5 x 4 voxels of layer 3: 20 along z, 16 + 15 across a face, 12 across a cell; a layer of 4 x 3
    # cells, each cut into 6 tetrahedra of which 4 have one vertex on a side (z first or last in the permutation) and 2 have two
    assert o['info'].tolist() == [1, 20 + 16 + 15 + 12, 4 * 3 * (4 * 1 + 2 * 2), 4 * 3 * 7]
    assert err <= 2.0 ** -52 * (abs(ORIGIN[2]) + VOXEL * z0)
    # a normal needs the samples one voxel to each side inside the box; z - z0 is trilinear, so the gradient there is exact
    gx, gy = (o['verts'][:, 0] - ORIGIN[0]) / VOXEL, (o['verts'][:, 1] - ORIGIN[1]) / VOXEL
    inner = (gx > 1 + 1e-9) & (gx < 3 - 1e-9) & (gy > 1 + 1e-9) & (gy < 2 - 1e-9)
    rim = (gx < 1 - 1e-9) | (gx > 3 + 1e-9) | (gy < 1 - 1e-9) | (gy > 2 + 1e-9)
    assert inner.sum() >= 3 and (o['normals'][inner] == [0.0, 0.0, 1.0]).all() and np.isnan(o['normals'][rim]).all() and rim.sum() > inner.sum()
    A, B, C = (o['verts'][o['tris'][:, n]] for n in range(3))
    n = np.cross(B - A, C - A)
    assert (n[:, 2] > 0).all() and (np.abs(n[:, :2]) <= 1e-15).all()
    assert abs(np.linalg.norm(n, axis=1).sum() / 2 - (4 * VOXEL) * (3 * VOXEL)) < 1e-12   # the triangles tile the 4 x 3 cells of the plane


def test_a_plane_through_lattice_points_keeps_its_triangles_of_no_area():
    dims = (5, 4, 8)
    through, between = mo.mesh(*mo.plane_volume(dims, 3.0), ORIGIN, VOXEL), mo.mesh(*mo.plane_volume(dims, 3.5), ORIGIN, VOXEL)
    # the value 0 counts as inside: the same sign pattern as the plane at 3.5, so the same counts and the same triangles
    assert through['info'].tolist() == between['info'].tolist() and np.array_equal(through['tris'], between['tris'])
    A, B, C = (through['verts'][through['tris'][:, n]] for n in range(3))
    area = np.linalg.norm(np.cross(B - A, C - A), axis=1)
    assert (area == 0).sum() > 0 and (area > 0).sum() > 0 and len(area) == through['info'][2]
    assert (through['verts'][:, 2] == ORIGIN[2] + VOXEL * 3.0).all()
    A, B, C = (between['verts'][between['tris'][:, n]] for n in range(3))
    assert (np.linalg.norm(np.cross(B - A, C - A), axis=1) > 0).all()


def test_an_unobserved_slab_opens_the_mesh_exactly_there():
    tsdf, weight, centre, full = sphere_mesh(17, 6.3)
    holed = weight.copy()
    holed[8] = 0   # the cells of layers 7 and 8 are invalid
    o = mo.mesh(tsdf, holed, (0.0, 0.0, 0.0), 1.0, normals=True)
    layer = full['tri_cell'] // (17 * 17)
    kept = (layer != 7) & (layer != 8)
    assert o['info'][3] == 16 * 16 * 14 and o['info'][2] == kept.sum() and 0 < kept.sum() < len(kept)
    assert np.array_equal(o['verts'][o['tris']], full['verts'][full['tris'][kept]])   # the same triangles in the same order, renumbered
    fwd, has_reverse = directed_edges(o['tris'])
    assert len(np.unique(fwd)) == len(fwd) and (~has_reverse).any()
    rim = np.unique(np.concatenate([fwd[~has_reverse] >> 32, fwd[~has_reverse] & 0xffffffff]))
    z = o['verts'][:, 2]
    assert np.isin(z[rim], (7.0, 9.0)).all() and not ((z > 7) & (z < 9)).any()
    # a normal needs the cells one voxel around the vertex: NaN next to the slab, and only there
    bad = np.isnan(o['normals']).any(1)
    assert bad.any() and (np.abs(z[bad] - 8) <= 3).all() and not bad[np.abs(z - 8) > 3].any() and np.isnan(o['normals'][bad]).all()


@pytest.mark.parametrize('dims, seed, holes', [((8, 8, 8), 0, 0.1), ((6, 6, 6), 1, 0.0)], ids=['8x8x8-holes', '6x6x6'])
def test_the_random_volumes_reach_all_96_cases(dims, seed, holes):
    o = mo.mesh(*mo.random_volume(dims, seed, holes), ORIGIN, VOXEL)
    assert o['cases'].shape == (6, 16) and o['cases'].all()
    assert (o['info'][3] < np.prod(np.array(dims) - 1)) == (holes > 0)


def test_found_0_is_an_empty_mesh():
    o = mo.mesh(*mo.random_volume((4, 4, 4), 0), ORIGIN, VOXEL, normals=True, found=[0])
    assert (o['info'] == 0).all() and o['verts'].shape == (0, 3) and o['tris'].shape == (0, 3) and o['normals'].shape == (0, 3)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and name in declared_symbols()
        assert getattr(_lib.load_library(), name) is not None


P = ctypes.c_void_p(4096)              # never dereferenced: every call below fails its checks before any HIP call
ODD8, ODD4 = ctypes.c_void_p(4100), ctypes.c_void_p(4098)
NAN, INF = float('nan'), float('inf')


def test_scratch_bytes_and_its_argument_errors():
    lib = _lib.load_library()
    n = ctypes.c_size_t()
    assert lib.cotr_tsdf_mesh_scratch_bytes(8, 8, 8, ctypes.byref(n)) == 0 and n.value >= 6 * 512
    small = n.value
    assert lib.cotr_tsdf_mesh_scratch_bytes(512, 512, 512, ctypes.byref(n)) == 0 and 6 << 27 <= n.value <= (6 << 27) + (1 << 23) and n.value > small
    for dims in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (512, 512, 513), (1 << 16, 1 << 16, 1 << 16), (1 << 22, 1 << 21, 1 << 21), (1 << 28, 2, 2)):   # 2^64 wraps to 0
        assert lib.cotr_tsdf_mesh_scratch_bytes(*dims, ctypes.byref(n)) == -1
        assert b'2^27' in lib.cotr_raster_last_error() and b'cotr_tsdf_mesh_scratch_bytes' in lib.cotr_raster_last_error()
    assert lib.cotr_tsdf_mesh_scratch_bytes(8, 8, 8, None) == -1 and b'NULL' in lib.cotr_raster_last_error()


def test_mesh_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    O = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    n = ctypes.c_size_t()
    assert lib.cotr_tsdf_mesh_scratch_bytes(8, 8, 8, ctypes.byref(n)) == 0

    def call(tsdf=P, weight=P, Nx=8, Ny=8, Nz=8, origin=O, voxel=0.1, found=None, verts=P, cap_verts=10, normals=None, tris=P, cap_tris=10, info=P,
             scratch=P, nbytes=n.value):
        return lib.cotr_tsdf_mesh(tsdf, weight, Nx, Ny, Nz, origin, voxel, found, verts, cap_verts, normals, tris, cap_tris, info, scratch, nbytes, None)
    cases = ((dict(Nx=1), b'2^27'), (dict(Ny=1), b'2^27'), (dict(Nz=1), b'2^27'), (dict(Nx=512, Ny=512, Nz=513), b'2^27'),
             (dict(Nx=1 << 16, Ny=1 << 16, Nz=1 << 16), b'2^27'), (dict(Nx=1 << 22, Ny=1 << 21, Nz=1 << 21), b'2^27'), (dict(voxel=0.0), b'voxel'), (dict(voxel=-1.0), b'voxel'), (dict(voxel=INF), b'voxel'),
             (dict(voxel=NAN), b'voxel'), (dict(tsdf=None), b'NULL'), (dict(weight=None), b'NULL'), (dict(origin=None), b'NULL'),
             (dict(origin=(ctypes.c_double * 3)(0.0, NAN, 0.0)), b'origin'), (dict(origin=(ctypes.c_double * 3)(INF, 0.0, 0.0)), b'origin'),
             (dict(tsdf=ODD4), b'aligned'), (dict(weight=ODD4), b'aligned'),
             (dict(cap_verts=-1), b'cap_verts'), (dict(cap_tris=-1), b'cap_tris'), (dict(verts=None), b'NULL'), (dict(tris=None), b'NULL'),
             (dict(info=None), b'NULL'), (dict(verts=None, cap_verts=0, info=None), b'NULL'), (dict(found=ODD4), b'aligned'), (dict(verts=ODD8), b'aligned'),
             (dict(normals=ODD8), b'aligned'), (dict(tris=ODD4), b'aligned'), (dict(info=ODD4), b'aligned'), (dict(scratch=None), b'scratch'),
             (dict(nbytes=n.value - 1), b'scratch'), (dict(nbytes=0), b'scratch'), (dict(scratch=ODD8), b'scratch'),
             (dict(Nx=9, nbytes=n.value), b'scratch'))
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error() and b'cotr_tsdf_mesh:' in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
def _volume(dims=(8, 8, 8)):
    """a volume's scalars without its tensors: every check below fails before a tensor is read"""
    v = TsdfVolume.__new__(TsdfVolume)
    v.origin, v.voxel, v.dims, v.trunc, v.max_weight = np.zeros(3), 0.1, dims, 0.3, 64.0
    v.device, v.tsdf, v.weight = torch.device('cpu'), None, None
    return v


def test_extract_mesh_argument_errors_without_a_gpu():
    for kw, word in ((dict(volume=None), 'TsdfVolume'), (dict(volume=_volume((512, 512, 513))), '2\\^27'), (dict(max_verts=10), 'go together'),
                     (dict(max_tris=10), 'go together'), (dict(max_verts=-1, max_tris=10), 'max_verts'), (dict(max_verts=10, max_tris=-1), 'max_tris'),
                     (dict(max_verts=1.5, max_tris=10), 'max_verts'), (dict(max_verts=10, max_tris=1 << 31), 'max_tris')):
        args = dict(volume=_volume())
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            extract_mesh(**args)


def test_write_ply_reads_back_and_drops_the_padding(tmp_path):
    tsdf, weight, centre, o = sphere_mesh(9, 2.7)
    padded = np.vstack([o['tris'], np.full((5, 3), -1, np.int32)])
    write_ply(tmp_path / 'a.ply', o['verts'], padded)
    cols, v, f = mo.read_ply(tmp_path / 'a.ply')
    assert cols == ['x', 'y', 'z'] and np.array_equal(v, o['verts']) and np.array_equal(f, o['tris'])
    write_ply(tmp_path / 'b.ply', torch.from_numpy(o['verts']), torch.from_numpy(padded), torch.from_numpy(o['normals']))
    cols, v, f = mo.read_ply(tmp_path / 'b.ply')
    assert cols == ['x', 'y', 'z', 'nx', 'ny', 'nz'] and np.array_equal(v[:, :3], o['verts']) and np.array_equal(v[:, 3:], o['normals'])
    assert np.array_equal(f, o['tris'])
    write_ply(tmp_path / 'c.ply', np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    cols, v, f = mo.read_ply(tmp_path / 'c.ply')
    assert v.shape == (0, 3) and f.shape == (0, 3)
    for kw, word in ((dict(verts=o['verts'][:, :2]), 'verts'), (dict(tris=o['tris'][:, :2]), 'tris'), (dict(tris=o['tris'].astype(np.float64)), 'tris'),
                     (dict(verts=o['verts'][:-1]), 'outside'), (dict(normals=o['normals'][:-1]), 'normals'),
                     (dict(tris=np.array([[0, 1, -2]], np.int32)), 'outside')):
        args = dict(path=tmp_path / 'bad.ply', verts=o['verts'], tris=o['tris'])
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            write_ply(**args)
