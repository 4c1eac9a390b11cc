"""numpy float64 restatement of ``cotr_tsdf_mesh`` (cotr_amd/csrc/tsdf.hip): marching tetrahedra on the Kuhn
split of every cell of a TSDF volume, with the vertex and triangle order, the interpolation and the normals in the device's
order of operations, so that vertices, triangles and normals can be compared bit for bit.

The 6 x 16 winding table is derived here, in integers, and not copied from the kernel: with the doubled midpoints of the
tetrahedron's edges as stand-in vertices and D = |S| sum(outside q) - |outside| sum(inside q) (a vector from the inside
vertices' mean to the outside vertices' mean), a triangle is turned over iff ((B - A) x (C - A)) . D < 0.  The product is never
0 for a proper tetrahedron: the stand-in surface separates the two sets.

numpy only.  Test infrastructure."""
import functools
import itertools

import numpy as np

AXES = np.eye(3, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def tetrahedra():
    """-> int [6, 4, 3]: the vertices q0 .. q3 of T_0 .. T_5 as offsets (x, y, z) from the cell's low corner"""
    out = []
    for p in itertools.permutations(range(3)):   # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx
        q1 = AXES[p[0]]
        out.append([np.zeros(3, np.int64), q1, q1 + AXES[p[1]], np.ones(3, np.int64)])
    return np.array(out)


def pattern_triangles(S):
    """the sign pattern S (bit a: q_a inside) -> its triangles, each three edges (a, b) with a < b, in the rule's order"""
    inside = [a for a in range(4) if S >> a & 1]
    outside = [a for a in range(4) if not S >> a & 1]
    e = lambda a, b: (min(a, b), max(a, b))   # noqa: E731
    if len(inside) in (0, 4):
        return []
    if len(inside) == 1:
        return [tuple(e(inside[0], b) for b in outside)]
    if len(inside) == 3:
        return [tuple(e(outside[0], b) for b in inside)]
    (a, b), (c, d) = inside, outside
    return [(e(a, c), e(a, d), e(b, d)), (e(a, c), e(b, d), e(b, c))]


@functools.lru_cache(maxsize=None)
def winding_table():
    """-> bool [6, 16, 2]: triangle n of pattern S of tetrahedron m leaves with its second and third vertex swapped"""
    swap = np.zeros((6, 16, 2), bool)
    for m, q in enumerate(tetrahedra()):
        for S in range(1, 15):
            inside = [a for a in range(4) if S >> a & 1]
            outside = [a for a in range(4) if not S >> a & 1]
            D = len(inside) * sum(q[a] for a in outside) - len(outside) * sum(q[a] for a in inside)
            for n, tri in enumerate(pattern_triangles(S)):
                A, B, C = (q[a] + q[b] for a, b in tri)   # twice the midpoints
                dot = int(np.cross(B - A, C - A) @ D)
                assert dot != 0
                swap[m, S, n] = dot < 0
    return swap


def corner_code(q):
    return int(q[0] + 2 * q[1] + 4 * q[2])


def _shift(a, d, dims):
    """the view of a [Nz, Ny, Nx] at v + d for the voxels v with v + d inside -> (view at v, view at v + d) trimmed alike"""
    Nx, Ny, Nz = dims
    lo = a[:Nz - d[2], :Ny - d[1], :Nx - d[0]]
    hi = a[d[2]:, d[1]:, d[0]:]
    return lo, hi


def sample_grid(tsdf, weight, g):
    """g [..., 3] grid coordinates -> (valid, f): ``ts_trilinear``'s value and validity"""
    Nz, Ny, Nx = tsdf.shape
    N = np.array([Nx, Ny, Nz], np.float64)
    with np.errstate(all='ignore'):
        i0 = np.floor(g)
        inb = ((g >= 0) & (g < N - 1)).all(-1)
        b = np.where(inb[..., None], i0, 0).astype(np.int64)
        fr = g - i0
    x, y, z = b[..., 0], b[..., 1], b[..., 2]
    corner = lambda a, dx, dy, dz: a[z + dz, y + dy, x + dx]   # noqa: E731
    seen = np.ones(inb.shape, bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                seen &= corner(weight, dx, dy, dz) > 0
    a = {(dx, dy, dz): corner(tsdf, dx, dy, dz).astype(np.float64) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
    with np.errstate(all='ignore'):
        c = {(dy, dz): a[0, dy, dz] + fr[..., 0] * (a[1, dy, dz] - a[0, dy, dz]) for dy in (0, 1) for dz in (0, 1)}
        e = {dz: c[0, dz] + fr[..., 1] * (c[1, dz] - c[0, dz]) for dz in (0, 1)}
        f = e[0] + fr[..., 2] * (e[1] - e[0])
    return inb & seen, f


def mesh(tsdf, weight, origin, voxel, normals=False, found=None):
    """-> dict(verts float64 [V, 3], tris int32 [T, 3], normals float64 [V, 3] or None, info int32 [4] = (ok, V, T, valid cells),
    vert_voxel int64 [V] and vert_dcode [V]: the edge of each vertex, tri_cell int64 [T] and tri_tet [T]: where each triangle
    comes from, cases bool [6, 16]: the (tetrahedron, pattern) pairs met in valid cells)"""
    tsdf, weight = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
    Nz, Ny, Nx = tsdf.shape
    dims = (Nx, Ny, Nz)
    if found is not None and found[0] == 0:
        return dict(verts=np.zeros((0, 3)), tris=np.zeros((0, 3), np.int32), normals=np.zeros((0, 3)) if normals else None,
                    info=np.zeros(4, np.int32), vert_voxel=np.zeros(0, np.int64), vert_dcode=np.zeros(0, np.int64), tri_cell=np.zeros(0, np.int64),
                    tri_tet=np.zeros(0, np.int64), cases=np.zeros((6, 16), bool))
    o = np.asarray(origin, np.float64)
    with np.errstate(invalid='ignore'):
        inside, seen = tsdf <= 0, weight > 0
    # valid[k, j, i] over the whole grid: False where the cell does not exist
    valid = np.zeros((Nz, Ny, Nx), bool)
    v = np.ones((Nz - 1, Ny - 1, Nx - 1), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                v &= seen[dz:Nz - 1 + dz, dy:Ny - 1 + dy, dx:Nx - 1 + dx]
    valid[:Nz - 1, :Ny - 1, :Nx - 1] = v
    # live[k, j, i, dcode - 1]
    live = np.zeros((Nz, Ny, Nx, 7), bool)
    for dcode in range(1, 8):
        d = (dcode & 1, dcode >> 1 & 1, dcode >> 2)
        a, b = _shift(inside, d, dims)
        cross = a != b
        # the cells that hold edge (v, d): c = v - s with s over the subsets of the axes d does not run along
        held = np.zeros(cross.shape, bool)
        free = [ax for ax in range(3) if not d[ax]]
        for bits in itertools.product((0, 1), repeat=len(free)):
            s = [0, 0, 0]
            for ax, bit in zip(free, bits):
                s[ax] = bit
            # valid at v - s for the voxels v of ``cross`` (v_a from 0 .. N_a - 1 - d_a), False where v - s leaves the grid
            shape = cross.shape
            part = np.zeros(shape, bool)
            part[s[2]:, s[1]:, s[0]:] = valid[:shape[0] - s[2], :shape[1] - s[1], :shape[2] - s[0]]
            held |= part
        live[:Nz - d[2], :Ny - d[1], :Nx - d[0], dcode - 1] = cross & held
    flat = live.reshape(-1)
    where = np.flatnonzero(flat)
    vid = np.full(flat.shape, -1, np.int64)
    vid[where] = np.arange(where.size)
    vid = vid.reshape(-1, 7)
    vv, vd = where // 7, where % 7 + 1
    dx, dy, dz = vd & 1, vd >> 1 & 1, vd >> 2
    i, j, k = vv % Nx, vv // Nx % Ny, vv // (Nx * Ny)
    fa = tsdf[k, j, i].astype(np.float64)
    fb = tsdf[k + dz, j + dy, i + dx].astype(np.float64)
    with np.errstate(all='ignore'):
        t = fa / (fa - fb)
        g = np.stack([np.where(dd == 1, c.astype(np.float64) + t, c.astype(np.float64)) for dd, c in ((dx, i), (dy, j), (dz, k))], -1)
        verts = np.stack([o[a] + voxel * g[:, a] for a in range(3)], -1)
    out = dict(verts=verts, normals=None, vert_voxel=vv, vert_dcode=vd)
    if normals:
        G, ok = [], np.ones(len(g), bool)
        for a in range(3):
            (vp, fp), (vm, fm) = sample_grid(tsdf, weight, g + AXES[a].astype(np.float64)), sample_grid(tsdf, weight, g - AXES[a].astype(np.float64))
            ok &= vp & vm
            G.append(fp - fm)
        with np.errstate(all='ignore'):
            L = np.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
            ok &= L > 0
            nrm = np.stack([G[a] / L for a in range(3)], -1)
        nrm[~ok] = np.nan
        out['normals'] = nrm
    # triangles
    cells = np.flatnonzero(valid.reshape(-1))
    ci, cj, ck = cells % Nx, cells // Nx % Ny, cells // (Nx * Ny)
    swap = winding_table()
    ins_flat = inside.reshape(-1)
    lin = lambda q: cells + q[0] + q[1] * Nx + q[2] * Nx * Ny   # noqa: E731
    rows, keys, tets, seen_cases = [], [], [], np.zeros((6, 16), bool)
    for m, q in enumerate(tetrahedra()):
        S = sum(ins_flat[lin(q[a])].astype(np.int64) << a for a in range(4)) if len(cells) else np.zeros(0, np.int64)
        for s in np.unique(S):
            seen_cases[m, s] = True
            pick = np.flatnonzero(S == s)
            for n, tri in enumerate(pattern_triangles(int(s))):
                idx = [vid[lin(q[a])[pick], corner_code(q[b]) - corner_code(q[a]) - 1] for a, b in tri]
                if swap[m, s, n]:
                    idx[1], idx[2] = idx[2], idx[1]
                rows.append(np.stack(idx, -1))
                keys.append(cells[pick] * 12 + m * 2 + n)
                tets.append(np.full(len(pick), m, np.int64))
    if rows:
        rows, keys, tets = np.concatenate(rows), np.concatenate(keys), np.concatenate(tets)
        order = np.argsort(keys, kind='stable')
        rows, keys, tets = rows[order], keys[order], tets[order]
    else:
        rows, keys, tets = np.zeros((0, 3), np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    assert (rows >= 0).all() and (len(verts) == 0 or np.array_equal(np.unique(rows), np.arange(len(verts))))   # every vertex is used, none is missing
    out.update(tris=rows.astype(np.int32), tri_cell=keys // 12, tri_tet=tets, cases=seen_cases,
               info=np.array([1, len(verts), len(rows), len(cells)], np.int32))
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def sphere(N, r, centre=None):
    """f = distance - r (in voxels) sampled to float32 in an N^3 volume observed everywhere, centre off the lattice
    -> (tsdf, weight, centre)"""
    c = np.asarray(centre if centre is not None else ((N - 1) / 2 + 0.137, (N - 1) / 2 - 0.211, (N - 1) / 2 + 0.073), np.float64)
    k, j, i = np.meshgrid(*[np.arange(N, dtype=np.float64)] * 3, indexing='ij')
    f = np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - r
    return f.astype(np.float32), np.ones((N, N, N), np.float32), c


def random_volume(dims, seed, holes=0.0):
    """values uniform in [-1, 1) as float32; a share ``holes`` of the voxels unobserved -> (tsdf, weight)"""
    Nx, Ny, Nz = dims
    rng = np.random.default_rng(seed)
    tsdf = rng.uniform(-1, 1, (Nz, Ny, Nx)).astype(np.float32)
    weight = (rng.uniform(0, 1, (Nz, Ny, Nx)) >= holes).astype(np.float32)
    return tsdf, weight


def plane_volume(dims, z0, axis=2):
    """f = z - z0 (in voxels; ``axis`` 0: x - z0) observed everywhere: one plane across an axis -> (tsdf, weight)"""
    Nx, Ny, Nz = dims
    shape = [1, 1, 1]
    shape[2 - axis] = dims[axis]
    f = np.broadcast_to((np.arange(dims[axis], dtype=np.float64) - z0).reshape(shape), (Nz, Ny, Nx))
    return np.ascontiguousarray(f.astype(np.float32)), np.ones((Nz, Ny, Nx), np.float32)


# ---- files ----------------------------------------------------------------------------------------------------------------
def read_ply(path):
    """the file back with numpy, from its own header -> (vertex rows [V, 3 or 6], faces [T, 3])"""
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    lines = raw[:end].decode('ascii').split('\n')
    assert lines[:2] == ['ply', 'format binary_little_endian 1.0']
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith('element')}
    props = [ln.split()[1:] for ln in lines if ln.startswith('property')]
    cols = [p[1] for p in props if p[0] == 'double']
    assert all(p[0] == 'double' for p in props[:-1]) and props[-1] == ['list', 'uchar', 'int', 'vertex_indices']
    v = np.frombuffer(raw, '<f8', counts['vertex'] * len(cols), end).reshape(-1, len(cols))
    f = np.frombuffer(raw, np.dtype([('n', 'u1'), ('v', '<i4', (3,))]), counts['face'], end + v.nbytes)
    assert end + v.nbytes + f.nbytes == len(raw) and (f['n'] == 3).all()
    return cols, v, f['v']
