"""The case table of tests/test_scratch_guard_gpu.py and tests/test_scratch_guard_cpu.py: one ``Entry`` for every entry point of
include/cotr_hip.h that takes ``void* scratch, size_t scratch_bytes`` and no ``cotr_handle`` (the CPU test parses the header and
fails when the two sets differ: an op added later needs a row here - DESIGN.md 3h-13).

A row gives
* ``query``: the op's scratch-size query on a shape;
* ``cases``: the shapes - the smallest that put something on an edge (an empty call, a workgroup or chunk width, a second chunk
  of ``scan_array``, a scratch region that is an exact multiple of 256 bytes so that one element too many leaves the region, a
  capacity at count - 1 / count / count + 1, every optional output NULL and present, mixed item sizes);
* ``build(params)``: the call as a list of arguments in the order of the C prototype - ``In`` (an input array), ``Out`` (an output
  of a type and shape), ``Table`` (an input that holds device addresses of other buffers, the ``Aux`` entries), plain values, ``NULL``, ``SCRATCH``,
  ``SCRATCH_BYTES``, ``STREAM`` - and ``expect(outs, fill)``, which compares the outputs with the numpy float64 restatement of
  that op under tests/, by the rule of the op's own GPU test (bit for bit where that test is, otherwise its tolerance), and
  requires every row the op must not write to hold the fill byte;
* ``early``: the case at which the last region of the op's scratch is written in full, for the early-band control, or the reason
  there is none.

``place`` puts a call into a ``guard_arena.Arena`` on any device: every buffer between two 64 KiB bands at the least alignment
the header documents, scratch of exactly the size queried.  Nothing here needs a GPU; the launch is in the GPU test."""
import collections
import ctypes
import functools

import numpy as np

from tests.guard_arena import Arena, is_fill

In = collections.namedtuple('In', 'name array kind', defaults=(None,))
Out = collections.namedtuple('Out', 'name dtype shape kind', defaults=(None,))
Aux = collections.namedtuple('Aux', 'name array kind', defaults=(None,))  # an input a Table points to: placed, not passed
AuxOut = collections.namedtuple('AuxOut', 'name dtype shape kind', defaults=(None,))  # an output a Table points to: placed, not passed
Table = collections.namedtuple('Table', 'name dtype shape make kind')      # make(addr) with addr(name) -> int: the array
Ref = collections.namedtuple('Ref', 'name offset', defaults=(0,))          # the address of a buffer placed by another argument, + offset bytes
NULL, SCRATCH, SCRATCH_BYTES, STREAM = 'NULL', 'SCRATCH', 'SCRATCH_BYTES', 'STREAM'

Call = collections.namedtuple('Call', 'args expect')
# refusal: 'both' - a scratch one byte short and a scratch 8 bytes off its alignment are each refused; 'align' - only the second (more
# overlap canvases than one: fewer canvases are still a legal scratch); 'none' - the shape returns before the scratch is looked at
Case = collections.namedtuple('Case', 'id params refusal', defaults=('both',))
# carver: the size is a sum of 256-byte regions; min_bytes(params): what the header's text promises at least
Entry = collections.namedtuple('Entry', 'name query cases build carver min_bytes early')

K9 = ctypes.c_double * 9


def size_by_pointer(fn_name, dims):
    """a ``*_scratch_bytes(dims..., size_t* bytes)`` query -> query(lib, params) -> bytes, asserting success; dims(params): its
    leading arguments"""
    def query(lib, params):
        n = ctypes.c_size_t()
        assert getattr(lib, fn_name)(*dims(params), ctypes.byref(n)) == 0, lib.cotr_raster_last_error()
        return n.value
    return query


def place(call, nbytes, device, fill, early_rear_band=0, scratch_shift=0, scratch_bytes=None, early_outputs=None):
    """-> (arena, argv, outs): the call's buffers in a fresh arena and the ctypes arguments; outs: name -> (dtype, shape);
    early_outputs: {output name: bytes by which its rear band starts early} (the control on a buffer that is not ``scratch``)"""
    arena, outs = Arena(device, fill), {}
    early_outputs = early_outputs or {}
    for a in call.args:
        if isinstance(a, (In, Aux)):
            arena.add_input(a.name, a.array, a.kind)
        elif isinstance(a, Table):
            arena.add_input(a.name, np.zeros(a.shape, a.dtype), a.kind)
        elif isinstance(a, (Out, AuxOut)):
            arena.add_output(a.name, a.dtype, a.shape, early_outputs.get(a.name, 0), kind=a.kind)
            outs[a.name] = (np.dtype(a.dtype), tuple(a.shape))
    arena.add('scratch', nbytes, 'scratch', early_rear_band)
    arena.build()
    for a in call.args:
        if isinstance(a, Table):
            arena.set_input(a.name, np.asarray(a.make(arena.addr), dtype=a.dtype).reshape(a.shape))
    argv = []
    for a in call.args:
        if isinstance(a, (Aux, AuxOut)):
            continue
        if isinstance(a, (In, Out, Table)):
            argv.append(arena.ptr(a.name))
        elif isinstance(a, Ref):
            argv.append(ctypes.c_void_p(arena.addr(a.name) + a.offset))
        elif a is NULL or a is STREAM:
            argv.append(None)
        elif a is SCRATCH:
            argv.append(ctypes.c_void_p(arena.addr('scratch') + scratch_shift))
        elif a is SCRATCH_BYTES:
            argv.append(nbytes if scratch_bytes is None else scratch_bytes)
        else:
            argv.append(a)
    return arena, argv, outs


def read_outputs(arena, outs):
    return {name: arena.view(name, dt, shape) for name, (dt, shape) in outs.items()}


def filled(a, fill):
    """every byte of the array is the fill"""
    return bool((np.ascontiguousarray(a).reshape(-1).view(np.uint8) == fill).all())


def same_written_bytes(a, fill_a, b, fill_b, what):
    """two runs' copies of one output: wherever either run wrote (an element that is not its run's fill) the bytes are equal"""
    both_fill = is_fill(a, fill_a) & is_fill(b, fill_b)
    ra = np.ascontiguousarray(a).reshape(-1).view(np.uint8).reshape(a.size, a.dtype.itemsize)
    rb = np.ascontiguousarray(b).reshape(-1).view(np.uint8).reshape(b.size, b.dtype.itemsize)
    differ = (ra != rb).any(axis=1) & ~both_fill.reshape(-1)
    assert not differ.any(), f'{what}: {int(differ.sum())} elements differ between fill 0x{fill_a:02X} and 0x{fill_b:02X}, first at {int(np.flatnonzero(differ)[0])}'


def opt(present, out):
    return out if present else NULL


# ---- cotr_raster_mesh (csrc/triangulate.hip) ---------------------------------------------------------------------------------
# SETUP_THREADS = 256 triangles a workgroup, 16 x 16 pixel tiles; scratch: ids [H W] int, recs [n_tris], local [n_tris] int64,
# bsum [nb + 1] int64 with nb = ceil(n_tris / 256); tri_scan_kernel writes bsum[0 .. nb] in full.
B_PX = 2048.0          # tests/test_triangulate_gpu.py: attribute errors in pixels of a 2048^2 image, at most 1e-3


@functools.lru_cache(maxsize=None)
def _raster_mesh(n_tris, H, W):
    from tests import raster_oracle as ro
    if n_tris == 0:
        z = np.zeros((0, 2), np.float32)
        return z, z, np.zeros((0, 3), np.int32), ro.raster(z, z, np.zeros((0, 3), np.int32), H, W)
    if n_tris == 1:                    # one triangle larger than the canvas
        verts, tris = np.array([[-1.5, -1.2], [3.3, -0.7], [-0.4, 3.9]], np.float32), np.array([[0, 1, 2]], np.int32)
    else:
        nx = int(np.ceil(np.sqrt(n_tris / 2)))
        ny = -(-n_tris // (2 * nx))
        verts, tris = ro.jittered_grid(nx, ny, 0.4, seed=n_tris + H)
        tris = np.ascontiguousarray(np.asarray(tris, np.int32)[:n_tris])
    rng = np.random.default_rng(n_tris)
    attrs = (verts * [0.8, 0.9] + 0.05 + rng.uniform(-0.01, 0.01, verts.shape)).astype(np.float32)
    return verts, attrs, tris, ro.raster(verts, attrs, tris, H, W)


def raster_build(params):
    n_tris, H, W, with_mask = params
    verts, attrs, tris, _ = _raster_mesh(n_tris, H, W)

    def expect(outs, fill):
        ref, ref_mask = _raster_mesh(n_tris, H, W)[3][:2]
        out = outs['out']
        if with_mask:
            assert np.array_equal(outs['mask'].astype(bool), ref_mask) and outs['mask'].max(initial=0) <= 1
        assert (out[~ref_mask] == 0).all()
        if ref_mask.any():
            assert (np.abs(out.astype(np.float64) - ref)[ref_mask] * B_PX).max() <= 1e-3
        assert n_tris == 0 or ref_mask.any()

    return Call([In('verts', verts), len(verts), In('attrs', attrs), In('tris', tris), n_tris, H, W, Out('out', np.float32, (H, W, 2), 'a8'),
                 opt(with_mask, Out('mask', np.uint8, (H, W))), SCRATCH, SCRATCH_BYTES, STREAM], expect)


RASTER = Entry('cotr_raster_mesh', size_by_pointer('cotr_raster_mesh_scratch_bytes', lambda p: p[:3]),
               [Case('empty-1x1', (0, 1, 1, True)), Case('one-triangle-1x1', (1, 1, 1, True)), Case('255-tris-15x17', (255, 15, 17, False)),
                Case('256-tris-16x16-interior-exact', (256, 16, 16, True)), Case('257-tris-17x15', (257, 17, 15, True)),
                Case('7936-tris-last-exact', (7936, 7, 13, False)), Case('65537-tris-second-scan-chunk', (65537, 64, 64, True))],
               raster_build, True, lambda p: 4 * p[1] * p[2] + 8 * p[0] + 8 * (-(-p[0] // 256) + 1), '7936-tris-last-exact')


# ---- cotr_delaunay (csrc/delaunay.hip) ---------------------------------------------------------------------------------------
# DEL_THREADS = 256 (4 points a workgroup in the walk, 256 in the snap); scratch: raw, pts [n] int2, stage [n][DEL_STAGE] int2, cnt,
# off [n] int; del_scan_kernel writes off[0 .. n) in full.  The capacity of tris is 2 n by the header, not the caller's choice.
@functools.lru_cache(maxsize=None)
def _delaunay_points(n):
    from tests import delaunay_oracle as do
    from tests.test_delaunay_cpu import large_lattice
    if n > 300:
        P = large_lattice(n)
        return P, do.triangulate(P, 'int64')
    P = np.random.default_rng(n).uniform(0, 1, (n, 2)).astype(np.float32)
    return P, do.triangulate(P)


def delaunay_build(params):
    n, = params
    P = _delaunay_points(n)[0]

    def expect(outs, fill):
        want, status = _delaunay_points(n)[1]
        count, dev_status = (int(v) for v in outs['info'])
        assert status == 0 and dev_status == 0 and count == len(want) and (n < 3 or count > 0)
        assert np.array_equal(outs['tris'][:count], want) and (outs['tris'][count:] == -1).all()

    return Call([In('verts', P), n, Out('tris', np.int32, (2 * n, 3)), Out('info', np.int32, (2,)), SCRATCH, SCRATCH_BYTES, STREAM], expect)


DELAUNAY = Entry('cotr_delaunay', size_by_pointer('cotr_delaunay_scratch_bytes', lambda p: p),
                 [Case('n0-empty', (0,)), Case('n1', (1,)), Case('n3', (3,)), Case('n63', (63,)), Case('n64-regions-exact', (64,)),
                  Case('n65', (65,)), Case('n255', (255,)), Case('n256', (256,)), Case('n257', (257,)), Case('n1024', (1024,))],
                 delaunay_build, True, lambda p: p[0] * (8 + 8 + 4 + 4), 'n64-regions-exact')


# ---- cotr_nearest_mutual (csrc/guided.hip) -----------------------------------------------------------------------------------
# NN_THREADS = 256 queries a workgroup, keypoint splits of multiples of 64; scratch: pd [parts] double, pj [parts] int with parts =
# splits_ab na + splits_ba nb; nn_partial_kernel writes every (split, query) of both, so pj in full.  Bit for bit.
@functools.lru_cache(maxsize=None)
def _nearest_points(na, nb):
    from tests import guided_oracle as go
    rng = np.random.default_rng(na * 7 + nb)
    kp_a, kp_b = rng.uniform(0, 1000, (na, 2)), rng.uniform(0, 1000, (nb, 2))
    pred_ab, pred_ba = rng.uniform(-20, 1020, (na, 2)), rng.uniform(-20, 1020, (nb, 2))
    ref_ab, ref_ba = go.nearest(pred_ab, kp_b), go.nearest(pred_ba, kp_a)
    return pred_ab, kp_b, pred_ba, kp_a, ref_ab, ref_ba, go.mutual(ref_ab, ref_ba)


def nearest_build(params):
    na, nb = params
    pred_ab, kp_b, pred_ba, kp_a, ref_ab, ref_ba, ref_mutual = _nearest_points(na, nb)

    def expect(outs, fill):
        assert np.array_equal(outs['idx_ab'], ref_ab) and np.array_equal(outs['idx_ba'], ref_ba)
        assert np.array_equal(outs['mutual'], ref_mutual.astype(np.uint8))

    return Call([In('pred_ab', pred_ab), In('kp_b', kp_b), In('pred_ba', pred_ba), In('kp_a', kp_a), na, nb, Out('idx_ab', np.int32, (na,)),
                 Out('idx_ba', np.int32, (nb,)), Out('mutual', np.uint8, (na,)), SCRATCH, SCRATCH_BYTES, STREAM], expect)


NEAREST = Entry('cotr_nearest_mutual', size_by_pointer('cotr_nearest_mutual_scratch_bytes', lambda p: p),
                [Case('1x1', (1, 1)), Case('63x65', (63, 65)), Case('64x64-regions-exact', (64, 64)), Case('255x257', (255, 257)),
                 Case('256x256', (256, 256)), Case('257x255', (257, 255))],
                nearest_build, True, lambda p: 12 * (p[0] + p[1]), '64x64-regions-exact')


# ---- cotr_tsdf_mesh (csrc/tsdf.hip) ------------------------------------------------------------------------------------------
# MS_BLOCK = 512 voxels a block; ms_scan_kernel takes 1024 block totals a chunk; scratch: code [voxels] uint16, rec [voxels] uint32,
# totals, bases [blocks] int2 - "6 a voxel"; ms_scan_kernel writes bases[0 .. blocks) in full.  Bit for bit (NaN where the
# restatement has NaN).  params: dims, volume ('random' with 4 % holes, or 'plane': one plane across x), capacities as offsets from
# the counts (None: capacity 0), normals present, found (None: NULL).
@functools.lru_cache(maxsize=None)
def _mesh_volume(dims, kind):
    from tests import mesh_oracle as mo
    tsdf, weight = mo.random_volume(dims, 11, 0.04) if kind == 'random' else mo.plane_volume(dims, dims[0] / 2 - 0.3, axis=0)
    return tsdf, weight, mo.mesh(tsdf, weight, MESH_ORIGIN, MESH_VOXEL, normals=True)


MESH_ORIGIN, MESH_VOXEL = (0.31, -1.27, 2.05), 0.05


def mesh_build(params):
    dims, kind, dv, dt, normals, found = params
    tsdf, weight, o = _mesh_volume(dims, kind)
    V, T = int(o['info'][1]), int(o['info'][2])
    cv, ct = (0 if dv is None else max(V + dv, 0)), (0 if dt is None else max(T + dt, 0))
    normals = normals and cv > 0
    origin = (ctypes.c_double * 3)(*MESH_ORIGIN)

    def expect(outs, fill):
        if found == 0:
            assert outs['info'].tolist() == [0, 0, 0, 0] and (ct == 0 or (outs['tris'] == -1).all())
            assert (cv == 0 or filled(outs['verts'], fill)) and (not normals or filled(outs['normals'], fill))
            return
        assert outs['info'].tolist() == o['info'].tolist() and V > 0 and T > 0
        nv, nt = min(V, cv), min(T, ct)
        if cv:
            assert np.array_equal(outs['verts'][:nv], o['verts'][:nv]) and filled(outs['verts'][nv:], fill)
        if ct:
            assert np.array_equal(outs['tris'][:nt], o['tris'][:nt]) and (outs['tris'][nt:] == -1).all()
        if normals:
            assert np.array_equal(outs['normals'][:nv], o['normals'][:nv], equal_nan=True) and filled(outs['normals'][nv:], fill)

    found_arg = NULL if found is None else In('found', np.array([found], np.int32))
    return Call([In('tsdf', tsdf), In('weight', weight), dims[0], dims[1], dims[2], origin, MESH_VOXEL, found_arg,
                 opt(cv > 0, Out('verts', np.float64, (cv, 3))), cv, opt(normals, Out('normals', np.float64, (cv, 3))),
                 opt(ct > 0, Out('tris', np.int32, (ct, 3))), ct, Out('info', np.int32, (4,)), SCRATCH, SCRATCH_BYTES, STREAM], expect)


def _mesh_id(p):
    dims, kind, dv, dt, normals, found = p
    cap = 'count-only' if dv is None and dt is None else f'cap{dv:+d}' if dv == dt else f'capv{dv}-capt{dt}'
    return f'{dims[0]}x{dims[1]}x{dims[2]}-{kind}-{cap}' + ('-normals' if normals else '') + ('' if found is None else f'-found{found}')


TSDF_MESH = Entry('cotr_tsdf_mesh', size_by_pointer('cotr_tsdf_mesh_scratch_bytes', lambda p: p[0]),
                  [Case(_mesh_id(p), p) for p in [
                      ((2, 2, 2), 'random', 0, 0, True, None), ((2, 3, 85), 'random', 0, 0, True, None), ((8, 8, 8), 'random', 0, 0, False, None),
                      ((3, 9, 19), 'random', 0, 0, True, 1), ((4, 4, 4), 'random', None, None, False, None), ((4, 4, 4), 'random', -1, -1, True, None),
                      ((4, 4, 4), 'random', 1, 1, True, None), ((4, 4, 4), 'random', None, 0, False, None), ((4, 4, 4), 'random', 0, None, True, None),
                      ((4, 4, 4), 'random', 0, 0, True, 0), ((32, 32, 16), 'plane', 0, 0, True, None), ((128, 64, 64), 'plane', 0, 0, False, None),
                      ((128, 64, 65), 'plane', 0, 0, False, None)]],
                  mesh_build, True, lambda p: 6 * p[0][0] * p[0][1] * p[0][2], _mesh_id(((32, 32, 16), 'plane', 0, 0, True, None)))


# ---- cotr_depth_corrs / cotr_depth_valid (csrc/reproject.hip) ----------------------------------------------------------------
# RP_THREADS = 256 source pixels a block, one scan_array walk of an item's block totals in chunks of 256; scratch: ballots
# [n][nb][4] uint64 then offsets [n][nb] int32 with nb = ceil(max_src / 256), the sum rounded up to 16 bytes (the header's rule;
# no 256-byte regions).  reproj_scan_kernel writes the offsets of every block below an item's own block count, so the last
# region is written in full when the last item has max_src pixels.
# params: the items as (seed, H, W, subset length or None), the capacity as an offset from the largest count (None: 0).
MARGIN, TOL, MAX_AMBIGUOUS = 1e-9, 1e-9, 1e-4           # tests/test_dataset_gpu.py


@functools.lru_cache(maxsize=None)
def _depth_items(items):
    from cotr_amd.data import _cam_rows
    from cotr_amd.utils.synth import synth_captures
    from tests import dataset_oracle as oracle
    out = []
    for k, (seed, H, W, n_sub) in enumerate(items):
        q, n = synth_captures(seed, H, W)
        f, t = (q, n) if k % 2 == 0 else (n, q)
        subset = None if n_sub is None else (np.arange(n_sub, dtype=np.int64) * 7 % (H * W)).astype(np.int32)
        r = oracle.reproject(f.depth, t.depth, f.K, f.c2w, t.K, t.c2w, subset=subset)
        out.append(dict(f=f, t=t, subset=subset, cams=_cam_rows(f, t), ref=r, n_src=H * W if n_sub is None else n_sub))
    return out


def _depth_tables(items):
    n = len(items)

    def ptrs(addr):
        return [[addr(f'from{i}'), addr(f'to{i}'), addr(f'subset{i}') if it['subset'] is not None else 0] for i, it in enumerate(items)]
    shapes = np.array([[*it['f'].depth.shape, *it['t'].depth.shape, it['n_src']] for it in items], np.int32).reshape(n, 5)
    bufs = []
    for i, it in enumerate(items):
        bufs += [Aux(f'from{i}', it['f'].depth), Aux(f'to{i}', it['t'].depth)]
        if it['subset'] is not None:
            bufs.append(Aux(f'subset{i}', it['subset']))
    return Table('ptrs', np.uint64, (n, 3), ptrs, 'a8'), In('shapes', shapes), bufs


def _check_corr_rows(rows, count, cap, it, fill):
    """tests/test_dataset_gpu.py::_compare with the fill in the place of its zeros"""
    r, W = it['ref'], it['f'].depth.shape[1]
    ambiguous = r['margin'] < MARGIN
    assert (ambiguous.mean() if ambiguous.size else 0.0) <= MAX_AMBIGUOUS
    amb_px = np.unique(r['index'][ambiguous])
    clear = r['keep'] & ~ambiguous
    want_px, want_uv = r['index'][clear], r['uv'][clear]
    written = min(count, cap)
    got = rows[:written]
    got_px = (got[:, 1] * W + got[:, 0]).astype(np.int64)
    assert np.array_equal(got[:, 0], np.floor(got[:, 0])) and np.array_equal(got[:, 1], np.floor(got[:, 1]))
    sel = ~np.isin(got_px, amb_px)
    got_px, got_uv = got_px[sel], got[sel, 2:]
    if count > cap:
        want_px, want_uv = want_px[:len(got_px)], want_uv[:len(got_px)]
        assert not amb_px.size or it['subset'] is None
    elif not amb_px.size:
        assert count == len(want_px)
    assert np.array_equal(got_px, want_px)
    if len(want_px):
        assert np.abs(got_uv - want_uv).max() <= TOL
    assert filled(rows[written:], fill)             # counted, not written; rows past the count are left alone


def _depth_cap(items, dcap, counts):
    return 0 if dcap is None else max(max(counts) + dcap, 0)


def corrs_build(params):
    spec, dcap = params
    items = _depth_items(spec)
    n = len(items)
    max_src = max([it['n_src'] for it in items] or [1])
    want_counts = [int(it['ref']['keep'].sum()) for it in items]
    cap = _depth_cap(items, dcap, want_counts or [0])
    ptrs, shapes, bufs = _depth_tables(items)

    def expect(outs, fill):
        if n == 0:
            assert filled(outs['rows'], fill) and filled(outs['counts'], fill)
            return
        assert max(want_counts) > 0 or max_src < 255
        for i, it in enumerate(items):
            if not (it['ref']['margin'] < MARGIN).any():
                assert int(outs['counts'][i]) == want_counts[i]
            if cap:
                _check_corr_rows(outs['rows'][i], int(outs['counts'][i]), cap, it, fill)

    cams = np.stack([it['cams'] for it in items]) if n else np.zeros((0, 37))
    return Call(bufs + [ptrs, shapes, In('cams', cams), n, max_src, opt(cap > 0 or n == 0, Out('rows', np.float64, (n, cap, 4), 'a16')), cap,
                        Out('counts', np.int32, (max(n, 1),)), SCRATCH, SCRATCH_BYTES, STREAM], expect)


def valid_build(params):
    spec, dcap = params
    items = _depth_items(spec)
    n = len(items)
    max_src = max([it['n_src'] for it in items] or [1])
    want = []
    for it in items:
        d = it['f'].depth.reshape(-1)
        src = np.arange(d.size) if it['subset'] is None else it['subset'].astype(np.int64)
        want.append(src[d[src] > 0].astype(np.int32))
    cap = _depth_cap(items, dcap, [len(w) for w in want] or [0])
    ptrs, shapes, bufs = _depth_tables(items)

    def expect(outs, fill):
        if n == 0:
            assert filled(outs['indices'], fill) and filled(outs['counts'], fill)
            return
        assert max(len(w) for w in want) > 0 or max_src < 255
        for i, w in enumerate(want):
            assert int(outs['counts'][i]) == len(w)
            if cap:
                k = min(len(w), cap)
                assert np.array_equal(outs['indices'][i, :k], w[:k]) and filled(outs['indices'][i, k:], fill)

    return Call(bufs + [ptrs, shapes, n, max_src, opt(cap > 0 or n == 0, Out('indices', np.int32, (n, cap))), cap,
                        Out('counts', np.int32, (max(n, 1),)), SCRATCH, SCRATCH_BYTES, STREAM], expect)


def _depth_query(lib, params):
    spec, _ = params
    return lib.cotr_depth_corrs_scratch(len(spec), max([(H * W if s is None else s) for _, H, W, s in spec] or [1]))


def _depth_min_bytes(params):
    spec, _ = params
    blocks = len(spec) * -(-max([(H * W if s is None else s) for _, H, W, s in spec] or [1]) // 256)
    return -(-blocks * 36 // 16) * 16


WIDTHS = ((3, 15, 17, None), (4, 16, 16, None), (5, 1, 257, None), (6, 1, 1, None))         # 255, 256, 257 pixels and 1: mixed sizes
DEPTH_CASES = [Case('no-items', ((), 0), 'none'), Case('one-pixel', (((6, 1, 1, None),), 0)), Case('mixed-255-256-257-1-cap-count', (WIDTHS, 0)),
               Case('mixed-cap-0', (WIDTHS, None)), Case('mixed-cap-count-1', (WIDTHS, -1)), Case('mixed-cap-count+1', (WIDTHS, 1)),
               Case('65537-subset-beside-one-pixel', (((7, 256, 256, 65537), (6, 1, 1, None)), 0)),
               Case('two-64x128-last-exact', (((8, 64, 128, None), (9, 64, 128, None)), 0))]
DEPTH_CORRS = Entry('cotr_depth_corrs', _depth_query, DEPTH_CASES, corrs_build, False, _depth_min_bytes, 'two-64x128-last-exact')
DEPTH_VALID = Entry('cotr_depth_valid', _depth_query, DEPTH_CASES, valid_build, False, _depth_min_bytes, 'two-64x128-last-exact')


# ---- cotr_overlap_pairs (csrc/overlap.hip) -----------------------------------------------------------------------------------
# OV_THREADS = 256 pixels a block; scratch: as many canvases of max_px uint32, each rounded up to 16 bytes, as the caller gives
# (the header's rule); every canvas of a tile is cleared before it is used, so the last one is written in full whenever the
# number of pairs is a multiple of the canvases.  The rule of tests/test_scene_gpu.py: counts equal and ratios bit-equal for every
# pair without a candidate within 1e-9 of a decision, and the scenes have none.
# params: scene key, the pairs ('all' or a tuple of (q, d)), canvases in flight.
@functools.lru_cache(maxsize=None)
def _overlap_scene(key, pairs):
    from cotr_amd.utils.synth import synth_scene
    from tests import scene_oracle as so
    if key == 'mixed':
        a, b = synth_scene(30, 4, 64, 96), synth_scene(30, 4, 48, 64)
        caps = [a[0], b[1], a[2], b[3]]
    else:
        seed, h, w = key
        caps = synth_scene(seed, 3 if h * w == 1 else 4, h, w)
    n = len(caps)
    pairs = np.argwhere(np.ones((n, n), dtype=bool)).astype(np.int32) if pairs == 'all' else np.array(pairs, np.int32).reshape(-1, 2)
    ratio, counts, ambiguous = so.overlap_pairs(caps, pairs) if len(pairs) else (np.zeros(0, np.float32), np.zeros((0, 2), np.int64), np.zeros(0))
    ties = sum(so.float32_ties(caps[d]) for d in set(pairs[:, 1].tolist()))
    xyz = [so.world_points(c)[0] for c in caps]
    return caps, pairs, xyz, ratio, counts, ambiguous, ties


def overlap_build(params):
    key, pair_spec, in_flight = params
    caps, pairs, xyz, want_ratio, want_counts, ambiguous, ties = _overlap_scene(key, pair_spec)
    n, n_pairs = len(caps), len(pairs)
    max_px = max(c.depth.size for c in caps)
    proj = np.stack([np.matmul(np.asarray(c.K), np.linalg.inv(np.asarray(c.c2w))[0:3, :]).ravel() for c in caps])
    shapes = np.array([c.depth.shape for c in caps], np.int32)

    def expect(outs, fill):
        assert ties == 0 and not ambiguous.any()
        assert np.array_equal(outs['counts'], want_counts.astype(np.int32))
        assert np.array_equal(outs['ratio'].view(np.uint32), want_ratio.view(np.uint32))

    bufs = [Aux(f'depth{i}', c.depth) for i, c in enumerate(caps)] + [Aux(f'xyz{i}', x.astype(np.float32)) for i, x in enumerate(xyz)]
    table = Table('caps', np.uint64, (n, 2), lambda addr: [[addr(f'depth{i}'), addr(f'xyz{i}')] for i in range(n)], 'a8')
    return Call(bufs + [table, In('shapes', shapes), In('proj', proj), n, In('pairs', pairs), n_pairs, max_px, Out('ratio', np.float32, (n_pairs,)),
                        Out('counts', np.int32, (n_pairs, 2)), SCRATCH, SCRATCH_BYTES, STREAM], expect)


def _overlap_query(lib, params):
    key, _, in_flight = params
    max_px = 64 * 96 if key == 'mixed' else key[1] * key[2]
    return lib.cotr_overlap_scratch(in_flight, max_px)


def _overlap_min_bytes(params):
    key, _, in_flight = params
    max_px = 64 * 96 if key == 'mixed' else key[1] * key[2]
    return in_flight * (-(-max_px * 4 // 16) * 16)


def _ov(id_, params):
    return Case(id_, params, 'both' if params[2] == 1 else 'align')


OVERLAP = Entry('cotr_overlap_pairs', _overlap_query,
                [Case('no-pairs', ((30, 17, 23), (), 1), 'none'), _ov('1x1-all-pairs', ((30, 1, 1), 'all', 9)), _ov('2x3-all-pairs', ((33, 2, 3), 'all', 16)),
                 _ov('17x23-one-canvas-16-pairs', ((30, 17, 23), 'all', 1)), _ov('17x23-three-canvases-ragged-tile', ((30, 17, 23), 'all', 3)),
                 _ov('13x20-260-pixels-four-canvases', ((30, 13, 20), 'all', 4)), _ov('15x17-255-pixels', ((30, 15, 17), 'all', 2)),
                 _ov('16x16-256-pixels', ((30, 16, 16), 'all', 5)), _ov('257x1-257-pixels', ((31, 257, 1), 'all', 16)), _ov('mixed-64x96-and-48x64', ('mixed', 'all', 16))],
                overlap_build, False, _overlap_min_bytes, '17x23-one-canvas-16-pairs')


# ---- the five RANSAC estimators (csrc/ransac.h: guided.hip, homography.hip, essential.hip, pnp.hip, rigid3d.hip) -------------
# RS_SOLVE_THREADS = 64 iterations a workgroup, RS_CHUNK = 2048 points a workgroup of the count, mask and refit passes; scratch:
# candidates [slots][9] double, counts [slots] int, then the estimator's own regions.  Scenes are (n, outliers, noise, threshold,
# confidence, max_iters <= 64, seed), those of the oracles' EDGES lists.  The rule of each estimator's own GPU test on the
# wavefront, chunk and workgroup edges: the samples are the restatement's; the counts, the selection, the chosen model and the
# mask are exact on the device's own candidates; a refit is the restatement's refit on the device's mask within that test's
# bound.  With the optional tables NULL the other outputs must be the bytes of the run with them (``twin``).
def _ransac_common(outs, twin, names):
    if twin is not None:
        for k in names:
            assert outs[k].tobytes() == twin[k].tobytes(), k


def _hyp(present, name, dtype, shape):
    return opt(present, Out(name, dtype, shape))


@functools.lru_cache(maxsize=None)
def _fm_scene(n, outl, seed):
    from tests import guided_oracle as go
    return go.two_view_scene(n, outl, seed)[:2]


def fundamental_build(params):
    from tests import guided_oracle as go
    (n, outl, thr, conf, iters, seed), hyp = params
    p1, p2 = _fm_scene(n, outl, seed)

    def expect(outs, fill, twin=None):
        if not hyp:
            return _ransac_common(outs, twin, ('F', 'mask', 'info'))
        assert np.array_equal(outs['samples'], go.samples(n, iters, seed))
        dev_H = outs['hyp_F']
        cnt = go.counts(dev_H, p1, p2, thr)
        assert np.array_equal(outs['hyp_count'], cnt) and np.array_equal(np.isnan(dev_H).all(axis=1), cnt < 0)
        info = tuple(int(v) for v in outs['info'])
        assert info == go.select(cnt, iters, n, conf) == go.select_sequential(cnt, iters, n, conf)
        found, best, runs, slot = info
        assert np.array_equal(outs['F'], dev_H[slot] if found else np.zeros(9))
        want = go.inliers(dev_H[slot], p1, p2, thr)[0] if found else np.zeros(n, bool)
        assert np.array_equal(outs['mask'].astype(bool), want) and outs['mask'].sum() == best and outs['mask'].max() <= 1

    return Call([In('pts1', p1), In('pts2', p2), n, float(thr), float(conf), iters, ctypes.c_uint64(seed), Out('F', np.float64, (9,)),
                 Out('mask', np.uint8, (n,)), Out('info', np.int32, (4,)), _hyp(hyp, 'hyp_F', np.float64, (3 * iters, 9)),
                 _hyp(hyp, 'hyp_count', np.int32, (3 * iters,)), _hyp(hyp, 'samples', np.int32, (iters, 7)), SCRATCH, SCRATCH_BYTES, STREAM], expect)


def _rs_cases(scenes, exact=None):
    """every scene with the hypothesis tables, the last one also without"""
    out = [Case(f'n{s[0]}-it{s[-2]}' + ('-regions-exact' if s == exact else ''), (s, True)) for s in scenes]
    return out + [Case(f'n{scenes[-1][0]}-it{scenes[-1][-2]}-no-tables', (scenes[-1], False))]


def _rs_twin(params):
    """the params of the run whose bytes a run without tables must reproduce"""
    return None if params[-1] else params[:-1] + (True,)


def _rs_dims(p):
    return p[0][0], p[0][-2]


FM_EXACT = (63, 0.3, 3.0, 0.99, 64, 0)     # 192 slots: candidates 54 x 256 bytes, counts 3 x 256
FUNDAMENTAL = Entry('cotr_ransac_fundamental', size_by_pointer('cotr_ransac_fundamental_scratch_bytes', _rs_dims),
                    _rs_cases([(15, 0.0, 3.0, 0.99, 1, 0), FM_EXACT, (2047, 0.4, 3.0, 0.99, 63, 0), (2048, 0.4, 3.0, 0.99, 64, 0),
                               (2049, 0.4, 3.0, 0.99, 64, 0)], FM_EXACT),
                    fundamental_build, True, lambda p: 3 * p[0][-2] * 76, 'n63-it64-regions-exact')


@functools.lru_cache(maxsize=None)
def _hg_scene(n, outl, seed, noise):
    from tests import homography_oracle as ho
    return ho.planar_scene(n, outl, seed, noise)[:2]


def homography_build(params):
    from tests import homography_oracle as ho
    (n, outl, noise, thr, conf, iters, seed), hyp = params
    p1, p2 = _hg_scene(n, outl, seed, noise)

    def expect(outs, fill, twin=None):
        if not hyp:
            return _ransac_common(outs, twin, ('H', 'mask', 'info'))
        assert np.array_equal(outs['samples'], ho.samples(n, iters, seed))
        dev_H, na = outs['hyp_H'], outs['hyp_count'] < 0
        assert np.array_equal(np.isnan(dev_H).all(axis=1), na) and np.isfinite(dev_H[~na]).all()
        cnt = ho.counts(dev_H, ~na, p1, p2, thr)
        assert np.array_equal(outs['hyp_count'], cnt)
        info = [int(v) for v in outs['info']]
        assert tuple(info[:4]) == ho.select(cnt, iters, n, conf) == ho.select_sequential(cnt, iters, n, conf)
        found, best, runs, slot, kept, status = info[:6]
        assert found and best >= 4 and info[6:] == [0, 0]
        assert np.array_equal(outs['H_ransac'], dev_H[slot])
        mask = outs['mask'].astype(bool)
        assert mask.sum() == best and outs['mask'].max() <= 1 and np.array_equal(mask, ho.inliers(dev_H[slot], p1, p2, thr)[0])
        ref, ref_kept, ref_status, _ = ho.refit(p1, p2, mask, 10, dev_H[slot])
        assert status == ref_status == 0 and 0 <= kept <= 10
        assert ho.corner_error(outs['H'], ref, p1) <= ho.REFIT_BOUND_PX

    return Call([In('pts1', p1), In('pts2', p2), n, float(thr), float(conf), iters, 10, ctypes.c_uint64(seed), Out('H', np.float64, (9,)),
                 Out('mask', np.uint8, (n,)), Out('info', np.int32, (8,)), _hyp(hyp, 'H_ransac', np.float64, (9,)),
                 _hyp(hyp, 'hyp_H', np.float64, (iters, 9)), _hyp(hyp, 'hyp_count', np.int32, (iters,)), _hyp(hyp, 'samples', np.int32, (iters, 4)),
                 SCRATCH, SCRATCH_BYTES, STREAM], expect)


# the last region, the refit's per-chunk sums [chunks][45] double, is a multiple of 256 bytes only at 32 chunks: n = 65536
HG_EXACT = (65536, 0.3, 0.5, 3.0, 0.995, 32, 3)
HOMOGRAPHY = Entry('cotr_ransac_homography', size_by_pointer('cotr_ransac_homography_scratch_bytes', _rs_dims),
                   _rs_cases([(4, 0.0, 0.5, 3.0, 0.995, 1, 1), (63, 0.3, 0.5, 3.0, 0.995, 64, 4), (2047, 0.4, 0.5, 3.0, 0.995, 63, 2),
                              (2048, 0.4, 0.5, 3.0, 0.995, 64, 1), HG_EXACT, (2049, 0.4, 1.0, 3.0, 0.995, 64, 1)], HG_EXACT),
                   homography_build, True, lambda p: p[0][-2] * 76 + -(-p[0][0] // 2048) * 45 * 8, 'n65536-it32-regions-exact')


@functools.lru_cache(maxsize=None)
def _es_scene(n, outl, seed, noise):
    from tests import essential_oracle as eo
    p1, p2, K1, K2 = eo.two_view_scene(n, outl, seed, noise)[:4]
    return p1, p2, K1, K2, eo.normalise(p1, K1), eo.normalise(p2, K2)


def essential_build(params):
    from tests import essential_oracle as eo
    (n, outl, noise, thr, conf, iters, seed), hyp = params
    p1, p2, K1, K2, xn1, xn2 = _es_scene(n, outl, seed, noise)
    sthr = eo.scaled_threshold(thr, K1, K2)

    def expect(outs, fill, twin=None):
        if not hyp:
            return _ransac_common(outs, twin, ('E', 'mask', 'info'))
        assert np.array_equal(outs['samples'], eo.samples(n, iters, seed))
        dev_E, cnt = outs['hyp_E'], outs['hyp_count']
        used = cnt >= 0
        assert np.array_equal(used, eo.slots_used(used.reshape(iters, 10).sum(axis=1)))
        assert np.isnan(dev_E[~used]).all() and np.isfinite(dev_E[used]).all()
        assert np.array_equal(cnt, eo.counts(dev_E, used, xn1, xn2, sthr))
        info = [int(v) for v in outs['info']]
        assert tuple(info[:4]) == eo.select(cnt, iters, n, conf) == eo.select_sequential(cnt, iters, n, conf)
        found, best, runs, slot = info[:4]
        assert found and best >= 5 and info[4:] == [0, 0, 0, 0]
        assert np.array_equal(outs['E'], dev_E[slot])
        mask = outs['mask'].astype(bool)
        assert mask.sum() == best and outs['mask'].max() <= 1 and np.array_equal(mask, eo.inliers(outs['E'], xn1, xn2, sthr)[0])

    return Call([In('pts1', p1.astype(np.float64)), In('pts2', p2.astype(np.float64)), n, K9(*K1.reshape(9)), K9(*K2.reshape(9)), float(thr), float(conf),
                 iters, ctypes.c_uint64(seed), Out('E', np.float64, (9,)), Out('mask', np.uint8, (n,)), Out('info', np.int32, (8,)),
                 _hyp(hyp, 'hyp_E', np.float64, (10 * iters, 9)), _hyp(hyp, 'hyp_count', np.int32, (10 * iters,)),
                 _hyp(hyp, 'samples', np.int32, (iters, 5)), SCRATCH, SCRATCH_BYTES, STREAM], expect)


# the last region, the normalised pairs [n][4] double, is a multiple of 256 bytes when n is one of 8: n = 64, and 32 iterations make
# the candidates (320 x 72) and the counts (320 x 4) whole regions too
ES_EXACT = (64, 0.3, 1.0, 1.0, 0.999, 32, 3)
ESSENTIAL = Entry('cotr_ransac_essential', size_by_pointer('cotr_ransac_essential_scratch_bytes', _rs_dims),
                  _rs_cases([(5, 0.0, 0.0, 1.0, 0.999, 1, 0), (63, 0.3, 1.0, 1.0, 0.999, 32, 2), ES_EXACT, (2047, 0.4, 1.0, 1.0, 0.999, 64, 5),
                             (2048, 0.4, 0.5, 1.0, 0.999, 64, 6), (2049, 0.4, 1.0, 1.0, 0.999, 63, 7)], ES_EXACT),
                  essential_build, True, lambda p: 10 * p[0][-2] * 76 + p[0][0] * 32, 'n64-it32-regions-exact')


@functools.lru_cache(maxsize=None)
def _pn_scene(n, outl, seed, noise):
    from tests import pnp_oracle as po
    return po.pnp_scene(n, outl, seed, noise)[:3]


def pnp_build(params):
    from tests import pnp_oracle as po
    (n, outl, noise, thr, conf, iters, seed), hyp = params
    obj, img, K = _pn_scene(n, outl, seed, noise)

    def expect(outs, fill, twin=None):
        if not hyp:
            return _ransac_common(outs, twin, ('R', 't', 'mask', 'info'))
        assert np.array_equal(outs['samples'], po.samples(n, iters, seed))
        dev, cnt = outs['hyp_pose'], outs['hyp_count']
        has = cnt >= 0
        assert np.isnan(dev[~has]).all() and np.isfinite(dev[has]).all()
        assert np.array_equal(cnt, po.counts(dev, has, obj, img, K, thr))
        info = [int(v) for v in outs['info']]
        assert tuple(info[:4]) == po.select(cnt, iters, n, conf) == po.select_sequential(cnt, iters, n, conf)
        found, best, runs, slot = info[:4]
        assert found and best >= 4 and info[5:] == [0, 0, 0] and 0 <= info[4] <= 10
        R0, t0 = po.expand(dev[slot])
        mask = outs['mask'].astype(bool)
        assert mask.sum() == best and outs['mask'].max() <= 1 and np.array_equal(mask, po.inliers(dev[slot], obj, img, K, thr)[0])
        Rr, tr, kept, margin = po.refit(obj, img, mask, K, R0, t0, 10)
        R, t = outs['R'].reshape(3, 3), outs['t']
        assert np.abs(R - Rr).max() <= po.REFIT_BOUND and np.abs(t - tr).max() / np.linalg.norm(tr) <= po.REFIT_BOUND
        if margin > 1e-6:
            assert info[4] == kept

    return Call([In('obj', obj), In('img', img.astype(np.float64)), n, K9(*np.asarray(K, np.float64).reshape(9)), float(thr), float(conf), iters,
                 ctypes.c_uint64(seed), 10, Out('R', np.float64, (9,)), Out('t', np.float64, (3,)), Out('mask', np.uint8, (n,)),
                 Out('info', np.int32, (8,)), _hyp(hyp, 'hyp_pose', np.float64, (iters, 9)), _hyp(hyp, 'hyp_count', np.int32, (iters,)),
                 _hyp(hyp, 'samples', np.int32, (iters, 4)), SCRATCH, SCRATCH_BYTES, STREAM], expect)


# the last region, the refit's per-chunk sums [chunks][29] double, is a multiple of 256 bytes only at 32 chunks: n = 65536
PN_EXACT = (65536, 0.3, 1.0, 4.0, 0.99, 32, 3)
PNP = Entry('cotr_ransac_pnp', size_by_pointer('cotr_ransac_pnp_scratch_bytes', _rs_dims),
            _rs_cases([(4, 0.0, 0.0, 2.0, 0.99, 64, 0), (63, 0.3, 1.0, 4.0, 0.99, 63, 2), (2047, 0.4, 1.0, 4.0, 0.99, 64, 8),
                       (2048, 0.4, 0.5, 4.0, 0.99, 64, 9), PN_EXACT, (2049, 0.4, 1.0, 4.0, 0.99, 63, (1 << 63) + 10)], PN_EXACT),
            pnp_build, True, lambda p: p[0][-2] * 76 + -(-p[0][0] // 2048) * 29 * 8, 'n65536-it32-regions-exact')


@functools.lru_cache(maxsize=None)
def _rg_scene(n, outl, seed, noise, ws):
    from tests import rigid3d_oracle as r3
    return r3.rigid_scene(n, outl, seed, noise, ws)[:2]


def rigid3d_build(params):
    from tests import rigid3d_oracle as r3
    (n, outl, noise, thr, conf, iters, seed), ws, hyp, rounds = params
    src, dst = _rg_scene(n, outl, seed, noise, ws)

    def expect(outs, fill, twin=None):
        if not hyp:
            return _ransac_common(outs, twin, ('R', 't', 'scale', 'mask', 'info'))
        assert np.array_equal(outs['samples'], r3.samples(n, iters, seed))
        dev, cnt = outs['hyp_model'], outs['hyp_count']
        has = cnt >= 0
        assert np.isnan(dev[~has]).all() and np.isfinite(dev[has]).all()
        assert np.array_equal(cnt, r3.counts(dev, has, src, dst, thr, ws))
        info = [int(v) for v in outs['info']]
        assert tuple(info[:4]) == r3.select(cnt, iters, n, conf) == r3.select_sequential(cnt, iters, n, conf)
        found, best, runs, slot = info[:4]
        mask = r3.inliers(dev[slot], src, dst, thr, ws)[0]
        assert found and best >= 3 and mask.sum() == best
        if rounds == 2:         # the second round fits on the re-count of the device's own model after one round: the twin's outputs
            for k in ('hyp_model', 'hyp_count', 'samples'):
                assert outs[k].tobytes() == twin[k].tobytes(), k
            mask = r3.model_inliers(twin['scale'][0] * twin['R'].reshape(3, 3), twin['t'], src, dst, thr)[0]
        assert info[4:] == [rounds, int(mask.sum()), 0, 0]
        assert np.array_equal(outs['mask'].astype(bool), mask) and outs['mask'].max() <= 1
        sRf, tf, sf, _ = r3.fit(src, dst, mask, ws)
        s = outs['scale'][0]
        assert r3.model_distance(s * outs['R'].reshape(3, 3), outs['t'], sRf, tf) <= r3.REFIT_BOUND and abs(s - sf) <= r3.REFIT_BOUND * sf
        assert ws or s == 1.0

    return Call([In('src', src), In('dst', dst), n, float(thr), float(conf), iters, ctypes.c_uint64(seed), int(ws), rounds, Out('R', np.float64, (9,)),
                 Out('t', np.float64, (3,)), Out('scale', np.float64, (1,)), Out('mask', np.uint8, (n,)), Out('info', np.int32, (8,)),
                 _hyp(hyp, 'hyp_model', np.float64, (iters, 9)), _hyp(hyp, 'hyp_count', np.int32, (iters,)), _hyp(hyp, 'samples', np.int32, (iters, 3)),
                 SCRATCH, SCRATCH_BYTES, STREAM], expect)


def _rg_twin(params):
    scene, ws, hyp, rounds = params
    return (scene, ws, True, rounds) if not hyp else (scene, ws, True, 1) if rounds == 2 else None


# the last region, the re-count's work mask [n] uint8, is a multiple of 256 bytes at n = 256; rg_mask_kernel writes it in full from the
# second refit round on
RG_SCENES = [((3, 0.0, 0.0, 0.02, 0.99, 64, 0), False), ((255, 0.4, 0.01, 0.04, 0.99, 63, 5), True), ((256, 0.2, 0.01, 0.04, 0.99, 64, 6), False),
             ((2047, 0.4, 0.01, 0.04, 0.99, 64, 8), True), ((2048, 0.4, 0.005, 0.04, 0.99, 64, 9), False),
             ((2049, 0.4, 0.01, 0.04, 0.99, 63, (1 << 63) + 10), True)]
RIGID3D = Entry('cotr_ransac_rigid3d', size_by_pointer('cotr_ransac_rigid3d_scratch_bytes', _rs_dims),
                [Case(f'n{s[0]}-it{s[-2]}-{"similarity" if ws else "rigid"}', (s, ws, True, 1)) for s, ws in RG_SCENES] +
                [Case('n256-it64-rigid-two-rounds-regions-exact', (RG_SCENES[2][0], False, True, 2)),
                 Case('n2049-it63-similarity-no-tables', (RG_SCENES[-1][0], True, False, 1))],
                rigid3d_build, True, lambda p: p[0][-2] * 76 + -(-p[0][0] // 2048) * 11 * 8 + p[0][0], 'n256-it64-rigid-two-rounds-regions-exact')


# ---- cotr_recover_pose (csrc/essential.hip) ------------------------------------------------------------------------------------
# RS_CHUNK = 2048 points a workgroup of the counting pass, 256 of the mask pass; scratch: one EsPose of 188 bytes in one 256-byte
# region.  E and the inlier mask are the restatement's RANSAC result on the scene; the rule of tests/test_essential_gpu.py: info
# and the mask exactly, R and t within 1e-9, on scenes where no depth comes within 1e-9 of a limit.
# params: scene, mask_in present, found (None: NULL).
@functools.lru_cache(maxsize=None)
def _pose_case(scene, masked):
    from tests import essential_oracle as eo
    ref = eo.reference(scene)
    E, mask = ref['ransac']['E'].reshape(9), ref['ransac']['mask']
    assert ref['ransac']['info'][0]
    want = eo.recover_pose(E, ref['p1'], ref['p2'], ref['K1'], ref['K2'], mask if masked else None)
    return ref, E, mask, want


def recover_build(params):
    scene, masked, found = params
    ref, E, mask, want = _pose_case(scene, masked)
    n = scene[0]

    def expect(outs, fill, twin=None):
        if found == 0:
            assert outs['info'].tolist() == [0, -1, 0, 0, 0, 0, 0, 0]
            assert not outs['R'].any() and not outs['t'].any() and not outs['mask'].any()
            return
        assert want['margin'] > 1e-9
        assert np.array_equal(outs['info'], want['info'])
        assert np.abs(outs['R'].reshape(3, 3) - want['R']).max() <= 1e-9 and np.abs(outs['t'] - want['t']).max() <= 1e-9
        assert np.array_equal(outs['mask'].astype(bool), want['mask']) and outs['mask'].sum() == outs['info'][0] and outs['mask'].max() <= 1

    return Call([In('E', E), In('pts1', ref['p1'].astype(np.float64)), In('pts2', ref['p2'].astype(np.float64)), n, K9(*ref['K1'].reshape(9)),
                 K9(*ref['K2'].reshape(9)), 50.0, opt(masked, In('mask_in', mask.astype(np.uint8))),
                 NULL if found is None else In('found', np.array([found], np.int32)), Out('R', np.float64, (9,)), Out('t', np.float64, (3,)),
                 Out('mask', np.uint8, (n,)), Out('info', np.int32, (8,)), SCRATCH, SCRATCH_BYTES, STREAM], expect)


RECOVER = Entry('cotr_recover_pose', size_by_pointer('cotr_recover_pose_scratch_bytes', lambda p: (p[0][0],)),
                [Case('n5-every-point', ((5, 0.0, 0.0, 1.0, 0.999, 1, 0), False, None)), Case('n63-masked', ((63, 0.3, 1.0, 1.0, 0.999, 32, 2), True, None)),
                 Case('n2047-masked-found1', ((2047, 0.4, 1.0, 1.0, 0.999, 64, 5), True, 1)), Case('n2048-masked', ((2048, 0.4, 0.5, 1.0, 0.999, 65, 6), True, None)),
                 Case('n2049-masked', ((2049, 0.4, 1.0, 1.0, 0.999, 103, 7), True, None)), Case('n63-found0', ((63, 0.3, 1.0, 1.0, 0.999, 32, 2), True, 0))],
                recover_build, True, lambda p: 188,
                'recover_pose: its one region holds a 188-byte struct in 256 bytes at every shape, so its last 256 bytes always end in padding')


# ---- cotr_refine_pose (csrc/essential.hip on refit.h) --------------------------------------------------------------------------
# RS_CHUNK = 2048 points a workgroup; scratch: the normalised pairs [n][4] double, the state, the per-chunk sums [chunks][22] double,
# every row of which rf_accum_kernel writes.  The rule of tests/test_pose_refit_gpu.py for one round from the fixture's start: the
# mask exactly, R and t within po.REFIT_BOUND of one round of the restatement, the counters, E from the device's own R and t.
def refine_build(params):
    from tests import essential_oracle as eo
    from tests import pose_refit_oracle as po
    scene, found = params
    s = po.start(scene)
    n = scene[0]

    def expect(outs, fill, twin=None):
        xn1, xn2 = eo.normalise(s['p1'], s['K1']), eo.normalise(s['p2'], s['K2'])
        mask = s['mask0']
        assert np.array_equal(outs['mask'].astype(bool), mask) and outs['mask'].max() <= 1
        want = po.fit(s['R0'], po.unit(s['t0']), xn1[mask], xn2[mask], 10)
        R, t, info = outs['R'].reshape(3, 3), outs['t'], outs['info']
        assert max(np.abs(R - want['R']).max(), np.abs(t - want['t']).max()) <= po.REFIT_BOUND
        if want['margin'] > 1e-6:
            assert info[4] == want['kept']
        assert list(info) == [1, mask.sum(), 1, info[4], info[4], want['skipped'], 0, 0]
        assert np.array_equal(outs['E'], po.unit_signed(po.cross_mat(t, R)))

    return Call([In('R_in', s['R0']), In('t_in', s['t0']), In('pts1', s['p1'].astype(np.float64)), In('pts2', s['p2'].astype(np.float64)), n,
                 K9(*s['K1'].reshape(9)), K9(*s['K2'].reshape(9)), float(s['thr']), 50.0, 1, 10, In('mask_in', s['mask0'].astype(np.uint8)),
                 NULL if found is None else In('found', np.array([found], np.int32)), Out('R', np.float64, (9,)), Out('t', np.float64, (3,)),
                 Out('E', np.float64, (9,)), Out('mask', np.uint8, (n,)), Out('info', np.int32, (8,)), SCRATCH, SCRATCH_BYTES, STREAM], expect)


# the last region, [chunks][22] double, is a multiple of 256 bytes only at 16 chunks: n = 32768, where the pairs are whole regions too
REFINE = Entry('cotr_refine_pose', size_by_pointer('cotr_refine_pose_scratch_bytes', lambda p: (p[0][0],)),
               [Case('n5', ((5, 0.0, 0.0, 1.0, 0, 0, 0), None)), Case('n2047', ((2047, 0.4, 1.0, 1.0, 0, 0, 8), None)),
                Case('n2048-found1', ((2048, 0.4, 0.5, 1.0, 0, 0, 9), 1)), Case('n2049', ((2049, 0.4, 1.0, 1.0, 0, 0, 10), None)),
                Case('n32768-regions-exact', ((32768, 0.3, 1.0, 1.0, 0, 0, 12), None))],
               refine_build, True, lambda p: p[0][0] * 32 + -(-p[0][0] // 2048) * 22 * 8, 'n32768-regions-exact')


# ---- cotr_icp_depth (csrc/icp.hip on refit.h) ------------------------------------------------------------------------------------
# 256 pixels a workgroup of the map pass (no tiles), RS_CHUNK = 2048 source pixels a workgroup of the accumulation; scratch: the state,
# the per-chunk sums [chunks][29], A's and B's vertices and normals, the source mask [n_src] uint8, which ic_map_kernel writes in full.
# One step (iters = 1) by the rule of tests/test_icp_gpu.py: the maps bit for bit, both evaluations' sums and the step within
# io.STEP_BOUND, the association exactly off the pixels the restatement flags as near a decision, info the restatement's.
# params: Ha, Wa, Hb, Wb, stride, the optional tables present, a source mask and the found flag present.
def _icp_mask(Hb, Wb):
    return (np.arange(Hb * Wb).reshape(Hb, Wb) % 5 != 0).astype(np.uint8)


def icp_build(params):
    from tests import icp_oracle as io
    Ha, Wa, Hb, Wb, stride, tables, gated = params
    sc = io.scene(Ha, Wa, Hb, Wb, 3, io.SWEEP_EDGE)
    src_mask = _icp_mask(Hb, Wb) if gated else None
    n_src = -(-Hb // stride) * -(-Wb // stride)
    kw = dict(stride=stride, src_mask=src_mask)

    def expect(outs, fill, twin=None):
        if not tables:
            return _ransac_common(outs, twin, ('R', 't', 'info', 'stats'))
        assert np.array_equal(outs['maps_a'], sc['maps_a'], equal_nan=True) and np.array_equal(outs['maps_b'], sc['maps_b'], equal_nan=True)
        R, t, info, hist = outs['R'].reshape(3, 3), outs['t'], outs['info'], outs['hist']

        def same_sums(row, e):
            assert e['near'].sum() <= 0.001 * int(e['usable'].sum())
            rel = np.abs(row[:28] - e['sums'][:28]) / np.where(e['abs'][:28] > 0, e['abs'][:28], 1.0)
            assert (rel <= io.STEP_BOUND).all()

        e0 = io.evaluate(sc['maps_a'], sc['K_a'], sc['maps_b'], sc['R0'], sc['t0'], 0.25, 0.5, **kw)
        same_sums(hist[0], e0)
        reason, d, lmin, lmax = io.step(e0['sums'])
        if reason == 0:
            R1, t1 = io.apply(sc['R0'], sc['t0'], d)
            assert io.pose_distance(R, t, R1, t1) <= io.STEP_BOUND and info[1] == 1
            assert abs(hist[0, 29] - lmin) <= 1e-9 * lmax and abs(hist[0, 30] - lmax) <= 1e-12 * lmax
            e, row = io.evaluate(sc['maps_a'], sc['K_a'], sc['maps_b'], R, t, 0.25, 0.5, **kw), hist[1]
            same_sums(row, e)
        else:
            assert np.array_equal(R, sc['R0']) and np.array_equal(t, sc['t0']) and info[3] == reason and info[1] == 0 and not hist[1].any()
            e, row = e0, hist[0]
        near = e['near']
        assert outs['assoc'].shape == e['assoc'].shape and np.array_equal(outs['assoc'][~near], e['assoc'][~near])
        if np.array_equal(outs['assoc'], e['assoc']):
            assert row[28] == e['sums'][28] == info[2]
        assert outs['stats'][0] == row[27] and abs(outs['stats'][1] - (np.sqrt(row[27] / row[28]) if row[28] else 0.0)) <= 1e-15 * max(1.0, outs['stats'][1])
        o = io.icp(sc['maps_a'], sc['K_a'], sc['maps_b'], sc['R0'], sc['t0'], iters=1, **kw)
        assert list(info) == list(o['info'])

    return Call([In('depth_a', sc['depth_a']), Ha, Wa, K9(*sc['K_a'].reshape(9)), In('depth_b', sc['depth_b']), Hb, Wb, K9(*sc['K_b'].reshape(9)),
                 In('R0', sc['R0']), In('t0', sc['t0']), NULL, In('found', np.array([1], np.int32)) if gated else NULL,
                 In('src_mask', src_mask) if gated else NULL, 0.25, 0.5, float(sc['edge']), 1e-6, 1, stride, Out('R', np.float64, (9,)),
                 Out('t', np.float64, (3,)), Out('info', np.int32, (8,)), Out('stats', np.float64, (2,)), opt(tables, Out('hist', np.float64, (2, 32))),
                 opt(tables, Out('assoc', np.int32, (n_src,))), opt(tables, Out('maps_a', np.float64, (Ha, Wa, 6))),
                 opt(tables, Out('maps_b', np.float64, (Hb, Wb, 6))), SCRATCH, SCRATCH_BYTES, STREAM], expect)


def _icp_twin(params):
    return None if params[5] else params[:5] + (True,) + params[6:]


ICP = Entry('cotr_icp_depth', size_by_pointer('cotr_icp_depth_scratch_bytes', lambda p: p[:5]),
            [Case('a96x128-b3x3-smallest', (96, 128, 3, 3, 1, True, False)), Case('a24x32-b16x16-regions-exact', (24, 32, 16, 16, 1, True, False)),
             Case('a96x128-b23x89-2047', (96, 128, 23, 89, 1, True, False)), Case('a96x128-b32x64-2048', (96, 128, 32, 64, 1, True, False)),
             Case('a96x128-b3x683-2049', (96, 128, 3, 683, 1, True, False)), Case('a24x32-b32x64-stride2-gated', (24, 32, 32, 64, 2, True, True)),
             Case('a24x32-b32x64-stride2-gated-no-tables', (24, 32, 32, 64, 2, False, True))],
            icp_build, True, lambda p: 48 * (p[0] * p[1] + p[2] * p[3]) + -(-p[2] // p[4]) * -(-p[3] // p[4]), 'a24x32-b16x16-regions-exact')


# ---- cotr_triangulate_views (csrc/structure.hip) ---------------------------------------------------------------------------------
# TV_THREADS = 64 points a workgroup; scratch: the view table [32][24] double (24 whole regions), of which tv_prepare_kernel writes
# the rows of the V views given: the last one only with 32 views.  Bit for bit (tests/test_structure_gpu.py).
# params: V, N, visible ('all': NULL, or 'random'), found (None: NULL), robust, refine_iters.
@functools.lru_cache(maxsize=None)
def _tv_case(V, N, vis_kind, found, robust, refine):
    from tests import structure_oracle as so
    sc = so.scene(V, N, noise=0.7, outlier_frac=0.34 if V >= 3 else 0.0, seed=100 * V + N)
    vis = None if vis_kind == 'all' else (np.random.default_rng(V + N).random((V, N)) < 0.8).astype(np.uint8)
    want = so.triangulate(sc['points'], sc['cams'], sc['poses'], visible=vis, robust=bool(robust), refine_iters=refine,
                          found=1 if found is None else found)
    return sc, vis, want


TV_MAX_COS = float(np.cos(np.deg2rad(1.5)))


def views_build(params):
    V, N, vis_kind, found, robust, refine = params
    sc, vis, want = _tv_case(*params)

    def expect(outs, fill, twin=None):
        for k in ('X', 'used', 'quality', 'mask', 'info'):
            assert np.array_equal(outs[k], want[k].astype(outs[k].dtype), equal_nan=True), k
        assert found == 0 or want['info'][1] + want['info'][2:7].sum() == N

    return Call([In('points', sc['points'], 'a16'), opt(vis is not None, In('visible', vis)), In('cams', sc['cams']), In('poses', sc['poses']), V, N,
                 NULL if found is None else In('found', np.array([found], np.int32)), 4.0, TV_MAX_COS, 50.0, refine, robust, 0,
                 Out('X', np.float64, (N, 3)), Out('used', np.uint8, (V, N)), Out('quality', np.float64, (N, 5)), Out('mask', np.uint8, (N,)),
                 Out('info', np.int32, (8,)), SCRATCH, SCRATCH_BYTES, STREAM], expect)


VIEWS = Entry('cotr_triangulate_views', size_by_pointer('cotr_triangulate_views_scratch_bytes', lambda p: p[:2]),
              [Case(f'V{p[0]}-N{p[1]}-{p[2]}' + ('' if p[3] is None else f'-found{p[3]}') + f'-robust{p[4]}-refine{p[5]}', p) for p in [
                  (2, 1, 'all', None, 0, 0), (3, 63, 'random', None, 1, 10), (3, 64, 'all', 1, 1, 10), (3, 65, 'random', None, 0, 10),
                  (5, 257, 'random', None, 1, 1), (3, 64, 'all', 0, 1, 10), (32, 65, 'random', None, 1, 10)]],
              views_build, True, lambda p: 32 * 24 * 8, 'V32-N65-random-robust1-refine10')


# ---- cotr_bundle_adjust (csrc/bundle.hip) ----------------------------------------------------------------------------------------
# BA_THREADS = 256 points a workgroup, RS_CHUNK = 2048 points a chunk of the pair sums; scratch (Carver): the view tables, the state,
# the counters, the steps, then per point X, set, landmark, moves, the point blocks, the cost parts, and last the pair sums
# [pairs][chunks][64] double - whole 512-byte rows at every shape; ba_pairs_kernel writes the row of the last pair whenever the last
# view is free.  One iteration by the rule of tests/test_bundle_gpu.py: the integers exactly, poses, X and both costs within
# bo.STEP_BOUND, on fixtures whose decision clears the margin.
# params: V, N, visible ('all', 'random' or 'used').
@functools.lru_cache(maxsize=None)
def _ba_case(V, N, vis_kind):
    from tests import bundle_oracle as bo
    fx = bo.big_fixture(N) if V == 32 else bo.step_fixture(V, N)
    vis = fx['used'] if V == 32 else dict(fx['visibles'])[vis_kind]
    trace = []
    want = bo.bundle_adjust(fx['points'], fx['cams'], fx['poses0'], fx['X0'], visible=vis, fixed_views=fx['fixed'], iters=1, lambda0=1e-3, trace=trace)
    return fx, vis, want, trace


def _ba_rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    if not ok.any():
        return 0.0
    assert np.array_equal(np.isinf(a[ok]), np.isinf(b[ok]))
    ok &= np.isfinite(b)
    return float(np.abs(a[ok] - b[ok]).max() / max(np.abs(b[ok]).max(), 1e-300)) if ok.any() else 0.0


def bundle_build(params):
    from tests import bundle_oracle as bo
    V, N, vis_kind = params
    fx, vis, want, trace = _ba_case(V, N, vis_kind)
    fixed = np.zeros(V, np.uint8)
    fixed[list(fx['fixed'])] = 1

    def expect(outs, fill, twin=None):
        assert all(t['solved'] and t['front'] and abs(t['cand'] - t['cost']) > bo.DECISION_MARGIN * t['cost'] for t in trace)
        assert np.array_equal(outs['used'], want['used'].astype(np.uint8))
        assert np.array_equal(outs['info'], want['info']) and outs['stats'][2] == want['stats'][2]
        d = (_ba_rel(outs['poses'], want['poses']), _ba_rel(outs['X'], want['X']), _ba_rel(outs['stats'][0], want['stats'][0]),
             _ba_rel(outs['stats'][1], want['stats'][1]))
        assert max(d) <= bo.STEP_BOUND, d
        assert outs['info'][5] + outs['info'][6] == len(trace)

    return Call([In('points', fx['points'], 'a16'), opt(vis is not None, In('visible', None if vis is None else np.asarray(vis, np.uint8))),
                 In('cams', fx['cams']), In('poses_in', fx['poses0']), In('X_in', fx['X0']), (ctypes.c_uint8 * V)(*fixed.tolist()), V, N, NULL, 4.0, 50.0, 1,
                 1, 1e-3, Out('poses', np.float64, (V, 12)), Out('X', np.float64, (N, 3)), Out('used', np.uint8, (V, N)), Out('stats', np.float64, (4,)),
                 Out('info', np.int32, (8,)), SCRATCH, SCRATCH_BYTES, STREAM], expect)


BUNDLE = Entry('cotr_bundle_adjust', size_by_pointer('cotr_bundle_adjust_scratch_bytes', lambda p: p[:2]),
               [Case(f'V{p[0]}-N{p[1]}-{p[2]}', p) for p in [(2, 1, 'all'), (3, 255, 'random'), (3, 256, 'used'), (3, 257, 'all'), (2, 2047, 'used'),
                                                            (2, 2048, 'all'), (2, 2049, 'random'), (32, 65, 'used')]],
               bundle_build, True, lambda p: p[1] * (48 + 4 + 1 + 1 + 72) + (p[0] * (p[0] + 1) // 2) * -(-p[1] // 2048) * 512, 'V3-N256-used')


ENTRIES = [RASTER, DELAUNAY, NEAREST, FUNDAMENTAL, HOMOGRAPHY, ESSENTIAL, RECOVER, REFINE, PNP, RIGID3D, ICP, TSDF_MESH, VIEWS, BUNDLE,
           DEPTH_CORRS, DEPTH_VALID, OVERLAP]
TWINS = {'cotr_ransac_fundamental': _rs_twin, 'cotr_ransac_homography': _rs_twin, 'cotr_ransac_essential': _rs_twin, 'cotr_ransac_pnp': _rs_twin,
         'cotr_ransac_rigid3d': _rg_twin, 'cotr_icp_depth': _icp_twin}


def twin_of(entry, params):
    """the params of the run whose bytes a run without its optional tables must reproduce, or None"""
    return TWINS[entry.name](params) if entry.name in TWINS else None


def all_cases():
    return [(e, c) for e in ENTRIES for c in e.cases]
