"""``cotr_tsdf_mesh`` on the MI355X (cotr_amd/csrc/tsdf.hip) against the numpy restatement tests/mesh_oracle.py: vertices,
triangles and normals bit for bit (NaN where the restatement has NaN) and ``info`` exactly, at the smallest volumes at which
the indexing can go wrong, on a sphere, on the fused corner scene and on a volume deeper than one pass of the scan; the
capacity rules, the ``found`` gate, repeatability, and the wrappers on top.

The sizes of the passes: ms_classify_kernel takes 256 voxels a block and ms_count_kernel 512, and both run on at most MS_GRID =
2048 workgroups that walk the blocks, so one walk covers 2048 * 256 = 524288 and 2048 * 512 = 1048576 voxels; ms_scan_kernel takes
1024 block totals a pass, 1024 * 512 = 524288 voxels.  ``DEEP`` has 160 * 96 * 72 = 1105920 voxels, more than any of them: 2160
blocks of 512, of which 112 workgroups of ms_count_kernel take a second, three passes of the scan, up to three walks of the
classify pass.  It is cut by one plane across x, so that every block holds vertices, triangles and valid cells - those of the
second walk too, which the test asserts."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.data import Capture
from cotr_amd.inference import TsdfVolume, extract_mesh, fuse_captures, integrate_depths, write_ply
from tests import icp_oracle as io
from tests import mesh_oracle as mo
from tests import tsdf_oracle as to

pytestmark = pytest.mark.gpu

ORIGIN, VOXEL = (0.31, -1.27, 2.05), 0.05
SENTINEL = -7.0
DEEP = (160, 96, 72)
WALK = 2048 * 512   # voxels of one walk of ms_count_kernel, the widest pass of any level
assert DEEP[0] * DEEP[1] * DEEP[2] > WALK > 1024 * 512


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Call:
    """the device copy of a volume and its scratch; ``run`` is one ``cotr_tsdf_mesh`` through the C ABI into fresh buffers filled
    with sentinels, so that what the call did not write shows"""

    def __init__(self, tsdf, weight, origin=ORIGIN, voxel=VOXEL):
        self.lib = _lib.load_library()
        self.tsdf, self.weight = (t if torch.is_tensor(t) else cu(t) for t in (tsdf, weight))
        self.Nz, self.Ny, self.Nx = (int(v) for v in self.tsdf.shape)
        self.origin, self.voxel = (ctypes.c_double * 3)(*origin), float(voxel)
        n = ctypes.c_size_t()
        assert self.lib.cotr_tsdf_mesh_scratch_bytes(self.Nx, self.Ny, self.Nz, ctypes.byref(n)) == 0
        self.nbytes = n.value
        self.scratch = torch.empty(n.value, dtype=torch.uint8, device='cuda')

    def buffers(self, cap_verts, cap_tris, normals):
        return dict(verts=torch.full((cap_verts, 3), SENTINEL, dtype=torch.float64, device='cuda'),
                    normals=torch.full((cap_verts, 3), SENTINEL, dtype=torch.float64, device='cuda') if normals else None,
                    tris=torch.full((cap_tris, 3), -9, dtype=torch.int32, device='cuda'), info=torch.full((4,), -3, dtype=torch.int32, device='cuda'))

    def enqueue(self, b, found=None, stream=None):
        cv, ct = int(b['verts'].shape[0]), int(b['tris'].shape[0])
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
        rc = self.lib.cotr_tsdf_mesh(p(self.tsdf), p(self.weight), self.Nx, self.Ny, self.Nz, self.origin, self.voxel, p(found), p(b['verts']) if cv else None,
                                     cv, p(b['normals']) if cv else None, p(b['tris']) if ct else None, ct, p(b['info']), p(self.scratch), self.nbytes, stream)
        assert rc == 0, self.lib.cotr_raster_last_error()

    def run(self, cap_verts, cap_tris, normals=False, found=None):
        b = self.buffers(cap_verts, cap_tris, normals)
        self.enqueue(b, None if found is None else torch.tensor([found], dtype=torch.int32, device='cuda'))
        torch.cuda.synchronize()
        return {k: None if v is None else v.cpu().numpy() for k, v in b.items()}


def same_mesh(r, o, cap_verts=None, cap_tris=None, what=''):
    """what a call wrote against the restatement under the capacity rules: the first min(count, capacity) rows are the mesh's,
    vertex rows past them are not written, triangle rows past the count are -1"""
    V, T = int(o['info'][1]), int(o['info'][2])
    cv, ct = len(r['verts']), len(r['tris'])
    assert r['info'].tolist() == o['info'].tolist(), (what, r['info'], o['info'])
    nv, nt = min(V, cv), min(T, ct)
    assert np.array_equal(r['verts'][:nv], o['verts'][:nv]) and (r['verts'][nv:] == SENTINEL).all(), what
    assert np.array_equal(r['tris'][:nt], o['tris'][:nt]) and (r['tris'][nt:] == -1).all(), what
    if r['normals'] is not None:
        assert np.array_equal(r['normals'][:nv], o['normals'][:nv], equal_nan=True) and (r['normals'][nv:] == SENTINEL).all(), what


def check(tsdf, weight, what, normals=True, origin=ORIGIN, voxel=VOXEL):
    """count only, then an exact call, against the restatement -> (the restatement, the Call)"""
    o = mo.mesh(tsdf, weight, origin, voxel, normals=True)
    call = Call(tsdf, weight, origin, voxel)
    count = call.run(0, 0)
    assert count['info'].tolist() == o['info'].tolist(), (what, count['info'], o['info'])
    r = call.run(int(o['info'][1]), int(o['info'][2]), normals)
    same_mesh(r, o, what=what)
    nan = int(np.isnan(o['normals']).any(1).sum())
    print(f'{what}: info {r["info"].tolist()}, {nan} vertices without a normal')
    return o, call


# ---- every size -----------------------------------------------------------------------------------------------------------
SMALL = ((2, 2, 2), (3, 5, 7), (4, 4, 4), (7, 3, 3), (65, 2, 2), (67, 3, 2))


@pytest.mark.parametrize('normals', [True, False], ids=['normals', 'plain'])
@pytest.mark.parametrize('holes', [0.0, 0.04], ids=['observed', 'holes'])
@pytest.mark.parametrize('dims', SMALL, ids=lambda d: 'x'.join(str(v) for v in d))
def test_random_volumes_at_every_size(dims, holes, normals):
    tsdf, weight = mo.random_volume(dims, 11, holes)
    o, _ = check(tsdf, weight, f'{dims} holes {holes}', normals)
    if holes == 0:
        assert o['info'][3] == np.prod(np.array(dims) - 1) and o['info'][2] > 0


def test_the_random_8_cubed_with_holes_reaches_all_96_cases():
    tsdf, weight = mo.random_volume((8, 8, 8), 0, 0.1)
    o, _ = check(tsdf, weight, '8^3 with holes')
    assert o['cases'].all() and np.isnan(o['normals']).any() and not np.isnan(o['normals']).all()


def test_the_sphere():
    tsdf, weight, _ = mo.sphere(17, 6.3)
    o, _ = check(tsdf, weight, 'sphere r = 6.3 in 17^3', origin=(0.0, 0.0, 0.0), voxel=1.0)
    assert o['info'].tolist() == [1, 2250, 4496, 4096] and not np.isnan(o['normals']).any()


_CORNER = {}


def corner_volume():
    """the corner's two 48 x 64 captures fused on the device into 32^3 voxels of 0.2"""
    if 'vol' not in _CORNER:
        vol = TsdfVolume(to.ORIGIN_64, 0.2, (32, 32, 32))
        integrate_depths(vol, *to.captures(48, 64))
        torch.cuda.synchronize()
        _CORNER['vol'] = vol
        _CORNER['mesh'] = mo.mesh(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.origin, vol.voxel, normals=True)
    return _CORNER['vol'], _CORNER['mesh']


def test_the_corner_scene_fused_on_the_device():
    vol, o = corner_volume()
    call = Call(vol.tsdf, vol.weight, vol.origin, vol.voxel)
    same_mesh(call.run(int(o['info'][1]), int(o['info'][2]), True), o, what='the corner')
    print(f'the corner in 32^3: info {o["info"].tolist()}')
    assert o['info'][1] > 1000 and o['info'][2] > 2000 and 0 < o['info'][3] < 31 ** 3
    # the mesh lies on the scene's planes: every vertex within a voxel of the nearest one
    d = np.min([np.abs(o['verts'] @ np.asarray(n) - c) / np.linalg.norm(n) for n, c in io.PLANES], axis=0)
    assert d.max() < vol.voxel, d.max()


def test_a_volume_deeper_than_one_pass_of_every_level():
    tsdf, weight = mo.plane_volume(DEEP, 70.37, axis=0)
    o, _ = check(tsdf, weight, f'{DEEP} cut by a plane across x')
    assert o['info'][2] == 8 * (DEEP[1] - 1) * (DEEP[2] - 1) and o['info'][3] == np.prod(np.array(DEEP) - 1)
    # vertices, triangles and valid cells in the first walk, past one pass of the scan, and in the second walk
    for what in (o['vert_voxel'], o['tri_cell']):
        assert (what < 1024 * 512).any() and ((what >= 1024 * 512) & (what < WALK)).any() and (what >= WALK).any()
    assert o['tri_cell'].max() >= WALK + 512   # more than one block of the second walk


# ---- capacities and the gate ----------------------------------------------------------------------------------------------
_RANDOM8 = {}


def random8():
    if not _RANDOM8:
        tsdf, weight = mo.random_volume((8, 8, 8), 0, 0.1)
        _RANDOM8.update(o=mo.mesh(tsdf, weight, ORIGIN, VOXEL, normals=True), call=Call(tsdf, weight))
    return _RANDOM8['o'], _RANDOM8['call']


@pytest.mark.parametrize('which', ['verts', 'tris'])
@pytest.mark.parametrize('delta', [None, -1, 0, 5], ids=['none', 'count-1', 'count', 'count+5'])
def test_capacities(which, delta):
    o, call = random8()
    V, T = int(o['info'][1]), int(o['info'][2])
    cap = 0 if delta is None else (V if which == 'verts' else T) + delta
    cv, ct = (cap, T) if which == 'verts' else (V, cap)
    same_mesh(call.run(cv, ct, True), o, what=f'capacities {cv} / {ct}')


def test_count_only_and_tiny_capacities():
    o, call = random8()
    for cv, ct in ((0, 0), (1, 1), (0, 7), (3, 0)):
        same_mesh(call.run(cv, ct, True), o, what=f'capacities {cv} / {ct}')


def test_found_0():
    o, call = random8()
    r = call.run(int(o['info'][1]), int(o['info'][2]) + 5, True, found=0)
    assert (r['info'] == 0).all() and (r['tris'] == -1).all() and (r['verts'] == SENTINEL).all() and (r['normals'] == SENTINEL).all()
    assert (call.run(0, 0, found=0)['info'] == 0).all()
    same_mesh(call.run(int(o['info'][1]), int(o['info'][2]), True, found=1), o, what='found = 1')


def test_same_bytes_across_calls_streams_and_graph_replay():
    vol, o = corner_volume()
    call = Call(vol.tsdf, vol.weight, vol.origin, vol.voxel)
    V, T = int(o['info'][1]), int(o['info'][2])

    def same(a, b):
        for key in a:
            assert a[key].cpu().numpy().tobytes() == b[key].cpu().numpy().tobytes(), key
    first, again = call.buffers(V + 3, T + 3, True), call.buffers(V + 3, T + 3, True)
    call.enqueue(first)
    call.enqueue(again)
    torch.cuda.synchronize()
    same(first, again)
    same_mesh({k: v.cpu().numpy() for k, v in first.items()}, o, what='first')
    b = call.buffers(V + 3, T + 3, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    call.enqueue(b, stream=ctypes.c_void_p(side.cuda_stream))
    side.synchronize()
    same(first, b)
    # captured once (a single linear chain on the capture stream), replayed once
    b = call.buffers(V + 3, T + 3, True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.enqueue(b)
    graph.replay()
    torch.cuda.synchronize()
    same(first, b)


# ---- the wrappers ---------------------------------------------------------------------------------------------------------
def test_extract_mesh_in_both_modes():
    vol, o = corner_volume()
    V, T = int(o['info'][1]), int(o['info'][2])
    verts, tris, normals, info = extract_mesh(vol, normals=True)
    assert tuple(verts.shape) == (V, 3) and tuple(tris.shape) == (T, 3) and verts.dtype == torch.float64 and tris.dtype == torch.int32
    assert np.array_equal(verts.cpu().numpy(), o['verts']) and np.array_equal(tris.cpu().numpy(), o['tris'])
    assert np.array_equal(normals.cpu().numpy(), o['normals'], equal_nan=True) and info.is_cuda and info.tolist() == o['info'].tolist()
    assert extract_mesh(vol)[2] is None
    # fixed capacities: padded tensors
    verts, tris, normals, info = extract_mesh(vol, max_verts=V + 4, max_tris=T - 10, normals=True)
    assert tuple(verts.shape) == (V + 4, 3) and tuple(tris.shape) == (T - 10, 3) and tuple(normals.shape) == (V + 4, 3) and info.tolist() == o['info'].tolist()
    assert np.array_equal(verts[:V].cpu().numpy(), o['verts']) and np.array_equal(tris.cpu().numpy(), o['tris'][:T - 10])
    verts, tris, normals, info = extract_mesh(vol, max_verts=0, max_tris=T + 2)
    assert normals is None and tuple(verts.shape) == (0, 3) and np.array_equal(tris[:T].cpu().numpy(), o['tris']) and (tris[T:] == -1).all()
    # a fresh volume has no valid cell
    empty = extract_mesh(TsdfVolume((0.0, 0.0, 0.0), 0.1, (5, 4, 3)), normals=True)
    assert tuple(empty[0].shape) == (0, 3) and tuple(empty[1].shape) == (0, 3) and tuple(empty[2].shape) == (0, 3) and empty[3].tolist() == [1, 0, 0, 0]


def test_fuse_captures_to_a_ply_file(tmp_path):
    sc = io.scene(48, 64, 48, 64, 3)
    caps = [Capture(None, sc['depth_a'], sc['K_a'], sc['c2w_a']), Capture(None, torch.from_numpy(sc['depth_b']).cuda(), sc['K_b'], sc['c2w_b'])]
    vol, infos = fuse_captures(caps, origin=to.ORIGIN_64, voxel=0.2, dims=(32, 32, 32))
    assert all(r['integrated'] for r in infos)
    _, o = corner_volume()
    verts, tris, normals, info = extract_mesh(vol, max_verts=int(o['info'][1]), max_tris=int(o['info'][2]) + 8, normals=True)
    write_ply(tmp_path / 'corner.ply', verts, tris, normals)
    cols, v, f = mo.read_ply(tmp_path / 'corner.ply')
    assert cols == ['x', 'y', 'z', 'nx', 'ny', 'nz'] and np.array_equal(v[:, :3], o['verts']) and np.array_equal(v[:, 3:], o['normals'], equal_nan=True)
    assert np.array_equal(f, o['tris'])
