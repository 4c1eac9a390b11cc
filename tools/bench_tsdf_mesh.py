"""Mesh extraction timings: cotr_tsdf_mesh (cotr_amd/csrc/tsdf.hip) on the three-plane corner of tests/icp_oracle.py fused from two
480 x 640 captures into 128^3 and 256^3 voxels, count only, with exact capacities and with normals, against the least bytes a call
must move (8 B a voxel read once, plus the outputs: 24 B a vertex, as much again with normals, 12 B a triangle).  Beside them the
numpy restatement of the same rule (tests/mesh_oracle.py) on the same host at 128^3, which the device result is checked against.

The volume: origin (-3.9, -3.0, 2.9), 6.4 a side (voxel 0.05 at 128^3, 0.025 at 256^3), trunc 3 voxels.  Device times: HIP events
around `--iters` calls after `--warmup`, median over `--rounds` rounds (min / max shown).  Host times once, host clock.
GPU box:  python tools/bench_tsdf_mesh.py [--out profiles/tsdf_mesh_bench.txt]
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cotr_amd import _lib
from cotr_amd.inference import TsdfVolume, extract_mesh, integrate_depths
from tests import mesh_oracle as mo
from tests import tsdf_oracle as to
from tools.bench_tsdf import ORIGIN, SHAPE, SIDE, timed


def mesh_call(vol, cap_verts, cap_tris, normals):
    """one cotr_tsdf_mesh through the C ABI with everything prepared: the time is the library's, not the wrapper's"""
    lib = _lib.load_library()
    Nx, Ny, Nz = vol.dims
    n = ctypes.c_size_t()
    assert lib.cotr_tsdf_mesh_scratch_bytes(Nx, Ny, Nz, ctypes.byref(n)) == 0
    scratch = torch.empty(n.value, dtype=torch.uint8, device='cuda')
    verts, nrm = (torch.empty((cap_verts, 3), dtype=torch.float64, device='cuda') for _ in range(2))
    tris, info = torch.empty((cap_tris, 3), dtype=torch.int32, device='cuda'), torch.empty(4, dtype=torch.int32, device='cuda')
    origin = (ctypes.c_double * 3)(*vol.origin)
    p = lambda x, on=True: ctypes.c_void_p(x.data_ptr()) if on and x.numel() else None   # noqa: E731
    stream = _lib.current_stream_ptr()

    def call():
        assert lib.cotr_tsdf_mesh(p(vol.tsdf), p(vol.weight), Nx, Ny, Nz, origin, vol.voxel, None, p(verts), cap_verts, p(nrm, normals), p(tris), cap_tris,
                                  p(info), p(scratch), n.value, stream) == 0
    return call, (verts, nrm, tris, info, scratch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tsdf_mesh_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_tsdf_mesh.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls; host times once, host clock']
    depths, Ks, c2ws = to.captures(*SHAPE, 2)
    for N in (128, 256):
        vol = TsdfVolume(ORIGIN, SIDE / N, (N, N, N))
        integrate_depths(vol, depths, Ks, c2ws)
        info = extract_mesh(vol, 0, 0)[3].cpu().numpy()
        V, T = int(info[1]), int(info[2])
        lines.append(f'{N}^3 ({N ** 3 / 1e6:.1f} M voxels), the corner fused from 2 captures of {SHAPE[0]} x {SHAPE[1]}: {V} vertices, {T} triangles, '
                     f'{info[3]} valid cells; scratch {6 * N ** 3 / 1e6:.0f} MB')
        for what, cv, ct, normals in (('count only (4 launches)', 0, 0, False), ('vertices and triangles (6 launches)', V, T, False),
                                      ('with normals (6 launches)', V, T, True)):
            call, keep = mesh_call(vol, cv, ct, normals)
            t = timed(call, a.warmup, a.iters, a.rounds)
            least = 8 * N ** 3 + 24 * cv * (2 if normals else 1) + 12 * ct
            lines.append(f'    {what}: {t[0]:.4f} ms ({t[1]:.4f} / {t[2]:.4f}); the least it must move: {least / 1e6:.1f} MB = '
                         f'{least / (t[0] * 1e-3) / 1e9:.0f} GB/s at that time')
            del keep
        if N == 128:
            verts, tris, nrm, _ = extract_mesh(vol, normals=True)
            c0 = time.perf_counter()
            o = mo.mesh(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.origin, vol.voxel, normals=True)
            host = time.perf_counter() - c0
            same = (np.array_equal(verts.cpu().numpy(), o['verts']) and np.array_equal(tris.cpu().numpy(), o['tris']) and
                    np.array_equal(nrm.cpu().numpy(), o['normals'], equal_nan=True) and list(info) == list(o['info']))
            lines.append(f'    vertices, triangles, normals and info identical to the restatement: {same}; host, numpy restatement with normals: {host * 1e3:.0f} ms')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
