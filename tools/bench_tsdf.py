"""TSDF volume timings: cotr_tsdf_integrate (cotr_amd/csrc/tsdf.hip) at 128^3 and 256^3 voxels with 1 and 8 captures of 480 x 640
of the three-plane corner of tests/icp_oracle.py, against the least bytes a call must move (16 B a voxel: tsdf and weight read
and written once, whatever the number of captures), and cotr_tsdf_raycast of the fused 128^3 volume at 480 x 640 in samples per
second (the samples the rule takes: every ray from sample 0 to its hit, its back face or its last sample).  Beside them the
numpy restatement of the same rules (tests/tsdf_oracle.py) on the same host at 128^3, which the device result is checked against.

The volume: origin (-3.9, -3.0, 2.9), 6.4 a side (voxel 0.05 at 128^3, 0.025 at 256^3), trunc 3 voxels; the raycast from the first
camera, near 0.5, far 8, step trunc / 2.  Device times: HIP events around `--iters` calls after `--warmup`, median over `--rounds`
rounds (min / max shown).  Host times once each, host clock.
GPU box:  python tools/bench_tsdf.py [--out profiles/tsdf_bench.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cotr_amd import _lib
from cotr_amd.inference import TsdfVolume, integrate_depths, raycast_volume
from cotr_amd.inference._args import camera
from tests import icp_oracle as io
from tests import tsdf_oracle as to

ORIGIN, SIDE, SHAPE = (-3.9, -3.0, 2.9), 6.4, (480, 640)


def timed(fn, warmup, iters, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / iters)
    return statistics.median(ts), min(ts), max(ts)


def integrate_call(vol, d, Ks, c):
    """one cotr_tsdf_integrate through the C ABI with everything prepared: the time is the library's, not the wrapper's"""
    lib, n = _lib.load_library(), int(d.shape[0])
    K = (ctypes.c_double * (9 * n))(*np.asarray(Ks[:n], np.float64).reshape(-1))
    info = torch.empty((n, 4), dtype=torch.int32, device='cuda')
    origin = (ctypes.c_double * 3)(*vol.origin)
    Nx, Ny, Nz = vol.dims
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    stream = _lib.current_stream_ptr()

    def call():
        assert lib.cotr_tsdf_integrate(p(vol.tsdf), p(vol.weight), Nx, Ny, Nz, origin, vol.voxel, vol.trunc, p(d), n, d.shape[1], d.shape[2], K, p(c),
                                       None, None, vol.max_weight, p(info), stream) == 0
    return call, info


def raycast_call(vol, K, pose, near, far, step, normals):
    lib = _lib.load_library()
    k, c = camera(K, 'K'), torch.from_numpy(pose.reshape(16)).cuda()
    depth, info = torch.empty(SHAPE, dtype=torch.float32, device='cuda'), torch.empty(4, dtype=torch.int32, device='cuda')
    nrm = torch.empty(SHAPE + (3,), dtype=torch.float64, device='cuda') if normals else None
    origin = (ctypes.c_double * 3)(*vol.origin)
    Nx, Ny, Nz = vol.dims
    p = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None else None)   # noqa: E731
    stream = _lib.current_stream_ptr()

    def call():
        assert lib.cotr_tsdf_raycast(p(vol.tsdf), p(vol.weight), Nx, Ny, Nz, origin, vol.voxel, k, p(c), None, SHAPE[0], SHAPE[1], near, far, step,
                                     p(depth), p(nrm), p(info), stream) == 0
    return call


def bench_integrate(N, n, depths, Ks, c2ws, a):
    vol = TsdfVolume(ORIGIN, SIDE / N, (N, N, N))
    d, c = torch.from_numpy(depths[:n]).cuda(), torch.from_numpy(np.ascontiguousarray(c2ws[:n].reshape(n, 16))).cuda()
    call, info = integrate_call(vol, d, Ks, c)
    t = timed(call, a.warmup, a.iters, a.rounds)
    info = info.cpu().numpy()
    least = 16 * N ** 3
    return (f'integrate {N}^3 ({N ** 3 / 1e6:.1f} M voxels), {n} capture{"s" if n > 1 else ""} of {SHAPE[0]} x {SHAPE[1]} (2 launches): {t[0]:.4f} ms '
            f'({t[1]:.4f} / {t[2]:.4f}); the least it must move: {least / 1e6:.1f} MB = {least / (t[0] * 1e-3) / 1e9:.0f} GB/s at that time, '
            f'{N ** 3 * n / (t[0] * 1e-3) / 1e9:.2f} G voxel-captures/s; updated {info[:, 1].tolist()}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tsdf_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_tsdf.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls; host times once, host clock']
    depths, Ks, c2ws = to.captures(*SHAPE, 8)
    for N in (128, 256):
        for n in (1, 8):
            lines.append(bench_integrate(N, n, depths, Ks, c2ws, a))
    # the raycast of the two captures fused at 128^3, and both steps against the restatement
    N = 128
    vol = TsdfVolume(ORIGIN, SIDE / N, (N, N, N))
    integrate_depths(vol, depths[:2], Ks[:2], c2ws[:2])
    K, pose = io.scaled_camera(io.corner_scene()['K_a'], *SHAPE), c2ws[0]
    ray = dict(near=0.5, far=8.0, step=vol.trunc / 2)
    t = timed(raycast_call(vol, K, pose, normals=False, **ray), a.warmup, a.iters, a.rounds)
    tn = timed(raycast_call(vol, K, pose, normals=True, **ray), a.warmup, a.iters, a.rounds)
    r = {k: v.cpu().numpy() for k, v in raycast_volume(vol, K, pose, SHAPE, normals=True, **ray).items()}
    c0 = time.perf_counter()
    o = to.integrate(*to.fresh(vol.dims), ORIGIN, vol.voxel, vol.trunc, depths[:2], Ks[:2], c2ws[:2])
    host_int = time.perf_counter() - c0
    c0 = time.perf_counter()
    q = to.raycast(o['tsdf'], o['weight'], ORIGIN, vol.voxel, K, pose, SHAPE, ray['near'], ray['far'], ray['step'], normals=True)
    host_ray = time.perf_counter() - c0
    same_vol = np.array_equal(vol.tsdf.cpu().numpy(), o['tsdf']) and np.array_equal(vol.weight.cpu().numpy(), o['weight'])
    same_ray = np.array_equal(r['depth'], q['depth']) and np.array_equal(r['normals'], q['normals'], equal_nan=True) and list(r['info']) == list(q['info'])
    ref = io.render(*SHAPE, K, pose, io.PLANES)
    e = np.abs(r['depth'] - ref)[r['depth'] > 0]
    lines += [f'raycast {N}^3 at {SHAPE[0]} x {SHAPE[1]}, {to.steps(ray["near"], ray["far"], ray["step"]) + 1} samples a ray at most (2 launches): {t[0]:.4f} ms '
              f'({t[1]:.4f} / {t[2]:.4f}), with normals {tn[0]:.4f} ms ({tn[1]:.4f} / {tn[2]:.4f}); {q["samples"]} samples = '
              f'{q["samples"] / (t[0] * 1e-3) / 1e9:.2f} G samples/s; {r["info"][1]} of {SHAPE[0] * SHAPE[1]} pixels hit, {r["info"][2]} back faces',
              f'    against the renderer of the scene: median {np.median(e):.2e}, p90 {np.percentile(e, 90):.2e}, max {e.max():.2e}',
              f'    volume identical to the restatement: {same_vol} ({int(o["near"].sum())} voxels flagged); depth, normals and info identical: {same_ray} '
              f'({int(q["near"].sum())} pixels flagged)',
              f'    host, numpy restatement: 2 captures into {N}^3 {host_int * 1e3:.0f} ms, the raycast with normals {host_ray * 1e3:.0f} ms']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
