"""triangulate_corr timings: the raster call alone and the whole function, at the demos' shapes.

  (a) 1000 correspondences, A = 768x1024   (demo_single_pair.py's max_corrs on a typical image)
  (b) 10 000 correspondences, A = 2048x2048

For each shape: device time of cotr_raster_mesh (inputs already on the device, scratch allocated once), and of the whole
triangulate_corr (normalisation, scipy Delaunay, upload, the call, the copy back): HIP events around `--iters` calls after
`--warmup`, median over `--rounds` rounds (min / max shown).  For scale, the numpy restatement (tests/raster_oracle.py) at
shape (a), host clock, once.  Correspondences: random A points, B = a fixed homography of them.  The GPU result is checked
against the restatement (coverage identical, values within 1e-3 px) at every shape.
GPU box:  python tools/bench_triangulate.py [--out profiles/triangulate_bench.txt]
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
from scipy.spatial import Delaunay

from cotr_amd import _lib
from cotr_amd.inference import triangulate_corr
from tests import raster_oracle as ro

SHAPES = [(1000, (768, 1024), (768, 1024)), (10000, (2048, 2048), (2048, 2048))]


def corrs(n, shape_a, seed=0):
    rng = np.random.default_rng(seed)
    pa = rng.uniform(0, 1, (n, 2)) * [shape_a[1], shape_a[0]]
    Hm = np.array([[0.9, 0.05, 30.0], [-0.03, 0.92, 20.0], [1e-5, -2e-5, 1.0]])
    q = np.hstack([pa, np.ones((n, 1))]) @ Hm.T
    return np.hstack([pa, q[:, :2] / q[:, 2:]])


def event_ms(fn, iters, warmup, rounds):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out')
    args = ap.parse_args()
    lib = _lib.load_library()
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {args.rounds} rounds of '
             f'{args.iters} calls after {args.warmup} warm-up calls']
    for n, shape_a, shape_b in SHAPES:
        H, W = shape_a
        corr = corrs(n, shape_a)
        norm = corr / [W, H, shape_b[1], shape_b[0]]
        simp = Delaunay(norm[:, :2]).simplices.astype(np.int32)
        v = torch.from_numpy(norm[:, :2].astype(np.float32)).cuda()
        a = torch.from_numpy(norm[:, 2:].astype(np.float32)).cuda()
        t = torch.from_numpy(simp).cuda()
        nb = ctypes.c_size_t()
        _lib.check(lib.cotr_raster_mesh_scratch_bytes(t.shape[0], H, W, ctypes.byref(nb)), None, 'scratch bytes')
        scratch = torch.empty(nb.value, dtype=torch.uint8, device='cuda')
        out = torch.empty((H, W, 2), device='cuda')
        mask = torch.empty((H, W), dtype=torch.uint8, device='cuda')
        stream = _lib.current_stream_ptr()

        def raster():
            rc = lib.cotr_raster_mesh(ctypes.c_void_p(v.data_ptr()), v.shape[0], ctypes.c_void_p(a.data_ptr()),
                                      ctypes.c_void_p(t.data_ptr()), t.shape[0], H, W, ctypes.c_void_p(out.data_ptr()),
                                      ctypes.c_void_p(mask.data_ptr()), ctypes.c_void_p(scratch.data_ptr()), nb.value, stream)
            assert rc == 0, lib.cotr_raster_last_error()

        r = event_ms(raster, args.iters, args.warmup, args.rounds)
        w = event_ms(lambda: triangulate_corr(corr, shape_a + (3,), shape_b + (3,)), max(1, args.iters // 4), 2, args.rounds)
        ref, ref_mask, _, _ = ro.raster(norm[:, :2].astype(np.float32), norm[:, 2:].astype(np.float32), simp, H, W)
        raster()
        torch.cuda.synchronize()
        m = mask.cpu().numpy().astype(bool)
        err = (np.abs(out.cpu().numpy() - ref) * [shape_b[1], shape_b[0]])[m].max()
        assert np.array_equal(m, ref_mask), 'coverage differs from the restatement'
        lines.append(f'{n} corrs, {len(simp)} triangles, A {H}x{W}: cotr_raster_mesh {r[0]:.4f} ms ({r[1]:.4f} / {r[2]:.4f}); '
                     f'triangulate_corr {w[0]:.3f} ms ({w[1]:.3f} / {w[2]:.3f}); coverage identical to the restatement, '
                     f'max |value - float64| {err:.2e} px')
        if n == SHAPES[0][0]:
            t0 = time.perf_counter()
            ro.raster(norm[:, :2].astype(np.float32), norm[:, 2:].astype(np.float32), simp, H, W)
            lines.append(f'    numpy restatement (tests/raster_oracle.py), same shape, host: {(time.perf_counter() - t0) * 1e3:.0f} ms')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text)


if __name__ == '__main__':
    main()
