"""cotr_delaunay timings: the device triangulation alone, and triangulate_corr with it and with scipy, at the shapes of
tools/bench_triangulate.py:

  (a) 1000 correspondences, A = 768x1024
  (b) 10 000 correspondences, A = 2048x2048

For each shape: device time of cotr_delaunay (points already on the device, scratch allocated once; HIP events around
`--iters` calls after `--warmup`, median over `--rounds` rounds, min / max shown), and the time of a whole
triangulate_corr(..., as_tensor=True) call ending in a device synchronise (host clock: the scipy path is host work), for
three forms measured alternately in the same process, round by round: simplices='device' from a device tensor,
simplices='device' from the numpy array, and the scipy path from the same numpy array.  The device triangles are checked
against scipy's of the snapped points (equal sets where no four points are cocircular) and the two maps against each other (1e-3 px).
GPU box:  python tools/bench_delaunay.py [--out profiles/delaunay_bench.txt]
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
from tools.bench_triangulate import SHAPES, corrs, event_ms


def wall_ms(fns, iters, warmup, rounds):
    """host-clock milliseconds per call of every fn, each call followed to its end on the device; the fns take turns within a round"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3 / iters)
    return [(statistics.median(o), min(o), max(o)) for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out')
    args = ap.parse_args()
    lib = _lib.load_library()
    lines = [f'device: {torch.cuda.get_device_name(0)}; median (min / max) over {args.rounds} rounds of {args.iters} calls after '
             f'{args.warmup} warm-up calls; cotr_delaunay by HIP events, whole calls by the host clock around calls that end in a '
             'synchronise, the three forms taking turns within a round']
    for n, shape_a, shape_b in SHAPES:
        H, W = shape_a
        corr = corrs(n, shape_a)
        norm = corr / [W, H, shape_b[1], shape_b[0]]
        v = torch.from_numpy(norm[:, :2].astype(np.float32)).cuda()
        nb = ctypes.c_size_t()
        _lib.check_op(lib.cotr_delaunay_scratch_bytes(n, ctypes.byref(nb)), 'scratch bytes')
        scratch = torch.empty(nb.value, dtype=torch.uint8, device='cuda')
        tris = torch.empty((lib.cotr_delaunay_max_tris(n), 3), dtype=torch.int32, device='cuda')
        info = torch.empty(2, dtype=torch.int32, device='cuda')
        stream = _lib.current_stream_ptr()

        def call():
            rc = lib.cotr_delaunay(ctypes.c_void_p(v.data_ptr()), n, ctypes.c_void_p(tris.data_ptr()), ctypes.c_void_p(info.data_ptr()),
                                   ctypes.c_void_p(scratch.data_ptr()), nb.value, stream)
            assert rc == 0, lib.cotr_raster_last_error()

        d = event_ms(call, args.iters, args.warmup, args.rounds)
        count, status = info.tolist()
        assert status == 0
        got = {tuple(sorted(t)) for t in tris[:count].cpu().numpy().tolist()}
        snapped = np.rint(norm[:, :2].astype(np.float32).astype(np.float64) * 2.0 ** 24)      # what the rule triangulates
        want = {tuple(sorted(t)) for t in Delaunay(snapped).simplices.tolist()}
        corr_dev = torch.from_numpy(corr).cuda()
        sa, sb = shape_a + (3,), shape_b + (3,)
        forms = [lambda: triangulate_corr(corr_dev, sa, sb, simplices='device', as_tensor=True),
                 lambda: triangulate_corr(corr, sa, sb, simplices='device', as_tensor=True),
                 lambda: triangulate_corr(corr, sa, sb, as_tensor=True)]
        w = wall_ms(forms, max(1, args.iters // 2), 2, args.rounds)
        m_dev, m_host = forms[1](), forms[2]()
        err = float((m_dev - m_host).abs().max())
        lines.append(f'{n} corrs, A {H}x{W}: cotr_delaunay {d[0]:.3f} ms ({d[1]:.3f} / {d[2]:.3f}), {count} triangles, '
                     f'{"the same set as" if got == want else f"{len(got ^ want)} triangles differ from"} scipy\'s of the snapped points')
        for name, t in zip(("simplices='device', corr on the device", "simplices='device', corr a numpy array", 'scipy path, corr a numpy array'), w):
            lines.append(f'    triangulate_corr(as_tensor=True), {name}: {t[0]:.3f} ms ({t[1]:.3f} / {t[2]:.3f})')
        lines.append(f'    max |device map - scipy map| {err:.2e} px')
    # where the quadratic cost starts to matter: the triangulations alone at the largest n the call takes
    n = 65536
    pts = np.random.default_rng(1).uniform(0, 1, (n, 2)).astype(np.float32)
    v = torch.from_numpy(pts).cuda()
    nb = ctypes.c_size_t()
    _lib.check_op(lib.cotr_delaunay_scratch_bytes(n, ctypes.byref(nb)), 'scratch bytes')
    scratch = torch.empty(nb.value, dtype=torch.uint8, device='cuda')
    tris = torch.empty((lib.cotr_delaunay_max_tris(n), 3), dtype=torch.int32, device='cuda')
    info = torch.empty(2, dtype=torch.int32, device='cuda')

    def call_max():
        rc = lib.cotr_delaunay(ctypes.c_void_p(v.data_ptr()), n, ctypes.c_void_p(tris.data_ptr()), ctypes.c_void_p(info.data_ptr()),
                               ctypes.c_void_p(scratch.data_ptr()), nb.value, _lib.current_stream_ptr())
        assert rc == 0, lib.cotr_raster_last_error()

    d = event_ms(call_max, 2, 1, 5)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        Delaunay(pts.astype(np.float64))
        host.append((time.perf_counter() - t0) * 1e3)
    lines.append(f'{n} points (the most the call takes), the triangulations alone: cotr_delaunay {d[0]:.1f} ms ({d[1]:.1f} / {d[2]:.1f}), '
                 f'{info.tolist()[0]} triangles, status {info.tolist()[1]}; scipy.spatial.Delaunay on the host {statistics.median(host):.1f} ms '
                 f'({min(host):.1f} / {max(host):.1f})')
    text ='\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text)


if __name__ == '__main__':
    main()
