"""N-view triangulation timings: cotr_triangulate_views (cotr_amd/csrc/structure.hip) at (V, N) = (2, 2048),
(8, 2048), (32, 2048), (32, 8192), with the pair vote (robust) and without, 10 refinement steps allowed (a scene of cameras
on a baseline, 0.7 px noise, up to a quarter of the views of a point planted as outliers from 5 views on, 4 px threshold), and
the numpy restatement of the same rules (tests/structure_oracle.py) on the same host.

Device times: HIP events around `--iters` calls after `--warmup` (inputs on the device, scratch allocated once), median over
`--rounds` rounds (min / max shown).  Host times once each, host clock.  Every device result is compared with the
restatement bit for bit.
GPU box:  python tools/bench_structure.py [--out profiles/structure_bench.txt]
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
from tests import structure_oracle as so

SHAPES = ((2, 2048), (8, 2048), (32, 2048), (32, 8192))


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


def bench(V, n, a, thr=4.0, dist=50.0, refine=10):
    sc = so.scene(V, n, noise=0.7, outlier_frac=0.25 if V >= 5 else 0.0, seed=V + n)
    pts, cams, poses = (torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ('points', 'cams', 'poses'))
    lib = _lib.load_library()
    nb = ctypes.c_size_t()
    assert lib.cotr_triangulate_views_scratch_bytes(V, n, ctypes.byref(nb)) == 0
    scratch = torch.empty(nb.value, dtype=torch.uint8, device='cuda')
    X, quality = torch.empty((n, 3), dtype=torch.float64, device='cuda'), torch.empty((n, 5), dtype=torch.float64, device='cuda')
    used, mask = torch.empty((V, n), dtype=torch.uint8, device='cuda'), torch.empty(n, dtype=torch.uint8, device='cuda')
    info = torch.empty(8, dtype=torch.int32, device='cuda')
    max_cos = float(np.cos(np.deg2rad(1.5)))
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    stream = _lib.current_stream_ptr()

    def call(robust):
        assert lib.cotr_triangulate_views(p(pts), None, p(cams), p(poses), V, n, None, thr, max_cos, dist, refine, robust, 0, p(X), p(used),
                                          p(quality), p(mask), p(info), p(scratch), nb.value, stream) == 0
    lines = []
    for robust in (1, 0):
        t = timed(lambda: call(robust), a.warmup, a.iters, a.rounds)
        call(robust)
        torch.cuda.synchronize()
        got = dict(X=X.cpu().numpy(), used=used.cpu().numpy(), quality=quality.cpu().numpy(), mask=mask.cpu().numpy(), info=info.cpu().numpy())
        c0 = time.perf_counter()
        want = so.triangulate(sc['points'], sc['cams'], sc['poses'], threshold=thr, max_cos=max_cos, distance_thresh=dist, refine_iters=refine,
                              robust=bool(robust))
        host = (time.perf_counter() - c0) * 1e3
        same = all(np.array_equal(got[k], want[k], equal_nan=True) for k in want)
        right = (got['used'].astype(bool) == ~sc['bad']).all(axis=0).mean()
        i = got['info']
        lines.append(f'V={V}, N={n}, robust={robust}: cotr_triangulate_views {t[0]:.4f} ms ({t[1]:.4f} / {t[2]:.4f}); numpy restatement on the host '
                     f'{host:.0f} ms; identical to numpy: {same}; {i[1]} points in the mask, {i[2]} with too few views, {i[3]} degenerate, '
                     f'{i[4]} / {i[5]} / {i[6]} dropped by depth / error / parallax, {i[7]} steps kept; planted views recovered on '
                     f'{100 * right:.1f} % of the points; median distance to the scene {np.nanmedian(np.linalg.norm(got["X"] - sc["X"], axis=1)):.4f}')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'structure_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_structure.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls; host times once, host clock; refine_iters = 10, threshold 4 px']
    for V, n in SHAPES:
        lines += bench(V, n, a)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
