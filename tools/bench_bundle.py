"""Bundle adjustment timings: cotr_bundle_adjust (cotr_amd/csrc/bundle.hip) at (V, N) = (2, 2048), (8, 2048),
(32, 2048), (32, 8192), 1 round of 10 iterations from lambda0 = 1e-3, view 0 fixed (a scene of cameras on a baseline, 0.7 px
noise, up to a quarter of the views of a point planted as outliers from 5 views on; the other poses turned by about 0.2 degrees
and moved by about 0.01; the points and the observation set from cotr_triangulate_views at those poses, 8 px threshold), and the
numpy restatement of the same rules (tests/bundle_oracle.py) on the same host.

Device times: HIP events around `--iters` calls after `--warmup` (inputs on the device, scratch allocated once), median over
`--rounds` rounds (min / max shown).  Host times once each, host clock.  Every device result is compared with the restatement.
`--shape V N` measures one shape only (for a kernel trace taken in a run of its own).
GPU box:  python tools/bench_bundle.py [--out profiles/bundle_bench.txt]
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
from cotr_amd.inference import triangulate_views
from tests import bundle_oracle as bo
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


def bench(V, n, a, thr=4.0, dist=50.0, ba_rounds=1, ba_iters=10, lam=1e-3):
    sc = so.scene(V, n, noise=0.7, outlier_frac=0.25 if V >= 5 else 0.0, seed=V + n)
    poses0 = bo.perturbed(sc, rot_deg=0.2, shift=0.01, keep=(0,))
    tri = triangulate_views(sc['points'], sc['cams'], poses0, threshold=8.0)
    torch.cuda.synchronize()
    pts, cams, poses = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (sc['points'], sc['cams'], poses0))
    X0, vis = tri['X'].contiguous(), tri['used'].to(torch.uint8).contiguous()
    lib = _lib.load_library()
    nb = ctypes.c_size_t()
    assert lib.cotr_bundle_adjust_scratch_bytes(V, n, ctypes.byref(nb)) == 0
    scratch = torch.empty(nb.value, dtype=torch.uint8, device='cuda')
    P, X = torch.empty((V, 12), dtype=torch.float64, device='cuda'), torch.empty((n, 3), dtype=torch.float64, device='cuda')
    used, stats, info = (torch.empty((V, n), dtype=torch.uint8, device='cuda'), torch.empty(4, dtype=torch.float64, device='cuda'),
                         torch.empty(8, dtype=torch.int32, device='cuda'))
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    stream = _lib.current_stream_ptr()

    def call():
        assert lib.cotr_bundle_adjust(p(pts), p(vis), p(cams), p(poses), p(X0), None, V, n, None, thr, dist, ba_rounds, ba_iters, lam, p(P), p(X),
                                      p(used), p(stats), p(info), p(scratch), nb.value, stream) == 0
    t = timed(call, a.warmup, a.iters, a.rounds)
    call()
    torch.cuda.synchronize()
    got = dict(poses=P.cpu().numpy(), X=X.cpu().numpy(), used=used.cpu().numpy(), stats=stats.cpu().numpy(), info=info.cpu().numpy())
    line = (f'V={V}, N={n}: cotr_bundle_adjust {t[0]:.4f} ms ({t[1]:.4f} / {t[2]:.4f}), {3 + ba_rounds * (3 + 5 * ba_iters)} launches, scratch '
            f'{nb.value / 2**20:.1f} MiB')
    if not a.no_host:
        c0 = time.perf_counter()
        want = bo.bundle_adjust(sc['points'], sc['cams'], poses0, X0.cpu().numpy(), visible=vis.cpu().numpy(), fixed_views=(0,), threshold=thr,
                                distance_thresh=dist, rounds=ba_rounds, iters=ba_iters, lambda0=lam)
        host = (time.perf_counter() - c0) * 1e3
        ok = np.isfinite(want['X'])
        diff = max(np.abs(got['poses'] - want['poses']).max() / np.abs(want['poses']).max(), np.abs(got['X'][ok] - want['X'][ok]).max() / np.abs(want['X'][ok]).max())
        line += (f'; numpy restatement on the host {host:.0f} ms; largest relative difference of poses and X {diff:.1e}, used and the '
                 f'counters of the set equal: {np.array_equal(got["used"], want["used"]) and np.array_equal(got["info"][:5], want["info"][:5])}, '
                 f'the restatement kept {want["info"][5]} steps')
    i, s = got['info'], got['stats']
    e0, e1 = bo.pose_errors(poses0, sc['poses']), bo.pose_errors(got['poses'], sc['poses'])
    line += (f'; {i[1]} observations, {i[2]} free views, {i[3]} frozen, {i[4]} landmarks, {i[5]} steps kept, {i[6]} rejected; cost {s[0]:.6g} -> '
             f'{s[1]:.6g}; worst rotation error {e0[0]:.3f} -> {e1[0]:.3f} deg')
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--shape', type=int, nargs=2, default=None, metavar=('V', 'N'))
    ap.add_argument('--no-host', action='store_true', help='skip the numpy restatement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bundle_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_bundle.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls; host times once, host clock; 1 round of 10 iterations, lambda0 = 1e-3, view 0 fixed']
    for V, n in ((tuple(a.shape),) if a.shape else SHAPES):
        lines += bench(V, n, a)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
