"""Timings of cotr_build_tracks (cotr_amd/csrc/tracks.hip) at V views x keypoints per view = (8, 2048), (32, 2048),
(32, 8192): every view holds the same points under a permutation of its own, every pair of views with j - i <= 2 (13 pairs at 8
views, 61 at 32) matches a random 80 % of them, 5 % of each pair's matches are replaced by wrong ones and a random 10 % are
switched off through keep; policy 'views', min_views 2, cap = K / 2.  Beside it the Python restatement of the same rules
(tests/tracks_oracle.py) and scipy's connected components of the live matches (the partition alone), once each on the same host.

Device times: HIP events around `--iters` calls after `--warmup` (inputs and outputs on the device, allocated once), median over
`--rounds` rounds (min / max shown).  Host times once each, host clock.  Every device output is compared with the restatement.
GPU box:  python tools/bench_tracks.py [--out profiles/tracks_bench.txt]
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
from tests import tracks_oracle as to

SHAPES = ((8, 2048), (32, 2048), (32, 8192))


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


def p(x):
    return ctypes.c_void_p(x.data_ptr())


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def graph(V, n, seed):
    rng = np.random.default_rng(seed)
    inv = [np.argsort(rng.permutation(n)) for _ in range(V)]       # point -> keypoint of view v
    offsets = (np.arange(V + 1) * n).astype(np.int32)
    matches, pairs = [], 0
    for i in range(V):
        for j in range(i + 1, min(V, i + 3)):
            pts = np.nonzero(rng.random(n) < 0.8)[0]
            m = np.stack([inv[i][pts], inv[j][pts]], axis=1)
            bad = rng.random(len(pts)) < 0.05
            m[bad, 1] = (m[bad, 1] + 1 + rng.integers(0, n - 1, size=int(bad.sum()))) % n
            matches.append(m + offsets[[i, j]])
            pairs += 1
    matches = np.concatenate(matches).astype(np.int32)
    keep = (rng.random(len(matches)) >= 0.1).astype(np.uint8)
    return offsets, matches, keep, rng.normal(size=(V * n, 2)) * 100, pairs


def bench(V, n, a):
    offsets, matches, keep, kp, pairs = graph(V, n, V + n)
    K, M, cap = V * n, len(matches), V * n // 2
    lib = _lib.load_library()
    count = ctypes.c_size_t()
    assert lib.cotr_build_tracks_work_ints(K, M, ctypes.byref(count)) == 0
    d_off, d_m, d_keep, d_kp = dev(offsets), dev(matches), dev(keep), dev(kp)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device='cuda')   # noqa: E731
    ton, node, info, work = i32(K), i32(V, cap), i32(8), i32(count.value)
    vis, pts = torch.empty((V, cap), dtype=torch.uint8, device='cuda'), torch.empty((V, cap, 2), dtype=torch.float64, device='cuda')
    stream = _lib.current_stream_ptr()

    def call():
        assert lib.cotr_build_tracks(p(d_off), p(d_m), p(d_keep), p(d_kp), V, K, M, 2, 1, cap, p(ton), p(node), p(vis), p(pts), p(info), p(work), stream) == 0
    t = timed(call, a.warmup, a.iters, a.rounds)
    torch.cuda.synchronize()
    gi = info.cpu().numpy()
    line = (f'V={V}, {n} keypoints per view, {pairs} pairs: K={K}, M={M}, cap={cap}: cotr_build_tracks {t[0]:.4f} ms ({t[1]:.4f} / {t[2]:.4f}), 7 launches, '
            f'work {count.value * 4 / 2**20:.2f} MiB; info {gi.tolist()}')
    if not a.no_host:
        c0 = time.perf_counter()
        want = to.build_tracks(offsets, matches, keep=keep, keypoints=kp, conflict=1, cap=cap)
        host = (time.perf_counter() - c0) * 1e3
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        c0 = time.perf_counter()
        e = matches[keep != 0]
        ncomp, _ = connected_components(coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(K, K)), directed=False)
        sci = (time.perf_counter() - c0) * 1e3
        got = dict(track_of_node=ton, node=node, visible=vis, points=pts, info=info)
        same = all(np.array_equal(got[k].cpu().numpy(), want[k], equal_nan=True) for k in got)
        line += f'; Python restatement on the host {host:.0f} ms, scipy connected_components (the partition alone) {sci:.1f} ms; every output equal: {same}'
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-host', action='store_true', help='skip the restatement and scipy')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tracks_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_tracks.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls; host times once, host clock']
    for V, n in SHAPES:
        lines += bench(V, n, a)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
