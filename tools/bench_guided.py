"""Guided-matching timings: the two device calls of cotr_amd.inference.guided at the demo's sizes, and the host recipes they
replace.

  mutual_matches:        cotr_nearest_mutual at 2048 x 2048 (the reference's DISK keypoint files) and 8192 x 8192 (random)
  find_fundamental_mat:  cotr_ransac_fundamental at n = 300, 2048, 8192 with max_iters = 1000 (two-view scene, 40 % outliers,
                         3 px); the device evaluates all 3 * max_iters candidate slots whatever the early stop

Device times: HIP events around `--iters` calls after `--warmup` (inputs on the device, scratch allocated once), median over
`--rounds` rounds (min / max shown).  Host times, once each, host clock: the reference's recipe (scipy distance_matrix + argmin
both ways, then the demo's double loop) at 2048, and the numpy restatement's RANSAC (tests/guided_oracle.py) as a stand-in for
cv2.findFundamentalMat, which is not installed.  Every device result is checked against the restatement.
GPU box:  python tools/bench_guided.py [--out profiles/guided_bench.txt]
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
from cotr_amd.inference.guided import nearest_mutual, ransac_fundamental
from tests import guided_oracle as go


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


def nn_inputs(n, seed):
    rng = np.random.default_rng(seed)
    if n == 2048:
        g = os.path.join(ROOT, 'tests', 'golden')
        kp_a = np.load(os.path.join(g, '21526113_4379776807.jpg.disk.kpts.npy')).astype(np.float64)
        kp_b = np.load(os.path.join(g, '21126421_4537535153.jpg.disk.kpts.npy')).astype(np.float64)
    else:
        kp_a, kp_b = rng.uniform(0, 1024, (n, 2)), rng.uniform(0, 768, (n, 2))
    pred_ab = kp_b[rng.permutation(n)] + rng.normal(0, 2, (n, 2))
    pred_ba = kp_a[rng.permutation(n)] + rng.normal(0, 2, (n, 2))
    return pred_ab, kp_b, pred_ba, kp_a


def bench_nearest(n, a):
    pred_ab, kp_b, pred_ba, kp_a = nn_inputs(n, n)
    dev = [torch.from_numpy(x).cuda() for x in (pred_ab, kp_b, pred_ba, kp_a)]
    lib = _lib.load_library()
    nbytes = ctypes.c_size_t()
    assert lib.cotr_nearest_mutual_scratch_bytes(n, n, ctypes.byref(nbytes)) == 0
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device='cuda')
    outs = [torch.empty(n, dtype=torch.int32, device='cuda'), torch.empty(n, dtype=torch.int32, device='cuda'),
            torch.empty(n, dtype=torch.uint8, device='cuda')]
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = _lib.current_stream_ptr()

    def call():
        assert lib.cotr_nearest_mutual(*[p(t) for t in dev], n, n, *[p(t) for t in outs], p(scratch), nbytes.value, stream) == 0
    t = timed(call, a.warmup, a.iters, a.rounds)
    idx_ab, idx_ba, _ = nearest_mutual(pred_ab, kp_b, pred_ba, kp_a)
    ok = np.array_equal(idx_ab.cpu().numpy(), go.nearest(pred_ab, kp_b)) and np.array_equal(idx_ba.cpu().numpy(), go.nearest(pred_ba, kp_a))
    line = f'nearest + mutual {n} x {n}: cotr_nearest_mutual {t[0]:.4f} ms ({t[1]:.4f} / {t[2]:.4f}); indices identical to numpy: {ok}'
    host = []
    try:
        from scipy.spatial import distance_matrix
        t0 = time.perf_counter()
        ia = np.argmin(distance_matrix(pred_ab, kp_b), axis=1)
        ib = np.argmin(distance_matrix(pred_ba, kp_a), axis=1)
        t1 = time.perf_counter()
        host.append(f'    host, scipy distance_matrix + argmin both ways: {(t1 - t0) * 1e3:.0f} ms')
        if n <= 2048:
            t0 = time.perf_counter()
            go.demo_double_loop(ia, ib)
            host.append(f'    host, the demo\'s mutual double loop: {(time.perf_counter() - t0) * 1e3:.0f} ms')
        else:
            host.append('    host, the demo\'s mutual double loop: not run (O(Na x Nb) Python iterations)')
    except ImportError:
        host.append('    host, scipy recipe: not measured (scipy is not installed)')
    return [line] + host


def bench_ransac(n, a, iters=1000):
    p1, p2, _, _ = go.two_view_scene(n, 0.4, n)
    d1, d2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
    lib = _lib.load_library()
    nbytes = ctypes.c_size_t()
    assert lib.cotr_ransac_fundamental_scratch_bytes(n, iters, ctypes.byref(nbytes)) == 0
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device='cuda')
    F = torch.empty(9, dtype=torch.float64, device='cuda')
    mask = torch.empty(n, dtype=torch.uint8, device='cuda')
    info = torch.empty(4, dtype=torch.int32, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = _lib.current_stream_ptr()

    def call():
        assert lib.cotr_ransac_fundamental(p(d1), p(d2), n, 3.0, 0.99, iters, 0, p(F), p(mask), p(info), None, None, None,
                                           p(scratch), nbytes.value, stream) == 0
    t = timed(call, a.warmup, a.iters, a.rounds)
    r = ransac_fundamental(p1, p2, 3.0, 0.99, iters, 0, hypotheses=True)
    cnt = r['hyp_count'].cpu().numpy()
    ok = np.array_equal(go.counts(r['hyp_F'].cpu().numpy(), p1, p2, 3.0), cnt) and \
        tuple(int(v) for v in r['info'].cpu()) == go.select(cnt, iters, n, 0.99)
    slots = int((cnt >= 0).sum())
    rate = slots * n / (t[0] * 1e-3)
    t0 = time.perf_counter()
    go.ransac(p1, p2, 3.0, 0.99, iters, 0)
    host = (time.perf_counter() - t0) * 1e3
    info = r['info'].cpu().numpy()
    return [f'RANSAC n={n}, max_iters={iters}: cotr_ransac_fundamental {t[0]:.4f} ms ({t[1]:.4f} / {t[2]:.4f}); {slots} candidates, '
            f'{rate / 1e9:.2f} G error evaluations/s over the whole call; best {info[1]}, {info[2]} sequential iterations; '
            f'counts and selection identical to numpy: {ok}',
            f'    host, numpy restatement (stand-in for cv2.findFundamentalMat, not installed), all {iters} iterations: {host:.0f} ms']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'guided_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_guided.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls; host times once, host clock']
    for n in (2048, 8192):
        lines += bench_nearest(n, a)
    for n in (300, 2048, 8192):
        lines += bench_ransac(n, a)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
