"""Homography timings: cotr_ransac_homography (cotr_amd/csrc/homography.hip) at n = 300, 2048, 8192 with max_iters = 2000
(planar scene, 40 % outliers, 1 px noise, 3 px threshold), with the default 10 refinement steps and with none, and the numpy
restatement of the same rules (tests/homography_oracle.py) on the same host as a stand-in for cv2.findHomography, which is
not installed.  The device evaluates all max_iters candidates whatever the early stop, and the refit chain has a fixed length.

Device times: HIP events around `--iters` calls after `--warmup` (inputs on the device, scratch allocated once), median over
`--rounds` rounds (min / max shown).  Host times once each, host clock.  Every device result is checked against the
restatement.
GPU box:  python tools/bench_homography.py [--out profiles/homography_bench.txt]
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
from cotr_amd.inference.homography import ransac_homography
from tests import homography_oracle as ho


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


def bench(n, a, iters=2000):
    p1, p2, _, Ht = ho.planar_scene(n, 0.4, n, 1.0)
    d1, d2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
    lib = _lib.load_library()
    nbytes = ctypes.c_size_t()
    assert lib.cotr_ransac_homography_scratch_bytes(n, iters, ctypes.byref(nbytes)) == 0
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device='cuda')
    H = torch.empty(9, dtype=torch.float64, device='cuda')
    mask = torch.empty(n, dtype=torch.uint8, device='cuda')
    info = torch.empty(8, dtype=torch.int32, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = _lib.current_stream_ptr()

    def call(refine):
        assert lib.cotr_ransac_homography(p(d1), p(d2), n, 3.0, 0.995, iters, refine, 0, p(H), p(mask), p(info), None, None, None,
                                          None, p(scratch), nbytes.value, stream) == 0
    t10 = timed(lambda: call(10), a.warmup, a.iters, a.rounds)
    t0 = timed(lambda: call(0), a.warmup, a.iters, a.rounds)
    r = {k: v.cpu().numpy() for k, v in ransac_homography(p1, p2, 3.0, 0.995, iters, 0, hypotheses=True).items()}
    cnt = r['hyp_count']
    ok = np.array_equal(ho.counts(r['hyp_H'], cnt >= 0, p1, p2, 3.0), cnt) and tuple(int(v) for v in r['info'][:4]) == ho.select(cnt, iters, n, 0.995)
    ref = ho.refit(p1, p2, r['mask'], 10, r['H_ransac'].reshape(9))[0]
    c0 = time.perf_counter()
    ho.ransac(p1, p2, 3.0, 0.995, iters, 0)
    host = (time.perf_counter() - c0) * 1e3
    i = r['info']
    return [f'n={n}, max_iters={iters}: cotr_ransac_homography {t10[0]:.4f} ms ({t10[1]:.4f} / {t10[2]:.4f}) with 10 refinement steps, '
            f'{t0[0]:.4f} ms ({t0[1]:.4f} / {t0[2]:.4f}) with none; {int((cnt >= 0).sum())} candidates, best {i[1]}, {i[2]} sequential '
            f'iterations, {i[4]} steps kept',
            f'    counts and selection identical to numpy: {ok}; refit against the restatement on the same mask: '
            f'{ho.corner_error(r["H"], ref, p1):.1e} px at the corners; corner error against the scene: H_ransac '
            f'{ho.corner_error(r["H_ransac"], Ht, p1):.2f} px, refit {ho.corner_error(r["H"], Ht, p1):.2f} px',
            f'    host, numpy restatement (stand-in for cv2.findHomography, not installed), all {iters} iterations: {host:.0f} ms']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'homography_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_homography.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls; host times once, host clock']
    for n in (300, 2048, 8192):
        lines += bench(n, a)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
