"""Absolute-pose timings: cotr_ransac_pnp (cotr_amd/csrc/pnp.hip) at n = 300, 2048, 8192 with max_iters = 1000 (a posed
scene, 40 % outliers, 1 px noise, 3 px threshold), with 10 refinement steps and with none, cotr_lift_pixels on the same number
of points of a 480 x 640 depth map, the two back to back, and the numpy restatement of the same rules (tests/pnp_oracle.py)
on the same host as a stand-in for cv2.solvePnPRansac, which is not installed.  The device evaluates all 1000 candidates
whatever the early stop.

Device times: HIP events around `--iters` calls after `--warmup` (inputs on the device, scratch allocated once), median over
`--rounds` rounds (min / max shown).  Host times once each, host clock.  Every device result is checked against the
restatement.
GPU box:  python tools/bench_pnp.py [--out profiles/pnp_bench.txt]
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
from cotr_amd.inference.pnp import ransac_pnp
from tests import pnp_oracle as po


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


def bench(n, a, iters=1000, thr=3.0, conf=0.99):
    obj, img, K, R, t, _ = po.pnp_scene(n, 0.4, n, 1.0)
    d1, d2 = torch.from_numpy(obj).cuda(), torch.from_numpy(img).cuda()
    rng = np.random.default_rng(n)
    depth = torch.from_numpy(rng.uniform(2, 9, (480, 640)).astype(np.float32)).cuda()
    pix = torch.from_numpy(rng.uniform([0, 0], [639, 479], (n, 2))).cuda()
    c2w = torch.from_numpy(po.pose_matrix((5.0, -3.0, 2.0), (0.3, 0.1, -0.2)).reshape(16)).cuda()
    lifted = torch.empty((n, 3), dtype=torch.float64, device='cuda')
    lib = _lib.load_library()
    nb = ctypes.c_size_t()
    assert lib.cotr_ransac_pnp_scratch_bytes(n, iters, ctypes.byref(nb)) == 0
    s1 = torch.empty(nb.value, dtype=torch.uint8, device='cuda')
    Rd, td = (torch.empty(k, dtype=torch.float64, device='cuda') for k in (9, 3))
    mask = torch.empty(n, dtype=torch.uint8, device='cuda')
    info = torch.empty(8, dtype=torch.int32, device='cuda')
    k9 = (ctypes.c_double * 9)(*K.reshape(9))
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    stream = _lib.current_stream_ptr()

    def pnp(refine, points=d1):
        assert lib.cotr_ransac_pnp(p(points), p(d2), n, k9, thr, conf, iters, 0, refine, p(Rd), p(td), p(mask), p(info), None, None, None, p(s1),
                                   nb.value, stream) == 0

    def lift():
        assert lib.cotr_lift_pixels(p(depth), 480, 640, k9, p(c2w), p(pix), n, p(lifted), stream) == 0

    def both():
        lift()
        pnp(10, lifted)
    t10 = timed(lambda: pnp(10), a.warmup, a.iters, a.rounds)
    t0 = timed(lambda: pnp(0), a.warmup, a.iters, a.rounds)
    tl = timed(lift, a.warmup, a.iters, a.rounds)
    tb = timed(both, a.warmup, a.iters, a.rounds)
    r = {k: v.cpu().numpy() for k, v in ransac_pnp(obj, img, K, thr, conf, iters, 0, 10, hypotheses=True).items()}
    cnt = r['hyp_count']
    ok = np.array_equal(po.counts(r['hyp_pose'], cnt >= 0, obj, img, K, thr), cnt) and tuple(int(v) for v in r['info'][:4]) == po.select(cnt, iters, n, conf)
    ok_lift = np.array_equal(lifted.cpu().numpy(), po.lift(pix.cpu().numpy(), depth.cpu().numpy(), K, c2w.cpu().numpy().reshape(4, 4)), equal_nan=True)
    c0 = time.perf_counter()
    o = po.ransac(obj, img, K, thr, conf, iters, 0)
    host = (time.perf_counter() - c0) * 1e3
    differ = sum(1 for it in range(iters) if (cnt[it] >= 0) != o['has'][it] or (o['has'][it] and po.pose_distance(r['hyp_pose'][it], o['hyp_pose'][it]) > 1e-7))
    i = r['info']
    return [f'n={n}, max_iters={iters}: cotr_ransac_pnp with 10 refinement steps {t10[0]:.4f} ms ({t10[1]:.4f} / {t10[2]:.4f}), with none {t0[0]:.4f} ms '
            f'({t0[1]:.4f} / {t0[2]:.4f}), cotr_lift_pixels {tl[0]:.4f} ms ({tl[1]:.4f} / {tl[2]:.4f}), lift and pnp back to back {tb[0]:.4f} ms '
            f'({tb[1]:.4f} / {tb[2]:.4f}); {int((cnt >= 0).sum())} candidates, best {i[1]}, {i[2]} sequential iterations, {i[4]} refit steps kept',
            f'    counts and selection identical to numpy: {ok}; lift identical to numpy: {ok_lift}; iterations whose candidate differs from the '
            f'restatement by more than 1e-7: {differ} of {iters}; refit against the restatement: R {np.abs(r["R"] - o["R"]).max():.1e}, '
            f't {np.abs(r["t"] - o["t"]).max() / np.linalg.norm(o["t"]):.1e}; against the scene: rotation {po.rotation_error(r["R"], R):.2e}, '
            f'translation {po.translation_error(r["t"], t):.2e}',
            f'    host, numpy restatement (stand-in for cv2.solvePnPRansac, not installed), all {iters} iterations: {host:.0f} ms']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pnp_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_pnp.py measures the GPU: no device found'
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
