"""Relative-pose timings: cotr_ransac_essential and cotr_recover_pose (cotr_amd/csrc/essential.hip) at n = 300, 2048, 8192
with max_iters = 1000 (two-view scene, 40 % outliers, 1 px noise, 1 px threshold), the two calls apart and back to back, and
the numpy restatement of the same rules (tests/essential_oracle.py) on the same host as a stand-in for cv2.findEssentialMat +
cv2.recoverPose, which are not installed.  The device evaluates all ~4500 candidates whatever the early stop.

Device times: HIP events around `--iters` calls after `--warmup` (inputs on the device, scratch allocated once), median over
`--rounds` rounds (min / max shown).  Host times once each, host clock.  Every device result is checked against the
restatement.
GPU box:  python tools/bench_essential.py [--out profiles/essential_bench.txt]
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
from cotr_amd.inference.essential import pose_of_essential, ransac_essential
from tests import essential_oracle as eo


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


def bench(n, a, iters=1000):
    p1, p2, K1, K2, R, t, _ = eo.two_view_scene(n, 0.4, n, 1.0)
    d1, d2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
    lib = _lib.load_library()
    nb, nbp = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.cotr_ransac_essential_scratch_bytes(n, iters, ctypes.byref(nb)) == 0
    assert lib.cotr_recover_pose_scratch_bytes(n, ctypes.byref(nbp)) == 0
    s1 = torch.empty(nb.value, dtype=torch.uint8, device='cuda')
    s2 = torch.empty(nbp.value, dtype=torch.uint8, device='cuda')
    E, Rd, td = (torch.empty(k, dtype=torch.float64, device='cuda') for k in (9, 9, 3))
    mask, mask2 = (torch.empty(n, dtype=torch.uint8, device='cuda') for _ in range(2))
    info, info2 = (torch.empty(8, dtype=torch.int32, device='cuda') for _ in range(2))
    K9 = ctypes.c_double * 9
    k1, k2 = K9(*K1.reshape(9)), K9(*K2.reshape(9))
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    stream = _lib.current_stream_ptr()

    def essential():
        assert lib.cotr_ransac_essential(p(d1), p(d2), n, k1, k2, 1.0, 0.999, iters, 0, p(E), p(mask), p(info), None, None, None, p(s1),
                                         nb.value, stream) == 0

    def pose():
        assert lib.cotr_recover_pose(p(E), p(d1), p(d2), n, k1, k2, 50.0, p(mask), p(info), p(Rd), p(td), p(mask2), p(info2), p(s2),
                                     nbp.value, stream) == 0

    def both():
        essential()
        pose()
    te = timed(essential, a.warmup, a.iters, a.rounds)
    tp = timed(pose, a.warmup, a.iters, a.rounds)
    tb = timed(both, a.warmup, a.iters, a.rounds)
    r = {k: v.cpu().numpy() for k, v in ransac_essential(p1, p2, K1, K2, 1.0, 0.999, iters, 0, hypotheses=True).items()}
    xn1, xn2, sthr = eo.normalise(p1, K1), eo.normalise(p2, K2), eo.scaled_threshold(1.0, K1, K2)
    cnt = r['hyp_count']
    ok = np.array_equal(eo.counts(r['hyp_E'], cnt >= 0, xn1, xn2, sthr), cnt) and tuple(int(v) for v in r['info'][:4]) == eo.select(cnt, iters, n, 0.999)
    q = {k: v.cpu().numpy() for k, v in pose_of_essential(r['E'], p1, p2, K1, K2, r['mask']).items()}
    want = eo.recover_pose(r['E'].reshape(9), p1, p2, K1, K2, r['mask'])
    ok_pose = np.array_equal(q['info'], want['info']) and np.array_equal(q['mask'], want['mask'])
    c0 = time.perf_counter()
    o = eo.ransac(p1, p2, K1, K2, 1.0, 0.999, iters, 0)
    eo.recover_pose(o['E'], p1, p2, K1, K2, o['mask'])
    host = (time.perf_counter() - c0) * 1e3
    differ = sum(eo.set_distance([r['hyp_E'][10 * it + k] for k in range(int((cnt[10 * it:10 * it + 10] >= 0).sum()))],
                                 [o['hyp_E'][10 * it + k] for k in range(o['ncand'][it])]) > 1e-7 for it in range(iters))
    i = r['info']
    return [f'n={n}, max_iters={iters}: cotr_ransac_essential {te[0]:.4f} ms ({te[1]:.4f} / {te[2]:.4f}), cotr_recover_pose {tp[0]:.4f} ms '
            f'({tp[1]:.4f} / {tp[2]:.4f}), both back to back {tb[0]:.4f} ms ({tb[1]:.4f} / {tb[2]:.4f}); {int((cnt >= 0).sum())} candidates, '
            f'best {i[1]}, {i[2]} sequential iterations, {q["info"][0]} points in front of candidate {q["info"][1]}',
            f'    counts and selection identical to numpy: {ok}; pose counts and mask identical to numpy: {ok_pose}, R within '
            f'{np.abs(q["R"] - want["R"]).max():.1e}; iterations whose candidates differ from the restatement by more than 1e-7: {differ} of {iters}; '
            f'against the scene: rotation {eo.rotation_error_deg(q["R"], R):.3f} deg, translation direction {eo.direction_error_deg(q["t"], t):.3f} deg',
            f'    host, numpy restatement (stand-in for cv2.findEssentialMat + cv2.recoverPose, not installed), all {iters} iterations: {host:.0f} ms']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'essential_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_essential.py measures the GPU: no device found'
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
