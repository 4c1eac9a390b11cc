"""Relative-pose refit timings: cotr_refine_pose (cotr_amd/csrc/essential.hip) at n = 300, 2048, 8192 with
rounds = 1 and 4 of 10 steps, after cotr_ransac_essential + cotr_recover_pose with max_iters = 1000 (two-view scene, 40 %
outliers, 1 px noise, 1 px threshold): the refit alone, the three calls back to back against the two without it, the numpy
restatement of the refit (tests/pose_refit_oracle.py) on the same host, and the pose errors against the scene before and after.

Device times: HIP events around `--iters` calls after `--warmup` (inputs on the device, scratch allocated once), median over
`--rounds` rounds (min / max shown).  Host times once each, host clock.  Every device result is checked against the
restatement started from the device's own RANSAC pose.
GPU box:  python tools/bench_pose_refit.py [--out profiles/pose_refit_bench.txt]
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
from tests import essential_oracle as eo
from tests import pose_refit_oracle as po


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


def bench(n, a, iters=1000, steps=10):
    p1, p2, K1, K2, R, t, _ = eo.two_view_scene(n, 0.4, n, 1.0)
    d1, d2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
    lib = _lib.load_library()
    nb, nbp, nbr = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.cotr_ransac_essential_scratch_bytes(n, iters, ctypes.byref(nb)) == 0
    assert lib.cotr_recover_pose_scratch_bytes(n, ctypes.byref(nbp)) == 0
    assert lib.cotr_refine_pose_scratch_bytes(n, ctypes.byref(nbr)) == 0
    s1, s2, s3 = (torch.empty(b.value, dtype=torch.uint8, device='cuda') for b in (nb, nbp, nbr))
    E, Rd, td, Rr, tr, Er = (torch.empty(k, dtype=torch.float64, device='cuda') for k in (9, 9, 3, 9, 3, 9))
    mask, mask2, mask3 = (torch.empty(n, dtype=torch.uint8, device='cuda') for _ in range(3))
    info, info2, info3 = (torch.empty(8, dtype=torch.int32, device='cuda') for _ in range(3))
    K9 = ctypes.c_double * 9
    k1, k2 = K9(*K1.reshape(9)), K9(*K2.reshape(9))
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    stream = _lib.current_stream_ptr()

    def pose():
        assert lib.cotr_ransac_essential(p(d1), p(d2), n, k1, k2, 1.0, 0.999, iters, 0, p(E), p(mask), p(info), None, None, None, p(s1),
                                         nb.value, stream) == 0
        assert lib.cotr_recover_pose(p(E), p(d1), p(d2), n, k1, k2, 50.0, p(mask), p(info), p(Rd), p(td), p(mask2), p(info2), p(s2),
                                     nbp.value, stream) == 0

    def refit(rounds):
        assert lib.cotr_refine_pose(p(Rd), p(td), p(d1), p(d2), n, k1, k2, 1.0, 50.0, rounds, steps, p(mask2), p(info), p(Rr), p(tr), p(Er),
                                    p(mask3), p(info3), p(s3), nbr.value, stream) == 0

    def both(rounds):
        pose()
        refit(rounds)
    tp = timed(pose, a.warmup, a.iters, a.rounds)
    pose()
    torch.cuda.synchronize()
    R0, t0, m0 = Rd.cpu().numpy().reshape(3, 3), td.cpu().numpy(), mask2.cpu().numpy().astype(bool)
    lines = [f'n={n}, max_iters={iters}, {steps} steps a round: cotr_ransac_essential + cotr_recover_pose {tp[0]:.4f} ms ({tp[1]:.4f} / {tp[2]:.4f}); '
             f'their pose against the scene: rotation {eo.rotation_error_deg(R0, R):.3f} deg, translation direction {eo.direction_error_deg(t0, t):.3f} deg, '
             f'{m0.sum()} points in its mask']
    for rounds in (1, 4):
        tr_ = timed(lambda: refit(rounds), a.warmup, a.iters, a.rounds)
        tb = timed(lambda: both(rounds), a.warmup, a.iters, a.rounds)
        refit(rounds)
        torch.cuda.synchronize()
        Rg, tg, mg, ig = Rr.cpu().numpy().reshape(3, 3), tr.cpu().numpy(), mask3.cpu().numpy().astype(bool), info3.cpu().numpy()
        c0 = time.perf_counter()
        want = po.refine(R0, t0, p1, p2, K1, K2, m0, 1.0, 50.0, rounds, steps)
        host = (time.perf_counter() - c0) * 1e3
        d = max(np.abs(Rg - want['R']).max(), np.abs(tg - want['t']).max())
        lines += [f'    rounds={rounds}: cotr_refine_pose {tr_[0]:.4f} ms ({tr_[1]:.4f} / {tr_[2]:.4f}), {2 + rounds * (1 + 2 * (steps + 1))} launches; '
                  f'the three calls back to back {tb[0]:.4f} ms ({tb[1]:.4f} / {tb[2]:.4f}); host, numpy restatement of the refit: {host:.0f} ms',
                  f'        against the scene: rotation {eo.rotation_error_deg(Rg, R):.3f} deg, translation direction {eo.direction_error_deg(tg, t):.3f} deg '
                  f'(restatement {eo.rotation_error_deg(want["R"], R):.3f} / {eo.direction_error_deg(want["t"], t):.3f}); info {[int(v) for v in ig[:6]]} '
                  f'(restatement {[int(v) for v in want["info"][:6]]}); R, t within {d:.1e} of the restatement, mask identical: '
                  f'{np.array_equal(mg, want["mask"])}']
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pose_refit_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_pose_refit.py measures the GPU: no device found'
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
