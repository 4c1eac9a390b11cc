"""3D-3D registration timings: cotr_ransac_rigid3d (cotr_amd/csrc/rigid3d.hip) at n = 300, 2048, 8192 with max_iters = 1000
(a 4-unit cloud, 40 % outliers, noise 0.01, threshold 0.04), rigid and with a scale, with two refit rounds and with none, and
the numpy restatement of the same rules (tests/rigid3d_oracle.py) on the same host.  The device evaluates all 1000 candidates
whatever the early stop.

Device times: HIP events around `--iters` calls after `--warmup` (inputs on the device, scratch allocated once), median over
`--rounds` rounds (min / max shown).  Host times once each, host clock.  Every device result is checked against the
restatement.
GPU box:  python tools/bench_rigid3d.py [--out profiles/rigid3d_bench.txt]
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
from cotr_amd.inference.rigid3d import ransac_rigid3d
from tests import rigid3d_oracle as go


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


def bench(n, ws, a, iters=1000, thr=0.04, conf=0.99):
    src, dst, R, t, s, _ = go.rigid_scene(n, 0.4, n, 0.01, ws)
    d1, d2 = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    lib = _lib.load_library()
    nb = ctypes.c_size_t()
    assert lib.cotr_ransac_rigid3d_scratch_bytes(n, iters, ctypes.byref(nb)) == 0
    s1 = torch.empty(nb.value, dtype=torch.uint8, device='cuda')
    Rd, td, sd = (torch.empty(k, dtype=torch.float64, device='cuda') for k in (9, 3, 1))
    mask = torch.empty(n, dtype=torch.uint8, device='cuda')
    info = torch.empty(8, dtype=torch.int32, device='cuda')
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    stream = _lib.current_stream_ptr()

    def call(rounds):
        assert lib.cotr_ransac_rigid3d(p(d1), p(d2), n, thr, conf, iters, 0, int(ws), rounds, p(Rd), p(td), p(sd), p(mask), p(info), None, None, None,
                                       p(s1), nb.value, stream) == 0
    t2 = timed(lambda: call(2), a.warmup, a.iters, a.rounds)
    t0 = timed(lambda: call(0), a.warmup, a.iters, a.rounds)
    r = {k: v.cpu().numpy() for k, v in ransac_rigid3d(src, dst, thr, conf, iters, 0, ws, 2, hypotheses=True).items()}
    cnt = r['hyp_count']
    ok = np.array_equal(go.counts(r['hyp_model'], cnt >= 0, src, dst, thr, ws), cnt) and tuple(int(v) for v in r['info'][:4]) == go.select(cnt, iters, n, conf)
    c0 = time.perf_counter()
    o = go.ransac(src, dst, thr, conf, iters, 0, ws, 2)
    host = (time.perf_counter() - c0) * 1e3
    differ = sum(1 for it in range(iters) if (cnt[it] >= 0) != o['has'][it] or
                 (o['has'][it] and go.candidate_distance(r['hyp_model'][it], o['hyp_model'][it], ws) > 1e-7))
    i = r['info']
    e = go.scene_errors(r['R'], r['t'], r['scale'][0], dict(R=R, t=t, s=s))
    return [f'n={n}, max_iters={iters}, {"similarity" if ws else "rigid"}: cotr_ransac_rigid3d with 2 refit rounds (14 launches) {t2[0]:.4f} ms '
            f'({t2[1]:.4f} / {t2[2]:.4f}), with none (4 launches) {t0[0]:.4f} ms ({t0[1]:.4f} / {t0[2]:.4f}); {int((cnt >= 0).sum())} candidates, best {i[1]}, '
            f'{i[2]} sequential iterations, {i[4]} rounds run, {i[5]} points in the mask',
            f'    counts and selection identical to numpy: {ok}; mask identical to the restatement: {np.array_equal(r["mask"], o["mask"])}; iterations '
            f'whose candidate differs from the restatement by more than 1e-7: {differ} of {iters}; refit against the restatement: '
            f'{go.model_distance(r["scale"][0] * r["R"], r["t"], o["scale"] * o["R"], o["t"]):.1e}; against the scene: rotation {e[0]:.2e}, '
            f'translation {e[1]:.2e}, scale {e[2]:.2e}',
            f'    host, numpy restatement, all {iters} iterations and 2 rounds: {host:.0f} ms']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rigid3d_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_rigid3d.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls; host times once, host clock']
    for n in (300, 2048, 8192):
        for ws in (False, True):
            lines += bench(n, ws, a)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
