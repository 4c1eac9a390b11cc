"""Times the device batch builders of cotr_amd/data.py on the GPU against the numpy oracle on the CPU:
make_zoom_batch at 16 samples x num_kp 100 (the shape of the recorded training step), depth_corrs alone at 16 x 256 x 256,
and tests/dataset_oracle.py for the same 16 samples.  Host clock around work that ends in a device synchronise; the
captures are uploaded once, outside the timed window (a loader would keep them on the device).

    python tools/bench_dataset.py [--samples 16] [--num-kp 100] [--iters 50] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cotr_amd import data  # noqa: E402
from cotr_amd.utils.synth import synth_captures  # noqa: E402
from tests import dataset_oracle as oracle  # noqa: E402


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--num-kp', type=int, default=100)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    zooms = np.logspace(0.0, -1.0, 10)
    pairs = [synth_captures(100 + i, 480, 640) for i in range(a.samples)]
    small = [synth_captures(200 + i, 256, 256) for i in range(a.samples)]
    up = lambda c: data.Capture(torch.from_numpy(c.image).cuda(), torch.from_numpy(c.depth).cuda(), c.K, c.c2w)   # noqa: E731
    qs, ns = [up(p[0]) for p in pairs], [up(p[1]) for p in pairs]
    sq, sn = [up(p[0]) for p in small], [up(p[1]) for p in small]
    rng = np.random.default_rng(0)
    rand = {'seed': rng.random((a.samples, 100)), 'zoom': rng.random(a.samples), 'jitter': rng.random((a.samples, 2)),
            'trim': rng.random((a.samples, a.num_kp)), 'flip': rng.random(a.samples)}
    drand = {k: torch.from_numpy(v).cuda() for k, v in rand.items()}
    lines = [f'device: {torch.cuda.get_device_name(0)}; {a.samples} samples, num_kp {a.num_kp}, captures 480 x 640, {a.iters} timed calls each']
    out = data.make_zoom_batch(qs, ns, a.num_kp, zooms, 0.125, rand=drand)
    lines.append(f'valid samples: {int(out["valid"].sum())} of {a.samples}')
    for name, fn in (('make_zoom_batch (bidirectional, 480 x 640 captures)', lambda: data.make_zoom_batch(qs, ns, a.num_kp, zooms, 0.125, rand=drand)),
                     ('make_batch (256 x 256 captures)', lambda: data.make_batch(sq, sn, a.num_kp, rand=drand)),
                     ('depth_corrs alone, 16 x 256 x 256', lambda: data.depth_corrs(sq, sn))):
        med, lo, hi = timed(fn, a.iters)
        lines.append(f'{name}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})')
    t0 = time.perf_counter()
    oracle.make_zoom_batch([p[0] for p in pairs], [p[1] for p in pairs], a.num_kp, zooms, 0.125, True, rand)
    lines.append(f'numpy oracle, make_zoom_batch for the same samples, one CPU core: {(time.perf_counter() - t0) * 1e3:.1f} ms')
    t0 = time.perf_counter()
    for q, n in small:
        oracle.reproject(q.depth, n.depth, q.K, q.c2w, n.K, n.c2w)
    lines.append(f'numpy oracle, depth reprojection 16 x 256 x 256: {(time.perf_counter() - t0) * 1e3:.1f} ms')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
