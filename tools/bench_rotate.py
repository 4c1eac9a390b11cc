"""Rotation-augmentation timings: cotr_rotate_captures on 32 captures of 480 x 640 - the 2B captures of the
16-sample batch of 3j - with image + depth and with depth only, and make_zoom_batch at 3j's shape with and without
``rotations``.

  kernel   HIP events around `--iters` calls of the C entry point (tables and destinations made once), median over `--rounds`
           rounds (min / max shown).  Every call works on the next of N sets of buffers (sources and destinations), N chosen so
           that the sets together exceed 320 MiB: the 256 MiB Infinity Cache cannot serve a repeat, the figures are HBM figures.
           Bytes moved are computed from the shapes: every source once, every destination in full; the bound is that figure
           over the 8 TB/s HBM peak (about 6.3 TB/s is achievable).  The result of set 0 is checked against the restatement
           (tests/rotate_oracle.py), whose own host time is taken once: it stands in for cv2, which is not installed.
  wrapper  data.rotate_captures for the same captures, host clock around a call that ends in a device synchronise: the table
           upload and the 64 allocations included.
  batch    make_zoom_batch, 16 samples x num_kp 100, bidirectional, 480 x 640 captures already on the device, uniforms passed
           in: without ``rotations`` and with all 32 captures turned, alternating call by call in one process; host clock
           around a call that ends in a device synchronise, 5 warm-up and `--batch-iters` timed calls each.
GPU box:  python tools/bench_rotate.py [--out profiles/rotate_bench.txt]
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

from cotr_amd import _lib, data
from cotr_amd.utils.synth import synth_captures
from tests import rotate_oracle as ro

HBM_PEAK = 8.0e12
CACHE = 320 << 20          # rotate over more bytes than the 256 MiB Infinity Cache holds
H, W = 480, 640


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def make_set(caps, angles, with_image):
    """device sources, destinations and the three tables of one buffer set"""
    srcs = [(torch.from_numpy(c.image).cuda() if with_image else None, torch.from_numpy(c.depth).cuda()) for c in caps]
    dsts = [(torch.empty_like(i) if with_image else None, torch.empty_like(d)) for i, d in srcs]
    ptrs = torch.tensor([[i.data_ptr() if with_image else 0, o[0].data_ptr() if with_image else 0, d.data_ptr(), o[1].data_ptr()]
                         for (i, d), o in zip(srcs, dsts)], dtype=torch.int64).cuda()
    shapes = torch.tensor([[H, W]] * len(caps), dtype=torch.int32).cuda()
    mats = torch.from_numpy(np.stack([data.rotation_matrix((H, W), a) for a in angles])).cuda()
    return srcs, dsts, ptrs, shapes, mats


def bench_kernel(name, caps, angles, with_image, a):
    n = len(caps)
    nbytes = n * (2 * H * W * 4 + (2 * H * W * 3 if with_image else 0))
    n_sets = int(np.ceil(CACHE / nbytes)) + 1
    sets = [make_set(caps, angles, with_image) for _ in range(n_sets)]
    lib, stream = _lib.load_library(), _lib.current_stream_ptr()

    def call(k):
        _, _, ptrs, shapes, mats = sets[k % n_sets]
        assert lib.cotr_rotate_captures(p(ptrs), p(shapes), p(mats), n, H, W, stream) == 0
    for k in range(max(a.warmup, n_sets)):
        call(k)
    torch.cuda.synchronize()
    ts, k = [], 0
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            call(k)
            k += 1
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / a.iters)
    t0 = time.perf_counter()
    want = [ro.rotate_capture(c if with_image else c._replace(image=None), x) for c, x in zip(caps, angles)]
    host = (time.perf_counter() - t0) * 1e3
    ok = all((not with_image or np.array_equal(o[0].cpu().numpy(), w.image)) and
             np.array_equal(o[1].cpu().numpy().view(np.int32), w.depth.view(np.int32)) for o, w in zip(sets[0][1], want))
    med = statistics.median(ts)
    bound = nbytes / HBM_PEAK * 1e3
    return [f'{name}: one launch {med:.4f} ms ({min(ts):.4f} / {max(ts):.4f}); {nbytes / 1e6:.1f} MB moved (sources once, destinations '
            f'in full) = {nbytes / med / 1e9:.2f} TB/s; bandwidth bound at 8 TB/s {bound:.4f} ms = {100 * bound / med:.0f} % of the '
            f'kernel time; {n_sets} buffer sets rotated (HBM, not cache-resident)',
            f'    identical to the restatement: {ok}; host, numpy restatement (stand-in for cv2, not installed), one run on one core: '
            f'{host:.0f} ms']


def host_timed(fns, iters, warmup=5):
    """fns: {name: fn}; the fns alternate call by call -> {name: (median, min, max) ms}"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(iters):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--num-kp', type=int, default=100)
    ap.add_argument('--max-rotation', type=float, default=30.0)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--batch-iters', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rotate_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_rotate.py measures the GPU: no device found'
    B = a.samples
    pairs = [synth_captures(100 + i, H, W) for i in range(B)]                    # the scenes of tools/bench_dataset.py
    rot = data.draw_rotations(B, a.max_rotation, 1.0, np.random.default_rng(0))  # every capture turned
    caps, angles = [p_[0] for p_ in pairs] + [p_[1] for p_ in pairs], list(rot.T.ravel())
    lines = [f'device: {torch.cuda.get_device_name(0)}; {2 * B} captures of {H} x {W}, angles uniform in +-{a.max_rotation} degrees; kernel: HIP '
             f'events, median (min / max) over {a.rounds} rounds of {a.iters} calls after {a.warmup} warm-up calls; wrapper and batch: host '
             f'clock, each call ends in a device synchronise, median (min - max)']
    lines += bench_kernel(f'cotr_rotate_captures, {2 * B} x image + depth', caps, angles, True, a)
    lines += bench_kernel(f'cotr_rotate_captures, {2 * B} x depth only', caps, angles, False, a)
    up = lambda c: data.Capture(torch.from_numpy(c.image).cuda(), torch.from_numpy(c.depth).cuda(), c.K, c.c2w)   # noqa: E731
    dev = [up(c) for c in caps]
    t = host_timed({'both': lambda: data.rotate_captures(dev, angles),
                    'depth': lambda: data.rotate_captures([c._replace(image=None) for c in dev], angles)}, a.batch_iters)
    lines.append('data.rotate_captures (tables uploaded, destinations allocated, pose on the host), image + depth: '
                 '%.3f ms (%.3f - %.3f); depth only: %.3f ms (%.3f - %.3f)' % (t['both'] + t['depth']))
    zooms = np.logspace(0.0, -1.0, 10)
    rng = np.random.default_rng(0)
    rand = {'seed': rng.random((B, 100)), 'zoom': rng.random(B), 'jitter': rng.random((B, 2)), 'trim': rng.random((B, a.num_kp)),
            'flip': rng.random(B)}
    drand = {k: torch.from_numpy(v).cuda() for k, v in rand.items()}
    qs, ns = dev[:B], dev[B:]
    plain = lambda: data.make_zoom_batch(qs, ns, a.num_kp, zooms, 0.125, rand=drand)                      # noqa: E731
    turned = lambda: data.make_zoom_batch(qs, ns, a.num_kp, zooms, 0.125, rand=drand, rotations=rot)      # noqa: E731
    valid = int(plain()['valid'].sum()), int(turned()['valid'].sum())
    t = host_timed({'plain': plain, 'turned': turned}, a.batch_iters)
    lines.append(f'make_zoom_batch, {B} samples x num_kp {a.num_kp}, bidirectional, rotations=None: %.3f ms (%.3f - %.3f), {valid[0]} valid '
                 f'samples; with all {2 * B} captures turned: %.3f ms (%.3f - %.3f), {valid[1]} valid samples; alternating, '
                 f'{a.batch_iters} calls each' % (t['plain'] + t['turned']))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
