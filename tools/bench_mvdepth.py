"""Multi-view depth map timings (cotr_amd/csrc/mvdepth.hip) at 480 x 640 on the arc of ``synth_scene``:
cotr_corr_depth with K = 1, 2, 4, 8 neighbour maps (the exact maps of the true depth with noise of 0.4 px and a sixth of the
entries thrown 8 to 20 px off, a validity mask, 10 refit steps) and cotr_depth_consistency on n = 2, 8, 32 depth maps, in
megapixels per second, beside the bytes each call must move at least (depth call: 8 K of correspondences, K of validity and 9 of
outputs per pixel; filter: 4 in and 5 out per pixel of every view, and 4 per gather, at most n - 1 per valid pixel) and the numpy
restatement tests/mvdepth_oracle.py on one core of the host (for n = 32 timed on the pairs of view 0 alone and scaled by 32).

Device times: HIP events around `--iters` calls after `--warmup` (inputs and outputs on the device, allocated once), median over
`--rounds` rounds (min / max shown).  Every device result is checked against the restatement, bit for bit.
GPU box:  python tools/bench_mvdepth.py [--out profiles/mvdepth_bench.txt]
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
from tests import mvdepth_oracle as mo

H, W = 480, 640
MAX_COS = float(np.cos(np.deg2rad(1.5)))


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


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def p(x):
    return ctypes.c_void_p(x.data_ptr() if x is not None else None)


def bench_depth(K, a):
    sc = mo.scene(H, W, K)
    rng = np.random.default_rng(K)
    corr = sc['corr'].astype(np.float64) + rng.normal(0.0, 0.4, sc['corr'].shape)
    off = rng.random(corr.shape[:3]) < 1 / 6
    ang, r = rng.uniform(0, 2 * np.pi, off.shape), rng.uniform(8.0, 20.0, off.shape)
    corr[..., 0] += np.where(off, r * np.cos(ang), 0.0)
    corr[..., 1] += np.where(off, r * np.sin(ang), 0.0)
    corr = corr.astype(np.float32)
    valid = sc['vis'].astype(np.uint8)
    lib = _lib.load_library()
    t = [cu(corr), cu(valid), cu(sc['cams']), cu(sc['poses'])]
    depth, views, err, info = (torch.empty((H, W), dtype=torch.float32, device='cuda'), torch.empty((H, W), dtype=torch.uint8, device='cuda'),
                               torch.empty((H, W), dtype=torch.float32, device='cuda'), torch.empty(8, dtype=torch.int32, device='cuda'))
    stream = _lib.current_stream_ptr()

    def call():
        assert lib.cotr_corr_depth(p(t[0]), p(t[1]), p(t[2]), p(t[3]), K + 1, H, W, None, 2.0, MAX_COS, 50.0, 1, 10, p(depth), p(views), p(err), p(info),
                                   stream) == 0
    ms = timed(call, a.warmup, a.iters, a.rounds)
    t0 = time.perf_counter()
    o = mo.corr_depth(corr, valid, sc['cams'], sc['poses'], threshold=2.0, max_cos=MAX_COS)
    host = time.perf_counter() - t0
    same = all(np.array_equal(x.cpu().numpy(), o[k], equal_nan=True) for x, k in ((depth, 'depth'), (views, 'views'), (err, 'err'), (info, 'info')))
    nbytes = H * W * (8 * K + K + 9)
    return (f'cotr_corr_depth   K = {K}: {ms[0] * 1e3:8.1f} us ({ms[1] * 1e3:.1f} / {ms[2] * 1e3:.1f}) = {H * W / ms[0] / 1e3:8.1f} Mpx/s; at least '
            f'{nbytes / 1e6:.2f} MB = {nbytes / ms[0] / 1e6:.1f} GB/s; info {o["info"].tolist()}; numpy restatement {host * 1e3:.0f} ms '
            f'({host / ms[0] * 1e3:.0f} x); identical to it: {same}')


def bench_filter(n, a):
    from cotr_amd.utils.synth import synth_scene
    caps = synth_scene(0, n + 2, H, W)[:n]
    depths, Ks, c2ws = np.stack([c.depth for c in caps]), np.stack([c.K for c in caps]), np.stack([c.c2w for c in caps])
    lib = _lib.load_library()
    d, m = cu(depths), cu(c2ws)
    K = (ctypes.c_double * (9 * n))(*Ks.reshape(-1))
    out, count, info = (torch.empty((n, H, W), dtype=torch.float32, device='cuda'), torch.empty((n, H, W), dtype=torch.uint8, device='cuda'),
                        torch.empty((n, 4), dtype=torch.int32, device='cuda'))
    stream = _lib.current_stream_ptr()

    def call(pairs=None):
        assert lib.cotr_depth_consistency(p(d), n, H, W, K, p(m), None, p(pairs), 1.0, 0.01, 1, -1, p(out), p(count), p(info), stream) == 0
    ms = timed(call, a.warmup, a.iters, a.rounds)
    pairs, scale = None, 1
    if n > 8:   # the restatement on the pairs of view 0 alone, scaled
        pairs, scale = np.zeros((n, n), np.uint8), n
        pairs[0] = 1
    t0 = time.perf_counter()
    o = mo.depth_consistency(depths, Ks, c2ws, pairs=pairs, min_views=1)
    host = (time.perf_counter() - t0) * scale
    call(None if pairs is None else cu(pairs))
    torch.cuda.synchronize()
    same = all(np.array_equal(x.cpu().numpy(), o[k]) for x, k in ((out, 'depth'), (count, 'count'), (info, 'info')))
    valid = int((depths > 0).sum())
    nbytes = n * H * W * 9 + 4 * (n - 1) * valid
    return (f'cotr_depth_consistency n = {n:2d}: {ms[0] * 1e3:8.1f} us ({ms[1] * 1e3:.1f} / {ms[2] * 1e3:.1f}) = {n * H * W / ms[0] / 1e3:8.1f} Mpx/s; '
            f'{n * H * W * 9 / 1e6:.2f} MB streamed and at most {4 * (n - 1) * valid / 1e6:.2f} MB gathered = {nbytes / ms[0] / 1e6:.1f} GB/s; numpy restatement '
            f'{host * 1e3:.0f} ms{" (view 0 times " + str(n) + ")" if scale > 1 else ""} ({host / ms[0] * 1e3:.0f} x); identical to it: {same}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mvdepth_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mvdepth.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; {H} x {W}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls']
    lines += [bench_depth(K, a) for K in (1, 2, 4, 8)]
    lines += [bench_filter(n, a) for n in (2, 8, 32)]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
