"""Dense point-to-plane ICP timings: cotr_icp_depth (cotr_amd/csrc/icp.hip) with 10 iterations on the three-plane corner of
tests/icp_oracle.py at 96 x 128 and 480 x 640 (both captures at that size, max_dist 0.25, stride 1), and the numpy restatement
of the same rules (tests/icp_oracle.py) on the same host.  Alongside, the least bytes an iteration must move: the source depth
(4 B a source pixel) plus 96 B a pair, the vertex and the normal gathered on both sides; the device time per iteration is the
difference between the calls with 10 iterations and with none, over 10.

Device times: HIP events around `--iters` calls after `--warmup` (inputs on the device, scratch allocated once), median over
`--rounds` rounds (min / max shown).  Host times once each, host clock.  The device result is checked against the restatement.
GPU box:  python tools/bench_icp.py [--out profiles/icp_bench.txt]
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
from cotr_amd.inference._args import camera
from cotr_amd.inference.icp import icp_depth
from tests import icp_oracle as io


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


def bench(H, W, a, steps=10, max_dist=0.25):
    sc = io.scene(H, W, H, W)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    da, db, R0, t0 = cu(sc['depth_a']), cu(sc['depth_b']), cu(sc['R0'].reshape(9)), cu(sc['t0'])
    ka, kb = camera(sc['K_a'], 'K_a'), camera(sc['K_b'], 'K_b')
    lib = _lib.load_library()
    nb = ctypes.c_size_t()
    assert lib.cotr_icp_depth_scratch_bytes(H, W, H, W, 1, ctypes.byref(nb)) == 0
    s1 = torch.empty(nb.value, dtype=torch.uint8, device='cuda')
    Rd, td, st = (torch.empty(k, dtype=torch.float64, device='cuda') for k in (9, 3, 2))
    info = torch.empty(8, dtype=torch.int32, device='cuda')
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    stream = _lib.current_stream_ptr()

    def call(iters):
        assert lib.cotr_icp_depth(p(da), H, W, ka, p(db), H, W, kb, p(R0), p(t0), None, None, None, max_dist, 0.5, 0.05, 1e-6, iters, 1, p(Rd), p(td),
                                  p(info), p(st), None, None, None, None, p(s1), nb.value, stream) == 0
    t10 = timed(lambda: call(steps), a.warmup, a.iters, a.rounds)
    t0_ = timed(lambda: call(0), a.warmup, a.iters, a.rounds)
    r = {k: v.cpu().numpy() for k, v in icp_depth(da, sc['K_a'], db, sc['K_b'], R0, t0, max_dist, iters=steps).items()}
    c0 = time.perf_counter()
    o = io.icp(sc['maps_a'], sc['K_a'], sc['maps_b'], sc['R0'], sc['t0'], iters=steps, max_dist=max_dist)
    host = (time.perf_counter() - c0) * 1e3
    c0 = time.perf_counter()
    io.maps(sc['depth_a'], sc['K_a']), io.maps(sc['depth_b'], sc['K_b'])
    host_maps = (time.perf_counter() - c0) * 1e3
    i = r['info']
    per_iter = (t10[0] - t0_[0]) / steps
    least = 4 * H * W + 96 * int(i[2])
    d, w = io.errors(r['R'], r['t'], sc), io.errors(o['R'], o['t'], sc)
    return [f'{H} x {W}, {steps} iterations ({3 + 2 * (steps + 1)} launches): cotr_icp_depth {t10[0]:.4f} ms ({t10[1]:.4f} / {t10[2]:.4f}), with '
            f'none (5 launches: the maps and one evaluation) {t0_[0]:.4f} ms ({t0_[1]:.4f} / {t0_[2]:.4f}); {i[1]} steps, {i[2]} pairs of {i[4]} '
            f'source pixels, stop reason {i[3]}, rmse {r["stats"][1]:.3e}',
            f'    an iteration: {per_iter * 1e3:.1f} us; the least it must move: {least} B (4 B x {H * W} source pixels + 96 B x {i[2]} pairs) = '
            f'{least / (per_iter * 1e-3) / 1e9:.1f} GB/s at that time',
            f'    info identical to the restatement: {list(i) == list(o["info"])}; pose against the restatement: '
            f'{io.pose_distance(r["R"], r["t"], o["R"], o["t"]):.1e}; against the scene: rotation {d[0]:.2e}, translation {d[1]:.2e} '
            f'(restatement {w[0]:.2e} / {w[1]:.2e})',
            f'    host, numpy restatement: {steps} iterations {host:.0f} ms, the two maps {host_maps:.0f} ms']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'icp_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_icp.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls; host times once, host clock']
    for H, W in ((96, 128), (480, 640)):
        lines += bench(H, W, a)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
