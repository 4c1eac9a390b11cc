"""Timings of cotr_detect_keypoints (cotr_amd/csrc/keypoints.hip) at H x W x n = 480 x 640 x 1, 480 x 640 x 8 and
1080 x 1920 x 1, on three inputs each: a textured scene (noise over rectangles) and uniform noise at the defaults (min_eig, window
radius 2, NMS radius 4, quality 0.01, K = 2048), and uniform noise at NMS radius 1, the worst case of the ranking stage: about one
pixel in nine is a candidate and nearly all survive.  Beside each the same call with min_score = inf, which leaves no candidate:
the fill, and the tile stage up to the keys, so that the difference is what the window scans, the candidate list and the ranking cost.  The floor is one read
of the images at the HBM rate of the data sheet (8 TB/s).

Device times: HIP events around `--iters` calls after `--warmup` (inputs and outputs on the device, allocated once), median over
`--rounds` rounds (min / max shown).  At 480 x 640 x 1 every output is compared with the restatement (tests/keypoints_oracle.py).
GPU box:  python tools/bench_keypoints.py [--out profiles/keypoints_bench.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cotr_amd import _lib
from tests import keypoints_oracle as ko

SHAPES = ((480, 640, 1), (480, 640, 8), (1080, 1920, 1))
HBM_BYTES_PER_S = 8e12
K = 2048


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


def p(x):
    return ctypes.c_void_p(x.data_ptr())


def bench(H, W, n, what, images, R, a):
    lib = _lib.load_library()
    count = ctypes.c_size_t()
    assert lib.cotr_detect_keypoints_work_bytes(n, H, W, R, ctypes.byref(count)) == 0
    d = torch.from_numpy(images).cuda()
    xy, score = torch.empty((n, K, 2), dtype=torch.float64, device='cuda'), torch.empty((n, K), dtype=torch.float64, device='cuda')
    pixel, info = torch.empty((n, K), dtype=torch.int32, device='cuda'), torch.empty((n, 4), dtype=torch.int32, device='cuda')
    work = torch.empty(count.value, dtype=torch.uint8, device='cuda')
    stream = _lib.current_stream_ptr()

    def call(min_score=0.0):
        assert lib.cotr_detect_keypoints(p(d), None, n, H, W, 0, 2, R, 0, 0.01, min_score, K, p(xy), p(score), p(pixel), p(info), p(work), stream) == 0
    tiles = timed(lambda: call(float('inf')), a.warmup, a.iters, a.rounds)
    t = timed(call, a.warmup, a.iters, a.rounds)
    torch.cuda.synchronize()
    gi = info.cpu().numpy()
    floor_ms = n * H * W / HBM_BYTES_PER_S * 1e3
    line = (f'{H} x {W} x {n}, {what}, R={R}: cotr_detect_keypoints {t[0]:.4f} ms ({t[1]:.4f} / {t[2]:.4f}), with min_score = inf (no window scans, no list, no ranking) '
            f'{tiles[0]:.4f} ms ({tiles[1]:.4f} / {tiles[2]:.4f}); 3 launches, work {count.value / 2**20:.2f} MiB; one read of the images at 8 TB/s '
            f'{floor_ms * 1e3:.2f} us: the call is {t[0] / floor_ms:.0f} x, the call with min_score = inf {tiles[0] / floor_ms:.0f} x that; candidates / survivors / written '
            f'of image 0: {gi[0, :3].tolist()}')
    if (H, W, n) == SHAPES[0] and not a.no_host:
        want = ko.detect(images, None, 'min_eig', 2, R, 0, 0.01, 0.0, K)
        got = dict(keypoints=xy, scores=score, pixel=pixel, info=info)
        line += f'; every output equal to the restatement: {all(np.array_equal(got[k].cpu().numpy(), want[k], equal_nan=True) for k in got)}'
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-host', action='store_true', help='skip the restatement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'keypoints_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_keypoints.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls; min_eig, window radius 2, quality 0.01, K = {K}']
    for H, W, n in SHAPES:
        for what, images, R in (('textured scene', ko.textured(n, H, W, seed=H + n), 4), ('uniform noise', ko.noise(n, H, W, seed=H + n), 4),
                                ('uniform noise', ko.noise(n, H, W, seed=H + n), 1)):
            lines.append(bench(H, W, n, what, images, R, a))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
