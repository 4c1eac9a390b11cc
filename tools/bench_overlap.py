"""Times the pair selection of cotr_amd/scene.py on the GPU against the numpy oracle on the CPU:
overlap_matrix for 32 captures of 480 x 640 with all 1024 cells, world_points alone, knn_pool + draw_pairs on the result,
and tests/scene_oracle.py for the same cells on one core.  Host clock around work that ends in a device synchronise; the
captures are uploaded once, outside the timed window (a loader would keep them on the device).  Beside the times: the
points re-projected per second and the bytes each launch must move at least.

    python tools/bench_overlap.py [--captures 32] [--iters 20] [--oracle-cells N] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cotr_amd import data, scene  # noqa: E402
from cotr_amd.utils.synth import synth_scene  # noqa: E402
from tests import scene_oracle as oracle  # noqa: E402


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
    ap.add_argument('--captures', type=int, default=32)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--oracle-cells', type=int, default=None, help='time the oracle on the first N cells only (default: all)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    n, px = a.captures, a.height * a.width
    caps = synth_scene(100, n, a.height, a.width)
    dcaps = [data.Capture(None, torch.from_numpy(c.depth).cuda(), c.K, c.c2w) for c in caps]
    pairs = np.argwhere(np.ones((n, n), dtype=bool))
    lines = [f'device: {torch.cuda.get_device_name(0)}; {n} captures of {a.height} x {a.width}, {len(pairs)} cells, {a.iters} timed calls each']
    ratio, counts = scene.overlap_pairs(dcaps, pairs)
    dist = ratio.view(n, n)
    valid = np.array([int((c.depth > 0).sum()) for c in caps])
    points = int(valid[pairs[:, 1]].sum())                      # world points projected, over all cells
    med, lo, hi = timed(lambda: scene.overlap_matrix(dcaps), a.iters)
    lines.append(f'overlap_matrix: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); {points} points re-projected, '
                 f'{points / med / 1e6:.2f} G points/s, {len(pairs) / med * 1e3:.0f} cells/s')
    wmed, wlo, whi = timed(lambda: scene.world_points(dcaps), a.iters)
    lines.append(f'world_points alone, {n} captures: median {wmed:.3f} ms (min {wlo:.3f}, max {whi:.3f})')
    in_flight = min(len(pairs), max(1, scene.SCRATCH_BYTES // (4 * px)))
    tiles = -(-len(pairs) // in_flight)
    lines.append(f'canvas scratch: {in_flight} pairs in flight x {4 * px} B = {in_flight * 4 * px / 2 ** 20:.0f} MiB, {tiles} tiles; '
                 f'launches per call: 1 world_points + {tiles} x (memset, splat, score) + 1 ratio')
    got = counts.cpu().numpy().astype(np.int64)
    # bytes each launch must move at least, summed over the call (float32 depth and xyz, uint32 canvas)
    b_world = n * px * (4 + 12)
    b_memset = len(pairs) * px * 4
    b_splat = len(pairs) * px * 12                              # every source slot is read; + one 4-byte atomic per kept point
    b_score = len(pairs) * px * (4 + 4)                         # canvas + query depth; + 12 bytes per pixel with a winner and depth
    lines.append(f'least bytes per call: world_points {b_world / 1e6:.0f} MB, canvas memsets {b_memset / 1e6:.0f} MB, splat {b_splat / 1e6:.0f} MB '
                 f'read + 4 B atomic per kept point, score {b_score / 1e6:.0f} MB + 12 B per scored pixel (at least {12 * int(got[:, 0].sum()) / 1e6:.0f} MB); '
                 f'sum {(b_world + b_memset + b_splat + b_score) / 1e6:.0f} MB = {(b_world + b_memset + b_splat + b_score) / med / 1e6:.1f} GB/s at the median')
    kmed, klo, khi = timed(lambda: scene.draw_pairs(*scene.knn_pool(dist, 8), np.full(n, 0.5)), a.iters)
    lines.append(f'knn_pool(k=8) + draw_pairs on the {n} x {n} matrix: median {kmed:.3f} ms (min {klo:.3f}, max {khi:.3f})')
    cells = pairs if a.oracle_cells is None else pairs[:a.oracle_cells]
    t0 = time.perf_counter()
    want_ratio, want_counts, _ = oracle.overlap_pairs(caps, cells)
    dt = time.perf_counter() - t0
    lines.append(f'numpy oracle, {len(cells)} of the same cells, one CPU core: {dt * 1e3:.0f} ms ({dt / len(cells) * 1e3:.1f} ms per cell'
                 + (f', {dt / len(cells) * len(pairs):.1f} s for all {len(pairs)}' if len(cells) != len(pairs) else '') + ')')
    lines.append(f'cells whose integer counts differ from the oracle: {int((got[:len(cells)] != want_counts).any(1).sum())} of {len(cells)}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
