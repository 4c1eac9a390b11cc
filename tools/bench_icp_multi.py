"""Joint point-to-plane ICP timings: cotr_icp_multiview (cotr_amd/csrc/icp_multi.hip) with 10 iterations over every ordered pair
of 4 and of 8 views of the three-plane corner of tests/icp_multi_oracle.py, at 96 x 128 and 480 x 640 (max_dist 0.25, stride 1),
and cotr_icp_maps on the same depth maps.  The device time per iteration is the difference between the calls with 10 iterations
and with none, over 10.  Beside it, the same evaluations done as a chain of cotr_icp_depth calls, one per ordered pair from the
same start (each takes its own maps again and solves its own 6 x 6 system): again 10 iterations against none, over 10.

Device times: HIP events around `--iters` calls after `--warmup` (inputs and outputs on the device, allocated once), median over
`--rounds` rounds (min / max shown).  The device result at 96 x 128 is checked against the numpy restatement.
GPU box:  python tools/bench_icp_multi.py [--out profiles/icp_multi_bench.txt]
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
from tests import icp_multi_oracle as mo


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


def bench(n, H, W, a, steps=10):
    sc = mo.scene(H, W, 0.05, n)
    edges_h = mo.all_pairs(n)
    E = len(edges_h)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    depths, start, edges = cu(sc['depths']), cu(np.stack(sc['start'])), cu(edges_h)
    K = (ctypes.c_double * (9 * n))(*sc['Ks'].reshape(-1))
    C = (ctypes.c_double * 3)(*sc['centre'])
    lib = _lib.load_library()
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device='cuda')   # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device='cuda')     # noqa: E731
    maps, minfo, c2w, info, vinfo, stats, sums = f64(n, H, W, 6), i32(n, 4), f64(n, 4, 4), i32(8), i32(n, 4), f64(2), f64(E, 8, 32)
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    stream = _lib.current_stream_ptr()

    def take_maps():
        assert lib.cotr_icp_maps(p(depths), n, H, W, K, 0.05, p(maps), p(minfo), stream) == 0

    def joint(iters):
        assert lib.cotr_icp_multiview(p(maps), n, H, W, K, p(start), p(edges), E, 1, C, None, mo.MAX_DIST, 0.5, 1e-9, iters, 1, p(c2w), p(info),
                                      p(vinfo), p(stats), p(sums), None, None, stream) == 0
    # the same evaluations as one cotr_icp_depth call per ordered pair
    nb = ctypes.c_size_t()
    assert lib.cotr_icp_depth_scratch_bytes(H, W, H, W, 1, ctypes.byref(nb)) == 0
    scratch = torch.empty(nb.value, dtype=torch.uint8, device='cuda')
    rel = [mo.relative(sc['start'][x], sc['start'][y]) for x, y in edges_h]
    R0s, t0s = cu(np.stack([r.reshape(9) for r, _ in rel])), cu(np.stack([t for _, t in rel]))
    Rd, td, st2, info2 = f64(9), f64(3), f64(2), i32(8)
    Ks = [(ctypes.c_double * 9)(*sc['Ks'][v].reshape(-1)) for v in range(n)]

    dp, Rp, tp = [p(depths[v]) for v in range(n)], [p(R0s[e]) for e in range(E)], [p(t0s[e]) for e in range(E)]

    def chain(iters):
        for e, (x, y) in enumerate(edges_h):
            assert lib.cotr_icp_depth(dp[x], H, W, Ks[x], dp[y], H, W, Ks[y], Rp[e], tp[e], None, None, None, mo.MAX_DIST, 0.5, 0.05,
                                      1e-6, iters, 1, p(Rd), p(td), p(info2), p(st2), None, None, None, None, p(scratch), nb.value, stream) == 0
    take_maps()
    tm = timed(take_maps, a.warmup, a.iters, a.rounds)
    t10, t0_ = timed(lambda: joint(steps), a.warmup, a.iters, a.rounds), timed(lambda: joint(0), a.warmup, a.iters, a.rounds)
    c10, c0_ = timed(lambda: chain(steps), a.warmup, a.iters, a.rounds), timed(lambda: chain(0), a.warmup, a.iters, a.rounds)
    joint(steps)
    torch.cuda.synchronize()
    i, rmse = info.cpu().numpy(), float(stats.cpu().numpy()[1])
    per, per_chain = (t10[0] - t0_[0]) / steps, (c10[0] - c0_[0]) / steps
    out = [f'{n} views at {H} x {W}, all {E} ordered pairs ({8 * E} workgroups an evaluation), {steps} iterations ({1 + 2 * (steps + 1)} launches): '
           f'cotr_icp_multiview {t10[0]:.4f} ms ({t10[1]:.4f} / {t10[2]:.4f}), with none (3 launches: one evaluation) {t0_[0]:.4f} ms '
           f'({t0_[1]:.4f} / {t0_[2]:.4f}); {i[1]} steps, {i[2]} pairs, {i[5]} of {i[4]} edges kept, {i[6]} free views, stop reason {i[3]}, rmse {rmse:.3e}',
           f'    an iteration: {per * 1e3:.1f} us = {per * 1e3 / E:.2f} us an edge; cotr_icp_maps of the {n} maps (2 launches): {tm[0]:.4f} ms '
           f'({tm[1]:.4f} / {tm[2]:.4f})',
           f'    the same as {E} chained cotr_icp_depth calls: {steps} iterations {c10[0]:.4f} ms ({c10[1]:.4f} / {c10[2]:.4f}), none '
           f'{c0_[0]:.4f} ms ({c0_[1]:.4f} / {c0_[2]:.4f}); an iteration of all pairs: {per_chain * 1e3:.1f} us = {per_chain / per:.2f} x the joint call']
    if H * W <= 96 * 128:
        o = mo.multiview(sc['maps'], sc['Ks'], sc['start'], edges_h, centre=sc['centre'], iters=steps)
        out.append(f'    info identical to the restatement: {list(i) == list(o["info"])}; poses against the restatement: '
                   f'{mo.pose_distance(list(c2w.cpu().numpy()), list(o["c2w"])):.1e}')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'icp_multi_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_icp_multi.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls']
    for H, W in ((96, 128), (480, 640)):
        for n in (4, 8):
            lines += bench(n, H, W, a)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
