"""Timings of the global pose step (cotr_amd/csrc/global_pose.hip): cotr_average_rotations at n, E = 8, 28 and
32, 496 (every unordered pair once, 0.3 degree noise, a tenth of the edges turned by about 20 degrees per axis; 12 steps), and
cotr_solve_positions at V, N = (2, 2048), (8, 2048), (32, 2048), (32, 8192) (the scene of tests/structure_oracle.py at 0.5 px
noise, the true rotations, every observation visible; 3 rounds, 16 steps of inverse iteration), beside the numpy restatement of
the same rules (tests/global_pose_oracle.py) on the same host.

Device times: HIP events around `--iters` calls after `--warmup` (inputs and outputs on the device, allocated once), median over
`--rounds` rounds (min / max shown).  Host times once each, host clock.  Every device result is compared with the restatement.
GPU box:  python tools/bench_global_pose.py [--out profiles/global_pose_bench.txt]
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
from tests import global_pose_oracle as go
from tests import structure_oracle as so

GRAPHS = ((8, 28), (32, 496))
SHAPES = ((2, 2048), (8, 2048), (32, 2048), (32, 8192))


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


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bench_rotations(n, E, a):
    rng = np.random.default_rng(n + E)
    truth = np.stack([so.rotation(rng.normal(size=3) * 0.3) if v else np.eye(3) for v in range(n)])
    edges = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], np.int32)
    assert len(edges) == E
    planted = rng.uniform(size=E) < 0.1
    planted[edges[:, 1] - edges[:, 0] == 1] = False
    R_rel = np.stack([go.exp_so3(rng.normal(size=3) * 0.3 * go.DEG + (rng.normal(20, 3, 3) * rng.choice([-1.0, 1.0], 3) * go.DEG if planted[e] else 0)) @
                      truth[j] @ truth[i].T for e, (i, j) in enumerate(edges)])
    lib = _lib.load_library()
    d_R, d_e = dev(R_rel), dev(edges)
    R, edge, vi, info, stats = (torch.empty((n, 9), dtype=torch.float64, device='cuda'), torch.empty((E, 4), dtype=torch.float64, device='cuda'),
                                torch.empty((n, 4), dtype=torch.int32, device='cuda'), torch.empty(8, dtype=torch.int32, device='cuda'),
                                torch.empty(2, dtype=torch.float64, device='cuda'))
    stream = _lib.current_stream_ptr()

    def call():
        assert lib.cotr_average_rotations(p(d_R), p(d_e), None, None, n, E, 0, 12, 32 * go.DEG, 1 * go.DEG, 3 * go.DEG, p(R), p(edge), p(vi), p(info),
                                          p(stats), stream) == 0
    t = timed(call, a.warmup, a.iters, a.rounds)
    torch.cuda.synchronize()
    got = R.cpu().numpy().reshape(n, 3, 3)
    line = f'n={n}, E={E}: cotr_average_rotations {t[0]:.4f} ms ({t[1]:.4f} / {t[2]:.4f}), 1 launch, 12 steps'
    if not a.no_host:
        c0 = time.perf_counter()
        want = go.average_rotations(R_rel, edges, n)
        host = (time.perf_counter() - c0) * 1e3
        flags = np.array_equal(edge.cpu().numpy()[:, 2:], want['edge'][:, 2:]) and np.array_equal(info.cpu().numpy(), want['info'])
        line += f'; numpy restatement on the host {host:.0f} ms; largest difference of R {np.abs(got - want["R"]).max():.1e}, flags and info equal: {flags}'
    inl = edge.cpu().numpy()[:, 3] != 0
    line += (f'; {int(planted.sum())} planted edges, flagged exactly: {np.array_equal(~inl, planted)}; worst rotation error '
             f'{go.rotation_error_deg(got, truth):.3f} deg')
    return [line]


def bench_positions(V, n, a):
    sc = so.scene(V, n, seed=V + n)
    Rt = go.true_rotations(sc)
    lib = _lib.load_library()
    count = ctypes.c_size_t()
    assert lib.cotr_solve_positions_work_doubles(V, n, ctypes.byref(count)) == 0
    pts, cams, R = dev(sc['points']), dev(sc['cams']), dev(Rt)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device='cuda')   # noqa: E731
    C, poses, X, stats, work = f64(V, 3), f64(V, 12), f64(n, 3), f64(4), f64(count.value)
    used, info = torch.empty((V, n), dtype=torch.uint8, device='cuda'), torch.empty(8, dtype=torch.int32, device='cuda')
    stream = _lib.current_stream_ptr()

    def call():
        assert lib.cotr_solve_positions(p(pts), None, p(cams), p(R), None, V, n, None, 0, 4.0, 3, 8, 16, p(C), p(poses), p(X), p(used), p(stats), p(info),
                                        p(work), stream) == 0
    t = timed(call, a.warmup, a.iters, a.rounds)
    torch.cuda.synchronize()
    gC, gs, gi = C.cpu().numpy(), stats.cpu().numpy(), info.cpu().numpy()
    line = f'V={V}, N={n}: cotr_solve_positions {t[0]:.4f} ms ({t[1]:.4f} / {t[2]:.4f}), 19 launches, work {count.value * 8 / 2**20:.2f} MiB'
    if not a.no_host:
        c0 = time.perf_counter()
        want = go.solve_positions(sc['points'], sc['cams'], Rt)
        host = (time.perf_counter() - c0) * 1e3
        same = np.array_equal(used.cpu().numpy(), want['used']) and np.array_equal(gi, want['info'])
        line += f'; numpy restatement on the host {host:.0f} ms; largest difference of C {np.abs(gC - want["C"]).max():.1e}, used and info equal: {same}'
    err, s = go.centre_error(gC, sc['poses'])
    line += f'; {gi[1]} observations, {gi[2]} views placed, lambda0 {gs[0]:.3e}, lambda1 {gs[1]:.3e}; centre error {err / abs(s):.4f} of a baseline of 0.6'
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy restatement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'global_pose_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_global_pose.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls; host times once, host clock']
    for n, E in GRAPHS:
        lines += bench_rotations(n, E, a)
    for V, n in SHAPES:
        lines += bench_positions(V, n, a)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
