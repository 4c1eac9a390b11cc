"""Photometric depth refinement timings (cotr_amd/csrc/photodepth.hip) at 480 x 640 on the arc of ``synth_scene``:
cotr_photo_depth with K = 1, 2, 4, 8 neighbour images at radius 2, 4 steps and 3 sweeps, and one line each for radius 4 and for 16
steps (K = 4), from the true depth times a smooth perturbation of 1 %.  Beside the time: megapixels per second and taps per second,
a tap being one projection and bilinear sample - counted as pixels that take a step x sweeps x (2 steps + 1) x K x (2 radius + 1)^2,
which is what the rule asks for at most (a neighbour that loses a tap outside its image ends that patch early).  The numpy
restatement tests/photodepth_oracle.py runs the same configuration at 96 x 128 on one core of the host, and the device is held
against it there on every pixel it does not call ambiguous.

Device times: HIP events around `--iters` calls of the C ABI after `--warmup` (inputs and outputs on the device, allocated once),
median over `--rounds` rounds (min / max shown).  Every configuration runs in a process of its own under a time limit; the first
that fails ends the run.
GPU box:  python tools/bench_photodepth.py [--out profiles/photodepth_bench.txt]
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 480, 640
SMALL = (96, 128)
# K, radius, steps
CONFIGS = [(1, 2, 4), (2, 2, 4), (4, 2, 4), (8, 2, 4), (4, 4, 4), (4, 2, 16)]
SWEEPS = 3
LIMIT = 300   # seconds a configuration may take, the restatement included


def timed(fn, warmup, iters, rounds):
    import torch
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


def device_call(sc, depth, R, S):
    """-> (call: one enqueue of cotr_photo_depth, the four device tensors it writes)"""
    import numpy as np
    import torch
    from cotr_amd import _lib
    lib = _lib.load_library()
    V, h, w = sc['grey'].shape
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (sc['grey'], depth, sc['cams'], sc['poses'])]
    out = (torch.empty((h, w), dtype=torch.float32, device='cuda'), torch.empty((h, w), dtype=torch.float32, device='cuda'),
           torch.empty((h, w), dtype=torch.uint8, device='cuda'), torch.empty(8, dtype=torch.int32, device='cuda'))
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    stream = _lib.current_stream_ptr()

    def call():
        assert lib.cotr_photo_depth(p(t[0]), p(t[1]), p(t[2]), p(t[3]), V, h, w, None, R, S, SWEEPS, 0.004 if S < 16 else 0.001, 4.0, 0.5, 1, 50.0, 1,
                                    p(out[0]), p(out[1]), p(out[2]), p(out[3]), stream) == 0, lib.cotr_raster_last_error()
    return call, out


def bench(K, R, S, a):
    import numpy as np
    import torch
    from tests import photodepth_oracle as po
    sc = po.scene(H, W, K)
    call, out = device_call(sc, po.perturbed(sc['depth'], 0.01), R, S)
    ms = timed(call, a.warmup, a.iters, a.rounds)
    info = out[3].cpu().numpy()
    stepping = int(info[1] + info[5] + info[6] + info[7])
    taps = stepping * SWEEPS * (2 * S + 1) * K * (2 * R + 1) ** 2
    # the restatement, and the device against it, at a size it finishes in seconds
    small = po.scene(*SMALL, K)
    start = po.perturbed(small['depth'], 0.01)
    t0 = time.perf_counter()
    o = po.photo_depth(small['grey'], start, small['cams'], small['poses'], radius=R, steps=S, sweeps=SWEEPS, rel_step=0.004 if S < 16 else 0.001)
    host = time.perf_counter() - t0
    call_s, out_s = device_call(small, start, R, S)
    small_ms = timed(call_s, 2, 5, 3)[0]
    sure = ~o['amb']
    same = all(np.array_equal(x.cpu().numpy()[sure], o[k][sure], equal_nan=True) for x, k in zip(out_s[:3], ('depth', 'score', 'views')))
    return (f'cotr_photo_depth K = {K} R = {R} S = {S:2d}: {ms[0]:8.3f} ms ({ms[1]:.3f} / {ms[2]:.3f}) = {H * W / ms[0] / 1e3:7.1f} Mpx/s, at most '
            f'{taps / 1e9:.3f} G taps = {taps / ms[0] / 1e9:.2f} T taps/s; info {info.tolist()}; at {SMALL[0]} x {SMALL[1]}: {small_ms * 1e3:.0f} us against '
            f'{host:.2f} s of the numpy restatement on one core ({host / small_ms * 1e3:.0f} x), {o["ambiguous"]} ambiguous pixels, identical on the others: {same}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--config', type=int, default=None, help='run this entry of CONFIGS alone and print its line')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'photodepth_bench.txt'))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_photodepth.py measures the GPU: no device found'
    if a.config is not None:
        print(bench(*CONFIGS[a.config], a))
        return
    lines = [f'device: {torch.cuda.get_device_name(0)}; {H} x {W}, {SWEEPS} sweeps; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} '
             f'calls after {a.warmup} warm-up calls']
    for i in range(len(CONFIGS)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--config', str(i), '--warmup', str(a.warmup), '--iters', str(a.iters), '--rounds',
                            str(a.rounds)], stdout=subprocess.PIPE, text=True, timeout=LIMIT)
        if r.returncode != 0:
            sys.exit(f'configuration {CONFIGS[i]} ended with status {r.returncode}: nothing more is started')
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
