"""Warp timings: cotr_warp_map / cotr_warp_perspective at the demos' shapes against the route the package offered before
them (torch.nn.functional.grid_sample on a float NCHW copy), and the numpy restatement on the host.

  single_pair   demo_single_pair.py:43: a 768 x 1024 x 3 image warped by a 768 x 1024 float64 map, a real
                triangulate_corr(as_tensor=True) output
  homography    demo_homography.py:46-49: a 1200 x 1000 x 3 picture pasted into a 4000 x 3000 x 3 photograph through four
                corners (one cotr_warp_perspective launch with the photograph as background)
  smooth 12 MP  a 3000 x 4000 x 3 image warped by a smooth random 3000 x 4000 float32 map

Device times: HIP events around `--iters` calls after `--warmup`, median over `--rounds` rounds (min / max shown); the new
call and the grid_sample route alternate round by round in one process, and the ratio is taken round by round.  Every call of a
round works on the next of N sets of buffers (inputs and outputs), N chosen so that the sets together exceed 320 MiB: the
256 MiB Infinity Cache cannot serve a repeat, the figures are HBM figures.  Bytes moved are computed from the shapes: map,
destination and background in full, the source once; the bound is that figure over the 8 TB/s HBM peak (about 6.3 TB/s is
achievable).  The grid_sample route: uint8 -> float, permute to NCHW, the grid normalised to [-1, 1] (for the paste: the grid
from the matrix, a second sample for the mask, the composite), grid_sample(bilinear, zeros, align_corners=True), round, clamp,
uint8, permute back, all on the device.  Every device result of the new calls is checked against the restatement
(tests/warp_oracle.py); the restatement's own host time is taken once, as a stand-in for cv2, which is not installed.
GPU box:  python tools/bench_warp.py [--out profiles/warp_bench.txt]
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
import torch.nn.functional as F

from cotr_amd import _lib
from cotr_amd.inference import get_perspective_transform, triangulate_corr, warp_by_map, warp_perspective
from cotr_amd.inference.warp import invert_perspective, picture_corners
from tests import raster_oracle as ro
from tests import warp_oracle as wo

HBM_PEAK = 8.0e12
CACHE = 320 << 20          # rotate over more bytes than the 256 MiB Infinity Cache holds


def timed_pair(fns, n_sets, warmup, iters, rounds):
    """fns: {name: fn(set index)}; the fns alternate round by round -> {name: [ms per call, one per round]}"""
    for fn in fns.values():
        for k in range(max(warmup, n_sets)):
            fn(k % n_sets)
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    k = 0
    for _ in range(rounds):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn(k % n_sets)
                k += 1
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b) / iters)
    return ts


def grid_route_map(img, m):
    """warp_by_map's job through grid_sample: img uint8 [H, W, C], m [Hd, Wd, 2] float32 / float64 pixel indices"""
    Hs, Ws = img.shape[:2]
    src = img.permute(2, 0, 1)[None].float()
    g = m.float()
    grid = torch.stack([g[..., 0] * (2.0 / max(Ws - 1, 1)) - 1, g[..., 1] * (2.0 / max(Hs - 1, 1)) - 1], -1)[None]
    out = F.grid_sample(src, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    return out[0].round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def grid_route_paste(picture, Minv, bg):
    """paste_by_corners' job through grid_sample: the grid from the matrix, picture and mask sampled, the composite"""
    Hd, Wd = bg.shape[:2]
    Hs, Ws = picture.shape[:2]
    x = torch.arange(Wd, device=bg.device, dtype=torch.float64)[None, :]
    y = torch.arange(Hd, device=bg.device, dtype=torch.float64)[:, None]
    W = Minv[2, 0] * x + Minv[2, 1] * y + Minv[2, 2]
    gx = ((Minv[0, 0] * x + Minv[0, 1] * y + Minv[0, 2]) / W).float() * (2.0 / (Ws - 1)) - 1
    gy = ((Minv[1, 0] * x + Minv[1, 1] * y + Minv[1, 2]) / W).float() * (2.0 / (Hs - 1)) - 1
    grid = torch.stack([gx, gy], -1)[None]
    src = torch.cat([picture.permute(2, 0, 1).float(), torch.ones((1, Hs, Ws), device=bg.device)])[None]
    out = F.grid_sample(src, grid, mode='bilinear', padding_mode='zeros', align_corners=True)[0]
    warped = out[:3].round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0)
    vmask = (out[3] > 0)[..., None]
    return torch.where(vmask, warped, bg)


def report(name, ts, nbytes, n_sets, ok, route_diff, host_ms):
    new, old = ts['new'], ts['grid_sample']
    ratio = [o / n for o, n in zip(old, new)]
    med = statistics.median(new)
    bound = nbytes / HBM_PEAK * 1e3
    verdict = 'not slower' if min(ratio) >= 1.0 else 'SLOWER in at least one round' if statistics.median(ratio) >= 1.0 else 'SLOWER'
    return [f'{name}: new call {med:.4f} ms ({min(new):.4f} / {max(new):.4f}); {nbytes / 1e6:.1f} MB moved (map, destination and '
            f'background in full, source once) = {nbytes / med / 1e9:.2f} TB/s; bandwidth bound at 8 TB/s {bound:.4f} ms = '
            f'{100 * bound / med:.0f} % of the kernel time; {n_sets} buffer sets rotated (HBM, not cache-resident)',
            f'    grid_sample route {statistics.median(old):.4f} ms ({min(old):.4f} / {max(old):.4f}); route / new call '
            f'{statistics.median(ratio):.2f}x ({min(ratio):.2f} / {max(ratio):.2f} over the rounds): the new call is {verdict}',
            f'    identical to the restatement: {ok}; grid_sample route differs from it in {route_diff[0]:.2%} of the bytes, by at most '
            f'{route_diff[1]} grey levels (other coordinates and float weights: not a check)',
            f'    host, numpy restatement (stand-in for cv2, not installed), one run: {host_ms:.0f} ms']


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def diff(a, b):
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    return float((d != 0).mean()), int(d.max())


def n_sets_for(nbytes):
    return int(np.ceil(CACHE / nbytes)) + 1


def bench_map(name, img, m, a):
    """img uint8 numpy, m numpy or device tensor"""
    m_dev = m if torch.is_tensor(m) else torch.from_numpy(m).cuda()
    nbytes = m_dev.numel() * m_dev.element_size() + m_dev.shape[0] * m_dev.shape[1] * img.shape[2] + img.size
    n = n_sets_for(nbytes)
    imgs = [torch.from_numpy(img).cuda() for _ in range(n)]
    ms = [m_dev.clone() for _ in range(n)]
    dsts = [torch.empty(tuple(m_dev.shape[:2]) + (img.shape[2],), dtype=torch.uint8, device='cuda') for _ in range(n)]
    lib, stream = _lib.load_library(), _lib.current_stream_ptr()
    f64 = int(m_dev.dtype == torch.float64)

    def new(k):
        assert lib.cotr_warp_map(p(imgs[k]), img.shape[0], img.shape[1], img.shape[2], p(ms[k]), f64, m_dev.shape[0], m_dev.shape[1],
                                 p(dsts[k]), None, None, stream) == 0
    fns = {'new': new, 'grid_sample': lambda k: grid_route_map(imgs[k], ms[k])}
    ts = timed_pair(fns, n, a.warmup, a.iters, a.rounds)
    got, route = warp_by_map(imgs[0], ms[0]), fns['grid_sample'](0).cpu().numpy()
    assert np.array_equal(dsts[0].cpu().numpy(), got)
    t0 = time.perf_counter()
    want, _ = wo.remap(img, m_dev.cpu().numpy())
    host = (time.perf_counter() - t0) * 1e3
    return report(name, ts, nbytes, n, np.array_equal(got, want), diff(route, want), host)


def bench_paste(a):
    picture, img_b = wo.image(1200, 1000, 3, 1), wo.image(4000, 3000, 3, 2)
    T = get_perspective_transform(picture_corners(picture.shape), np.float32([[932, 1025], [2469, 901], [908, 2927], [2436, 3080]]))
    Tinv = invert_perspective(T)
    nbytes = 2 * img_b.size + picture.size
    n = n_sets_for(nbytes)
    pics = [torch.from_numpy(picture).cuda() for _ in range(n)]
    bgs = [torch.from_numpy(img_b).cuda() for _ in range(n)]
    Td = torch.from_numpy(Tinv).cuda()
    dsts = [torch.empty_like(b) for b in bgs]
    lib, stream = _lib.load_library(), _lib.current_stream_ptr()
    Mc = np.ascontiguousarray(Tinv).ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def new(k):
        assert lib.cotr_warp_perspective(p(pics[k]), 1200, 1000, 3, Mc, 4000, 3000, p(dsts[k]), None, p(bgs[k]), stream) == 0
    fns = {'new': new, 'grid_sample': lambda k: grid_route_paste(pics[k], Td, bgs[k])}
    ts = timed_pair(fns, n, a.warmup, a.iters, a.rounds)
    got = warp_perspective(pics[0], Tinv, (3000, 4000), inverse_map=True, background=bgs[0])
    route = fns['grid_sample'](0).cpu().numpy()
    assert np.array_equal(dsts[0].cpu().numpy(), got)
    t0 = time.perf_counter()
    want, _ = wo.warp_perspective(picture, Tinv, 4000, 3000, img_b)
    host = (time.perf_counter() - t0) * 1e3
    return report('homography: 1200 x 1000 x 3 pasted into 4000 x 3000 x 3, cotr_warp_perspective with background', ts, nbytes, n,
                  np.array_equal(got, want), diff(route, want), host)


def single_pair_map():
    verts, tris = ro.jittered_grid(12, 9, 0.4, 3, lo=0.05, hi=0.95)
    pb = verts.astype(np.float64) * [0.8, 0.85] + 0.08
    corr = np.hstack([verts.astype(np.float64) * [1024, 768], pb * [1024, 768]])
    return triangulate_corr(corr, (768, 1024), (768, 1024), simplices=tris, as_tensor=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'warp_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_warp.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls after '
             f'{a.warmup} warm-up calls, the new call (the C entry point, outputs allocated once) and the grid_sample route alternating; '
             f'host times once, host clock']
    lines += bench_map('single_pair: 768 x 1024 x 3 by a 768 x 1024 float64 triangulate_corr map, cotr_warp_map',
                       wo.image(768, 1024, 3, 0), single_pair_map(), a)
    lines += bench_paste(a)
    lines += bench_map('smooth 12 MP: 3000 x 4000 x 3 by a 3000 x 4000 float32 smooth random map, cotr_warp_map',
                       wo.image(3000, 4000, 3, 4), wo.smooth_map(3000, 4000, 3000, 4000, 5, margin=0.02), a)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
