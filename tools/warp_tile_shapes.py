"""Tile shapes of csrc/warp.hip against each other -> profiles/warp_tile_shapes.txt.

warp.hip takes its destination tile from -DWARP_TW / -DWARP_TH (4 pixels per lane, TW/4 x TH threads).  This script builds one
small library per shape (hipcc, into build/warp_tiles/, git-ignored; --build-only does just that, without a GPU), then times
them in one process, alternating round by round, on the 12-megapixel shapes, with HIP events and buffer sets rotated past the
256 MiB Infinity Cache, and checks that every variant writes the same bytes.
GPU box:  python tools/warp_tile_shapes.py [--out profiles/warp_tile_shapes.txt]
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ['256x4', '128x8', '64x16', '32x32', '16x64', '64x4', '32x8']


def build_variants():
    from cotr_amd.build import CSRC, _hipcc
    d = os.path.join(ROOT, 'build', 'warp_tiles')
    os.makedirs(d, exist_ok=True)
    libs = {}
    for v in SHAPES:
        tw, th = v.split('x')
        libs[v] = os.path.join(d, f'libwarp_{v}.so')
        subprocess.run([_hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-mcode-object-version=5', '-ffp-contract=off',
                        f'-DWARP_TW={tw}', f'-DWARP_TH={th}', '-shared', '-o', libs[v], os.path.join(CSRC, 'warp.hip'),
                        os.path.join(CSRC, 'handleless.hip')], check=True)
    return libs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--build-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'warp_tile_shapes.txt'))
    a = ap.parse_args()
    paths = build_variants()
    if a.build_only:
        print('\n'.join(paths.values()))
        return
    import numpy as np
    import torch
    from cotr_amd.inference.warp import get_perspective_transform, invert_perspective, picture_corners
    from tests import warp_oracle as wo
    assert torch.cuda.is_available(), 'warp_tile_shapes.py measures the GPU: no device found'
    libs = {v: ctypes.CDLL(f) for v, f in paths.items()}
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    img = wo.image(3000, 4000, 3, 4); m = wo.smooth_map(3000, 4000, 3000, 4000, 5, margin=0.02)
    N = 3
    imgs = [torch.from_numpy(img).cuda() for _ in range(N)]; ms = [torch.from_numpy(m).cuda() for _ in range(N)]
    m64 = [x.double() for x in ms[:2]]
    dsts = [torch.empty_like(imgs[0]) for _ in range(N)]
    pic = wo.image(1200, 1000, 3, 1); pics = [torch.from_numpy(pic).cuda() for _ in range(5)]
    bgs = [torch.from_numpy(wo.image(4000, 3000, 3, 2)).cuda() for _ in range(5)]; pd = [torch.empty_like(b) for b in bgs]
    Tinv = np.ascontiguousarray(invert_perspective(get_perspective_transform(picture_corners(pic.shape), np.float32([[932, 1025], [2469, 901], [908, 2927], [2436, 3080]]))))
    Mc = Tinv.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    gray = [x[..., 0].contiguous() for x in imgs]; gd = [torch.empty_like(g) for g in gray]
    def run(lib, what, k):
        if what == 'map12':
            rc = lib.cotr_warp_map(p(imgs[k % N]), 3000, 4000, 3, p(ms[k % N]), 0, 3000, 4000, p(dsts[k % N]), None, None, None)
        elif what == 'map12_f64':
            rc = lib.cotr_warp_map(p(imgs[k % N]), 3000, 4000, 3, p(m64[k % 2]), 1, 3000, 4000, p(dsts[k % N]), None, None, None)
        elif what == 'gray12':
            rc = lib.cotr_warp_map(p(gray[k % N]), 3000, 4000, 1, p(ms[k % N]), 0, 3000, 4000, p(gd[k % N]), None, None, None)
        else:
            rc = lib.cotr_warp_perspective(p(pics[k % 5]), 1200, 1000, 3, Mc, 4000, 3000, p(pd[k % 5]), None, p(bgs[k % 5]), None)
        assert rc == 0
    ref = {}
    lines = []
    for what in ('map12', 'map12_f64', 'gray12', 'paste'):
        ts = {n: [] for n in libs}
        for n, lib in libs.items():
            for k in range(6): run(lib, what, k)
            torch.cuda.synchronize()
            out = {'map12': dsts, 'map12_f64': dsts, 'gray12': gd, 'paste': pd}[what][0].clone()
            if what not in ref: ref[what] = out
            assert torch.equal(out, ref[what]), (what, n)
        for r in range(7):
            for n, lib in libs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for k in range(20): run(lib, what, k)
                b.record(); b.synchronize()
                ts[n].append(a.elapsed_time(b) / 20)
        for n in libs:
            lines.append(f'{what:10s} {n:7s} {statistics.median(ts[n]):.4f} ms ({min(ts[n]):.4f} / {max(ts[n]):.4f})')
            print(lines[-1], flush=True)
    hdr = (f'device: {torch.cuda.get_device_name(0)}; csrc/warp.hip built with -DWARP_TW=<w> -DWARP_TH=<h> (destination tile of a workgroup, '
           '4 pixels per lane, w/4 x h threads), the variants alternating round by round in one process; HIP events, median (min / max) over 7 '
           'rounds of 20 calls; buffers rotated over sets that together exceed the 256 MiB Infinity Cache; every variant\'s output identical.\n'
           'map12: 3000 x 4000 x 3 by a float32 smooth map; map12_f64: the same map as float64; gray12: the same with C = 1; paste: 1200 x 1000 x 3 '
           'into 4000 x 3000 x 3, cotr_warp_perspective with background.\n')
    with open(a.out, 'w') as f:
        f.write(hdr + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
