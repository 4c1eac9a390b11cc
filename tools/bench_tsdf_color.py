"""Colour volume timings: cotr_tsdf_color_integrate (cotr_amd/csrc/tsdf.hip) at 128^3 and 256^3 voxels with 1 and 8 captures of
480 x 640 of the three-plane corner of tests/icp_oracle.py with the textured images of tests/tsdf_color_oracle.py, beside
cotr_tsdf_integrate on the same inputs in the same run, each against the bytes it moves (the colour call reads 16 B a voxel and
writes 16 B a voxel a capture coloured; the depth call reads 8 B a voxel and writes 8 B a voxel a capture updated);
cotr_tsdf_color_map of the raycast of the fused 128^3 volume at 480 x 640, and cotr_tsdf_color_points on the vertices of its
mesh, against the bytes of their inputs and outputs and of the eight 16 B corners a pixel or point gathers.  The device results
at 128^3 are checked against the numpy restatement on the same host.

The volume: origin (-3.9, -3.0, 2.9), 6.4 a side (voxel 0.05 at 128^3, 0.025 at 256^3), trunc 3 voxels; the raycast from the first
camera, near 0.5, far 8, step trunc / 2.  Device times: HIP events around `--iters` calls after `--warmup`, median over `--rounds`
rounds (min / max shown).
GPU box:  python tools/bench_tsdf_color.py [--out profiles/tsdf_color_bench.txt]
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
from cotr_amd.inference import TsdfVolume, extract_mesh, integrate_colors, integrate_depths, raycast_volume
from cotr_amd.inference._args import camera
from tests import icp_oracle as io
from tests import tsdf_color_oracle as tc
from tests import tsdf_oracle as to

ORIGIN, SIDE, SHAPE = (-3.9, -3.0, 2.9), 6.4, (480, 640)
p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731


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


def ms(t):
    return f'{t[0]:.4f} ms ({t[1]:.4f} / {t[2]:.4f})'


def bench_integrate(N, n, depths, images, Ks, c2ws, a):
    """both integrate calls through the C ABI with everything prepared: the times are the library's, not the wrapper's"""
    lib = _lib.load_library()
    vol = TsdfVolume(ORIGIN, SIDE / N, (N, N, N), color=True)
    d, im = torch.from_numpy(depths[:n]).cuda(), torch.from_numpy(np.ascontiguousarray(images[:n])).cuda()
    c = torch.from_numpy(np.ascontiguousarray(c2ws[:n].reshape(n, 16))).cuda()
    K = (ctypes.c_double * (9 * n))(*np.asarray(Ks[:n], np.float64).reshape(-1))
    info, cinfo = torch.empty((n, 4), dtype=torch.int32, device='cuda'), torch.empty((n, 4), dtype=torch.int32, device='cuda')
    origin, stream = (ctypes.c_double * 3)(*vol.origin), _lib.current_stream_ptr()

    def depth_call():
        assert lib.cotr_tsdf_integrate(p(vol.tsdf), p(vol.weight), N, N, N, origin, vol.voxel, vol.trunc, p(d), n, SHAPE[0], SHAPE[1], K, p(c), None, None,
                                       vol.max_weight, p(info), stream) == 0

    def color_call():
        assert lib.cotr_tsdf_color_integrate(p(vol.color), N, N, N, origin, vol.voxel, vol.trunc, p(d), p(im), n, SHAPE[0], SHAPE[1], K, p(c), None, None,
                                             vol.max_weight, p(cinfo), stream) == 0
    td, tcol = timed(depth_call, a.warmup, a.iters, a.rounds), timed(color_call, a.warmup, a.iters, a.rounds)
    info, cinfo = info.cpu().numpy(), cinfo.cpu().numpy()
    touched = lambda rows: int(min(rows[:, 1].sum(), N ** 3))   # noqa: E731  (at most: voxels two captures reach are written once)
    bd, bc = 8 * N ** 3 + 8 * touched(info), 16 * N ** 3 + 16 * touched(cinfo)
    cap = f'{n} capture{"s" if n > 1 else ""}'
    return [f'integrate {N}^3 ({N ** 3 / 1e6:.1f} M voxels), {cap} of {SHAPE[0]} x {SHAPE[1]} (2 launches each):',
            f'    colour {ms(tcol)}; at most {bc / 1e6:.1f} MB = {bc / (tcol[0] * 1e-3) / 1e9:.0f} GB/s, {N ** 3 * n / (tcol[0] * 1e-3) / 1e9:.2f} G voxel-captures/s; '
            f'coloured {cinfo[:, 1].tolist()} of valid {cinfo[:, 2].tolist()}',
            f'    depth  {ms(td)}; at most {bd / 1e6:.1f} MB = {bd / (td[0] * 1e-3) / 1e9:.0f} GB/s, {N ** 3 * n / (td[0] * 1e-3) / 1e9:.2f} G voxel-captures/s; '
            f'updated {info[:, 1].tolist()}; the pair {td[0] + tcol[0]:.4f} ms, colour / depth {tcol[0] / td[0]:.2f}']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tsdf_color_bench.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_tsdf_color.py measures the GPU: no device found'
    lines = [f'device: {torch.cuda.get_device_name(0)}; HIP events, median (min / max) over {a.rounds} rounds of {a.iters} calls '
             f'after {a.warmup} warm-up calls']
    depths, Ks, c2ws = to.captures(*SHAPE, 8)
    images = tc.images(*SHAPE, 8)
    for N in (128, 256):
        for n in (1, 8):
            lines += bench_integrate(N, n, depths, images, Ks, c2ws, a)
    # the two captures fused at 128^3: the colour of its raycast and of its mesh, and all of it against the restatement
    N, lib = 128, _lib.load_library()
    vol = TsdfVolume(ORIGIN, SIDE / N, (N, N, N), color=True)
    integrate_depths(vol, depths[:2], Ks[:2], c2ws[:2])
    integrate_colors(vol, depths[:2], images[:2], Ks[:2], c2ws[:2], weights=tc.FUSED_WEIGHTS)
    K, pose = io.scaled_camera(io.corner_scene()['K_a'], *SHAPE), c2ws[0]
    depth = raycast_volume(vol, K, pose, SHAPE, near=0.5, far=8.0, step=vol.trunc / 2)['depth']
    verts = extract_mesh(vol)[0]
    V = int(verts.shape[0])
    k, c = camera(K, 'K'), torch.from_numpy(pose.reshape(16)).cuda()
    rgb, minfo = torch.empty(SHAPE + (3,), dtype=torch.uint8, device='cuda'), torch.empty(4, dtype=torch.int32, device='cuda')
    vrgb, vok, pinfo = torch.empty((V, 3), dtype=torch.uint8, device='cuda'), torch.empty(V, dtype=torch.uint8, device='cuda'), torch.empty(4, dtype=torch.int32, device='cuda')
    origin, stream = (ctypes.c_double * 3)(*vol.origin), _lib.current_stream_ptr()

    def map_call():
        assert lib.cotr_tsdf_color_map(p(vol.color), N, N, N, origin, vol.voxel, p(depth), SHAPE[0], SHAPE[1], k, p(c), None, p(rgb), p(minfo), stream) == 0

    def points_call():
        assert lib.cotr_tsdf_color_points(p(vol.color), N, N, N, origin, vol.voxel, p(verts), V, None, p(vrgb), p(vok), p(pinfo), stream) == 0
    tm, tp = timed(map_call, a.warmup, a.iters, a.rounds), timed(points_call, a.warmup, a.iters, a.rounds)
    minfo, pinfo = minfo.cpu().numpy(), pinfo.cpu().numpy()
    pixels = SHAPE[0] * SHAPE[1]
    bm, gm = 7 * pixels, 128 * int(minfo[2])
    bp, gp = 28 * V, 128 * V
    o = tc.integrate(tc.fresh(vol.dims), ORIGIN, vol.voxel, vol.trunc, depths[:2], images[:2], Ks[:2], c2ws[:2], weights=tc.FUSED_WEIGHTS)
    om = tc.color_map(o['color'], ORIGIN, vol.voxel, depth.cpu().numpy(), K, pose)
    v = verts.cpu().numpy()
    op = tc.sample(o['color'], ORIGIN, vol.voxel, v)
    same_vol = np.array_equal(vol.color.cpu().numpy(), o['color'])
    same_map = np.array_equal(rgb.cpu().numpy()[~om['near']], om['rgb'][~om['near']]) and (om['near'].any() or list(minfo) == list(om['info']))
    same_pts = np.array_equal(vrgb.cpu().numpy()[~op[2]], op[0][~op[2]]) and np.array_equal(vok.cpu().numpy()[~op[2]] != 0, op[1][~op[2]])
    em = tc.texture_error(om['rgb'], om['rgb'].any(-1), tc.lift(depth.cpu().numpy(), K, pose)[0])
    ep = tc.texture_error(op[0], op[1], v)
    lines += [f'colour of a depth map, {N}^3 at {SHAPE[0]} x {SHAPE[1]} (2 launches): {ms(tm)}; {minfo[1]} of {minfo[2]} pixels with a depth coloured = '
              f'{minfo[2] / (tm[0] * 1e-3) / 1e9:.2f} G pixels/s; {bm / 1e6:.1f} MB of depth and bytes + {gm / 1e6:.1f} MB of corners gathered = '
              f'{(bm + gm) / (tm[0] * 1e-3) / 1e9:.0f} GB/s',
              f'    against the texture: median {em[0].round(2).tolist()}, p90 {em[1].round(2).tolist()} (0 .. 255, per channel)',
              f'colour of the mesh vertices, {N}^3, {V} vertices (2 launches): {ms(tp)}; {pinfo[1]} valid = {V / (tp[0] * 1e-3) / 1e9:.2f} G points/s; '
              f'{bp / 1e6:.1f} MB of points and bytes + {gp / 1e6:.1f} MB of corners gathered = {(bp + gp) / (tp[0] * 1e-3) / 1e9:.0f} GB/s',
              f'    against the texture: median {ep[0].round(2).tolist()}, p90 {ep[1].round(2).tolist()}',
              f'    colour volume identical to the restatement: {same_vol} ({int(o["near"].sum())} voxels flagged); the map: {same_map} ({int(om["near"].sum())} '
              f'pixels flagged); the vertices: {same_pts} ({int(op[2].sum())} flagged)']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
