"""The TSDF volume on the MI355X (cotr_amd/csrc/tsdf.hip) against the numpy restatement tests/tsdf_oracle.py: the volume after
every integration and the raycast's depth map and normals bit for bit (NaN where the restatement has NaN), the counts exactly,
at the smallest sizes at which the indexing can go wrong; the ``found`` gate, repeatability, and the wrappers on top.

Voxels and pixels the restatement flags as near a decision (within 1e-9) may be left out of a comparison, at most 0.1 % of a
case; every case prints its share.  The two accuracy figures - the raycast depth against the scene's renderer and the tracked
pose against the scene - are held to 1.5 times the restatement's own figure on the same case (the family's factor, as
tests/test_icp_gpu.py).  Measured figures: DESIGN.md 3h-11."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.data import Capture
from cotr_amd.inference import TsdfVolume, ZoomEngine, fuse_captures, integrate_depths, raycast_volume, track_capture
from cotr_amd.inference import _args, tsdf as tsdf_mod
from tests import icp_oracle as io
from tests import pnp_oracle as po
from tests import tsdf_oracle as to

pytestmark = pytest.mark.gpu

CAP = 0.001
VOLUMES = ((2, 2, 2), (3, 5, 7), (4, 4, 4), (7, 3, 3), (65, 2, 2), (67, 3, 2), (8, 8, 8), (64, 64, 64))
MAPS = ((24, 32), (48, 64))


def origin_of(dims):
    return to.ORIGIN_64 if dims == (64, 64, 64) else to.small_origin(dims)


def same_volume(vol, o, what):
    """the device's volume against the restatement's, outside the flagged voxels -> their share"""
    torch.cuda.synchronize()
    T, Wt = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()
    keep = ~o['near']
    share = to.share(o['near'])
    assert share <= CAP, (what, share)
    assert T.shape == o['tsdf'].shape and np.array_equal(T[keep], o['tsdf'][keep]) and np.array_equal(Wt[keep], o['weight'][keep]), what
    return share


def integrate_both(vol, state, depths, Ks, c2ws, found=None, weights=None, on_device=False):
    """one call on the device (``on_device``: poses and ``found`` as device tensors) and in the restatement (from ``state`` = (tsdf,
    weight)) -> (info of the device, the restatement's dict)"""
    f = None if found is None else (torch.tensor(found, dtype=torch.int32, device='cuda') if on_device else np.asarray(found))
    info = integrate_depths(vol, depths, Ks, torch.from_numpy(c2ws).cuda() if on_device else c2ws, found=f, weights=weights).cpu().numpy()
    o = to.integrate(*state, vol.origin, vol.voxel, vol.trunc, depths, Ks, c2ws, found=found, weights=weights, max_weight=vol.max_weight)
    return info, o


# ---- integration ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', MAPS, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('dims', VOLUMES, ids=lambda d: 'x'.join(str(v) for v in d))
def test_integration_at_every_size_with_a_second_call_and_the_cap(dims, shape):
    depths, Ks, c2ws = to.captures(*shape)
    vol = TsdfVolume(origin_of(dims), to.VOXEL_64, dims, max_weight=3.0)
    assert (vol.tsdf == 1).all() and (vol.weight == 0).all() and vol.trunc == 3 * to.VOXEL_64 and tuple(vol.tsdf.shape) == dims[::-1]
    info, o = integrate_both(vol, to.fresh(dims), depths, Ks, c2ws)
    share = same_volume(vol, o, 'first call')
    assert np.array_equal(info, o['info']) and (info[:, 1] > 0).all(), (info, o['info'])
    # the same captures again with other weights: accumulation, and the cap at 3
    info2, o2 = integrate_both(vol, (o['tsdf'], o['weight']), depths, Ks, c2ws, weights=[1.5, 0.75])
    o2['near'] |= o['near']
    share2 = same_volume(vol, o2, 'second call')
    assert np.array_equal(info2, o2['info']) and np.array_equal(info2, info)
    assert (o2['weight'] == 3.0).any() and (o2['weight'] <= 3.0).all() and not np.array_equal(o2['tsdf'], o['tsdf'])
    print(f'{dims} with maps {shape}: updated {info[:, 1].tolist()}, valid {info[:, 2].tolist()}, flagged {100 * share:.4f} % / {100 * share2:.4f} % of the voxels')
    if dims == (64, 64, 64) and shape == (48, 64):
        assert info[:, 1].tolist() == [62639, 49100]


@pytest.mark.parametrize('n', [1, 2, 3, 32])
@pytest.mark.parametrize('dims', [(8, 8, 8), (67, 3, 2)], ids=['8x8x8', '67x3x2'])
def test_captures_per_call(dims, n):
    depths, Ks, c2ws = to.captures(24, 32, n)
    weights = [1.0 + 0.25 * (c % 3) for c in range(n)]
    vol = TsdfVolume(origin_of(dims), to.VOXEL_64, dims, max_weight=20.0)
    info, o = integrate_both(vol, to.fresh(dims), depths, Ks, c2ws, weights=weights)
    share = same_volume(vol, o, f'{n} captures')
    assert info.shape == (n, 4) and np.array_equal(info, o['info']) and (info[:, 0] == 1).all()
    assert (o['weight'] == 20.0).any() == (n == 32)
    # and the same bits as n calls of one capture each
    one = TsdfVolume(origin_of(dims), to.VOXEL_64, dims, max_weight=20.0)
    rows = [integrate_depths(one, depths[c:c + 1], Ks[c:c + 1], c2ws[c:c + 1], weights=weights[c:c + 1]) for c in range(n)]
    assert torch.equal(one.tsdf, vol.tsdf) and torch.equal(one.weight, vol.weight) and np.array_equal(torch.cat(rows).cpu().numpy(), info)
    print(f'{dims}, {n} captures in one call: flagged {100 * share:.4f} % of the voxels')


@pytest.mark.parametrize('on_device', [True, False], ids=['device', 'host'])
def test_found_skips_the_first_a_middle_and_the_last_capture(on_device):
    depths, Ks, c2ws = to.captures(24, 32, 5)
    dims, found = (8, 8, 8), [0, 1, 0, 1, 0]
    vol = TsdfVolume(origin_of(dims), to.VOXEL_64, dims)
    info, o = integrate_both(vol, to.fresh(dims), depths, Ks, c2ws, found=found, on_device=on_device)
    same_volume(vol, o, 'found')
    assert np.array_equal(info, o['info']) and (info[[0, 2, 4]] == 0).all() and (info[[1, 3], 0] == 1).all() and (info[[1, 3], 1] > 0).all()
    # nothing found: the volume stays fresh
    vol.reset()
    info, _ = integrate_both(vol, to.fresh(dims), depths, Ks, c2ws, found=[0] * 5)
    assert (info == 0).all() and (vol.tsdf == 1).all() and (vol.weight == 0).all()


def test_more_than_32_captures_go_in_calls_of_32():
    depths, Ks, c2ws = to.captures(24, 32, 35)
    dims = (7, 3, 3)
    vol = TsdfVolume(origin_of(dims), to.VOXEL_64, dims)
    info, o = integrate_both(vol, to.fresh(dims), depths, Ks, c2ws)
    same_volume(vol, o, '35 captures')
    assert info.shape == (35, 4) and np.array_equal(info, o['info'])


# ---- the raycast ----------------------------------------------------------------------------------------------------------
_FUSED = {}


def fused_volume():
    """the corner's two 48 x 64 captures in the 64^3 volume, integrated on the device once and checked against the restatement"""
    if 'vol' not in _FUSED:
        f = to.fused()
        vol = TsdfVolume(f['origin'], f['voxel'], f['dims'])
        integrate_depths(vol, *to.captures(48, 64))
        same_volume(vol, f, 'the fused corner')
        _FUSED['vol'] = vol
    return _FUSED['vol']


def camera(where, shape):
    sc = io.corner_scene()
    pose = sc['c2w_a'].copy()
    if where == 'inside':      # between the volume's near face (z = 1) and the far wall, off the voxel centres
        pose[:3, 3] = (0.213, -0.107, 3.021)
    return io.scaled_camera(sc['K_a'], *shape), pose


def check_raycast(shape, where, near, far, step, what):
    f, vol = to.fused(), fused_volume()
    K, pose = camera(where, shape)
    r = raycast_volume(vol, K, pose, shape, near=near, far=far, step=step, normals=True)
    torch.cuda.synchronize()
    depth, normals, info = (r[k].cpu().numpy() for k in ('depth', 'normals', 'info'))
    o = to.raycast(f['tsdf'], f['weight'], f['origin'], f['voxel'], K, pose, shape, near, far, step, normals=True)
    keep, share = ~o['near'], to.share(o['near'])
    assert share <= CAP, (what, share)
    assert depth.dtype == np.float32 and depth.shape == shape and np.array_equal(depth[keep], o['depth'][keep]), what
    assert normals.shape == shape + (3,) and np.array_equal(normals[keep], o['normals'][keep], equal_nan=True), what
    if not o['near'].any():
        assert np.array_equal(info, o['info']), (what, info, o['info'])
    print(f'{what}: info {info.tolist()}, {int(np.isfinite(normals[..., 0]).sum())} normals, {o["samples"]} samples, flagged {100 * share:.4f} % of the pixels')
    return depth, normals, info, o


SHAPES = ((1, 1), (3, 3), (7, 9), (8, 8), (5, 13), (48, 64))


@pytest.mark.parametrize('where', ['outside', 'inside'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_raycast_at_every_size_from_outside_and_inside_the_box(shape, where):
    # 7.56 / 0.15 = 50.4: the last sample lies beyond far
    assert to.steps(0.37, 7.93, 0.15) == 51 and 0.37 + 50 * 0.15 < 7.93 < 0.37 + 51 * 0.15
    depth, normals, info, o = check_raycast(shape, where, 0.37, 7.93, 0.15, f'{shape} from {where}')
    assert info[0] == 1 and info[1] == (depth > 0).sum()
    if shape == (48, 64):
        assert info[1] > 1500 and np.isfinite(normals[..., 0]).sum() > 1000


@pytest.mark.parametrize('where, far', [('outside', 5.2), ('inside', 3.3)])
def test_raycast_with_a_far_that_ends_inside_the_box(where, far):
    # the far wall lies at z of about 6, 3 in front of the camera inside: a walk that ends at 5.2 from outside reaches the side walls
    # only, one that ends at 3.3 from inside the middle of the far wall only
    full = check_raycast((48, 64), where, 0.0, 9.0, 0.15, f'far 9.0 from {where}')
    short = check_raycast((48, 64), where, 0.0, far, 0.15, f'far {far} from {where}')
    assert 0 < short[2][1] < full[2][1]
    reached = short[0] > 0
    assert np.array_equal(short[0][reached], full[0][reached])


def test_raycast_defaults_and_a_device_pose():
    vol = fused_volume()
    K, pose = camera('outside', (48, 64))
    far = float(np.linalg.norm(vol.corners() - pose[:3, 3], axis=1).max())
    a = raycast_volume(vol, K, pose, (48, 64))
    b = raycast_volume(vol, K, torch.from_numpy(pose).cuda(), (48, 64), near=0.0, far=far, step=vol.trunc / 2)
    assert sorted(a) == ['depth', 'info'] and torch.equal(a['depth'], b['depth']) and torch.equal(a['info'], b['info']) and a['info'][1] > 1500
    with pytest.raises(ValueError, match='far must be given'):
        raycast_volume(vol, K, torch.from_numpy(pose).cuda(), (48, 64))
    # the map is a valid input of the integration: the model fused into a second volume
    again = TsdfVolume(vol.origin, vol.voxel, vol.dims)
    info = integrate_depths(again, a['depth'][None], K, pose[None]).cpu().numpy()
    o = to.integrate(*to.fresh(vol.dims), vol.origin, vol.voxel, vol.trunc, a['depth'].cpu().numpy()[None], K[None], pose[None])
    same_volume(again, o, 'the raycast map fused')
    assert np.array_equal(info, o['info']) and info[0, 1] > 10000


def test_the_raycast_depth_against_the_renderer():
    f, vol = to.fused(), fused_volume()
    sc = io.scene(48, 64, 48, 64, 3)
    ref = io.render(48, 64, sc['K_a'], sc['c2w_a'], io.PLANES)
    d = raycast_volume(vol, sc['K_a'], sc['c2w_a'], (48, 64), near=0.5, far=8.0)['depth'].cpu().numpy()
    o = to.raycast(f['tsdf'], f['weight'], f['origin'], f['voxel'], sc['K_a'], sc['c2w_a'], (48, 64), 0.5, 8.0, f['trunc'] / 2)['depth']
    assert ((d > 0) == (o > 0)).all() and (d > 0).sum() == 2353
    e, w = np.abs(d - ref)[d > 0], np.abs(o - ref)[o > 0]
    print(f'raycast of the fused corner against the renderer: median {np.median(e):.3e} (restatement {np.median(w):.3e}), '
          f'p90 {np.percentile(e, 90):.3e} ({np.percentile(w, 90):.3e}), max {e.max():.3e} ({w.max():.3e})')
    assert np.median(e) <= 1.5 * np.median(w) and np.percentile(e, 90) <= 1.5 * np.percentile(w, 90) and e.max() <= 1.5 * w.max()


def test_a_crossing_from_behind_ends_the_ray_and_an_unobserved_slab_resets_the_walk():
    c = to.crossings()
    vol = TsdfVolume(c['origin'], c['voxel'], c['dims'])
    gap = c['weight'].copy()
    gap[21:23] = 0
    for near, weight, want in ((0.52, c['weight'], [1, 25, 0, 0]), (1.83, c['weight'], [1, 0, 25, 0]), (1.83, gap, [1, 25, 0, 0])):   # no sample on a crossing
        vol.tsdf.copy_(torch.from_numpy(c['tsdf']))
        vol.weight.copy_(torch.from_numpy(weight))
        r = raycast_volume(vol, c['K'], c['c2w'], c['shape'], near=near, far=3.8, step=0.15, normals=True)
        o = to.raycast(c['tsdf'], weight, c['origin'], c['voxel'], c['K'], c['c2w'], c['shape'], near, 3.8, 0.15, normals=True)
        assert r['info'].tolist() == want == o['info'].tolist() and not o['near'].any()
        assert np.array_equal(r['depth'].cpu().numpy(), o['depth']) and np.array_equal(r['normals'].cpu().numpy(), o['normals'], equal_nan=True)


# ---- the gate and repeatability ---------------------------------------------------------------------------------------------
def test_found_0_zeroes_every_output_of_the_raycast():
    vol = fused_volume()
    K, pose = camera('outside', (7, 9))
    k, c2w = _args.camera(K, 'K'), torch.from_numpy(pose.reshape(16)).cuda()
    with torch.cuda.device(vol.device):
        off = tsdf_mod._enqueue_raycast(_lib.load_library(), vol, k, c2w, torch.zeros(1, dtype=torch.int32, device='cuda'), 7, 9, 0.0, 8.0, 0.15, True)
        on_ = tsdf_mod._enqueue_raycast(_lib.load_library(), vol, k, c2w, torch.ones(1, dtype=torch.int32, device='cuda'), 7, 9, 0.0, 8.0, 0.15, True)
        free = tsdf_mod._enqueue_raycast(_lib.load_library(), vol, k, c2w, None, 7, 9, 0.0, 8.0, 0.15, True)
    for key in ('depth', 'normals', 'info'):
        assert (off[key] == 0).all(), key
        assert np.array_equal(on_[key].cpu().numpy(), free[key].cpu().numpy(), equal_nan=True), key
    assert free['info'][0] == 1 and free['info'][1] > 0


def test_same_bits_across_calls_streams_and_graph_replay():
    f = to.fused()
    depths, Ks, c2ws = to.captures(48, 64)
    K, pose = camera('outside', (48, 64))
    lib = _lib.load_library()
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    d_dev, c_dev, pose_dev = cu(depths), cu(c2ws.reshape(2, 16)), cu(pose.reshape(16))
    K2 = (ctypes.c_double * 18)(*Ks.reshape(-1))
    K1 = _args.camera(K, 'K')
    origin = (ctypes.c_double * 3)(*f['origin'])

    def buffers():
        return dict(tsdf=torch.ones((64, 64, 64), dtype=torch.float32, device='cuda'), weight=torch.zeros((64, 64, 64), dtype=torch.float32, device='cuda'),
                    info=torch.full((2, 4), -3, dtype=torch.int32, device='cuda'), depth=torch.full((48, 64), -7.0, dtype=torch.float32, device='cuda'),
                    normals=torch.full((48, 64, 3), -7.0, dtype=torch.float64, device='cuda'), rinfo=torch.full((4,), -3, dtype=torch.int32, device='cuda'))

    def enqueue(b, stream):
        rc = lib.cotr_tsdf_integrate(p(b['tsdf']), p(b['weight']), 64, 64, 64, origin, f['voxel'], f['trunc'], p(d_dev), 2, 48, 64, K2, p(c_dev), None, None,
                                     64.0, p(b['info']), stream)
        assert rc == 0, lib.cotr_raster_last_error()
        rc = lib.cotr_tsdf_raycast(p(b['tsdf']), p(b['weight']), 64, 64, 64, origin, f['voxel'], K1, p(pose_dev), None, 48, 64, 0.0, 9.0, 0.15,
                                   p(b['depth']), p(b['normals']), p(b['rinfo']), stream)
        assert rc == 0, lib.cotr_raster_last_error()

    def same(a, b):
        for key in a:
            assert np.array_equal(a[key].cpu().numpy(), b[key].cpu().numpy(), equal_nan=True), key
    first, again = buffers(), buffers()
    here = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    enqueue(first, here)
    enqueue(again, here)
    torch.cuda.synchronize()
    same(first, again)
    assert np.array_equal(first['tsdf'].cpu().numpy(), f['tsdf']) and first['info'][:, 1].tolist() == [62639, 49100] and first['rinfo'][1] > 1500
    b = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    enqueue(b, ctypes.c_void_p(side.cuda_stream))
    side.synchronize()
    same(first, b)
    # captured once (a single linear chain on the capture stream), replayed once
    b = buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue(b, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    graph.replay()
    torch.cuda.synchronize()
    same(first, b)


# ---- the wrappers on top ----------------------------------------------------------------------------------------------------
def test_fuse_captures_then_track_capture_of_b_from_the_scene_start():
    f = to.fused()
    sc = io.scene(48, 64, 48, 64, 3)
    cap_a, cap_b = Capture(None, sc['depth_a'], sc['K_a'], sc['c2w_a']), Capture(None, torch.from_numpy(sc['depth_b']).cuda(), sc['K_b'], sc['c2w_b'])
    vol, infos = fuse_captures([cap_a, cap_b], origin=f['origin'], voxel=f['voxel'], dims=f['dims'])
    same_volume(vol, f, 'fuse_captures')
    assert infos == [dict(integrated=True, updated=62639, valid=int(f['info'][0, 2])), dict(integrated=True, updated=49100, valid=int(f['info'][1, 2]))]
    # captures of two sizes: neighbours of one size share a call, the list order is kept
    small = to.captures(24, 32)
    mixed = [cap_a, Capture(None, small[0][1], small[1][1], small[2][1]), cap_b]
    vol3, infos3 = fuse_captures(mixed, origin=f['origin'], voxel=f['voxel'], dims=f['dims'])
    o = to.fresh(f['dims'])
    for cap in mixed:
        depth = cap.depth.cpu().numpy() if torch.is_tensor(cap.depth) else cap.depth
        r = to.integrate(*o, f['origin'], f['voxel'], f['trunc'], depth[None], cap.K[None], cap.c2w[None])
        o = (r['tsdf'], r['weight'])
    assert np.array_equal(vol3.tsdf.cpu().numpy(), o[0]) and np.array_equal(vol3.weight.cpu().numpy(), o[1]) and len(infos3) == 3
    # frame-to-model tracking of B from the scene's start, against the restatement of the same two steps
    start = sc['c2w_a'] @ np.vstack([np.hstack([sc['R0'], sc['t0'][:, None]]), [0, 0, 0, 1]])
    c2w, info = track_capture(vol, cap_b, start, max_dist=0.25, near=0.5, far=8.0)
    model = to.raycast(f['tsdf'], f['weight'], f['origin'], f['voxel'], sc['K_b'], start, (48, 64), 0.5, 8.0, f['trunc'] / 2)['depth']
    ro = io.icp(io.maps(model, sc['K_b']), sc['K_b'], sc['maps_b'], np.eye(3), np.zeros(3), iters=10, max_dist=0.25)
    ow = start @ np.vstack([np.hstack([ro['R'], ro['t'][:, None]]), [0, 0, 0, 1]])
    truth = dict(R=sc['c2w_b'][:3, :3], t=sc['c2w_b'][:3, 3])
    s, d, w = io.errors(start[:3, :3], start[:3, 3], truth), io.errors(c2w[:3, :3], c2w[:3, 3], truth), io.errors(ow[:3, :3], ow[:3, 3], truth)
    print(f'track_capture of B against the model from {s[0]:.3e} / {s[1]:.3e}: rotation {d[0]:.3e} (restatement {w[0]:.3e}), translation {d[1]:.3e} '
          f'({w[1]:.3e}), {info["pairs"]} pairs, stop {info["stop"]!r}')
    assert info['ok'] and ro['info'][0] == 1 and info['steps'] == 10 and c2w.shape == (4, 4) and np.array_equal(c2w[3], [0, 0, 0, 1])
    assert d[0] <= 1.5 * w[0] and d[1] <= 1.5 * w[1]


def test_zoom_engine_fuse():
    from tests.engine_fixtures import CyclicFakeModel, synthetic_pair
    img_a, img_b = synthetic_pair(1)
    H, W = img_a.shape[:2]
    Hb, Wb = img_b.shape[:2]
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    depth_a = (4.0 + xs / 64.0 + ys / 128.0).astype(np.float32)
    xs, ys = np.meshgrid(np.arange(Wb), np.arange(Hb))
    depth_b = (3.5 + xs / 96.0 + ys / 80.0).astype(np.float32)
    K_a = np.array([[300.0, 0.5, W / 2], [0.0, 310.0, H / 2], [0.0, 0.0, 1.0]])
    K_b = np.array([[280.0, -0.5, Wb / 2], [0.0, 290.0, Hb / 2], [0.0, 0.0, 1.0]])
    cap_a = Capture(img_a, depth_a, K_a, po.pose_matrix((5.0, -3.0, 2.0), (0.3, 0.1, -0.2)))
    cap_b = Capture(img_b, depth_b, K_b, np.eye(4))
    eng = ZoomEngine(CyclicFakeModel().cuda())
    rng = np.random.default_rng(0)
    q = np.stack([rng.uniform(5, W - 5, 40), rng.uniform(5, H - 5, 40)], 1).astype(np.float32)
    kw = dict(queries_a=q, threshold=0.5, max_iters=100, seed=3, icp_max_dist=0.3)
    make = lambda: TsdfVolume((-2.0, -2.0, 3.0), 0.125, (40, 36, 33))   # noqa: E731
    with torch.no_grad():
        vol, poses, found = eng.fuse([cap_a, cap_b], make(), icp_iters=2, **kw)
        c2w = eng.register(cap_a, cap_b, icp_iters=2, **kw)[0]
    assert len(poses) == 2 and np.array_equal(poses[0], cap_a.c2w) and found == [True, c2w is not None] and (vol.weight > 0).any()
    assert (poses[1] is None) == (c2w is None)
    placed = [cap_a] + ([cap_b._replace(c2w=c2w)] if c2w is not None else [])
    if c2w is not None:
        assert np.array_equal(poses[1], c2w)
    want, infos = fuse_captures(placed, make())
    assert torch.equal(vol.tsdf, want.tsdf) and torch.equal(vol.weight, want.weight) and infos[0]['updated'] > 0
