"""cotr_corr_depth and cotr_depth_consistency on the device against the numpy restatement tests/mvdepth_oracle.py (DESIGN.md
3h-16): every output of both calls bit for bit, every pixel compared, at every shape and option; bad data; the same bits across
calls, streams and a graph replay; 0xA5 bands around every output; the chain into the TSDF volume; the engine's two methods."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.data import Capture
from cotr_amd.inference import (TsdfVolume, ZoomEngine, depth_from_corr, filter_captures, filter_depths, flow_to_corr, fuse_captures,
                                raycast_volume)
from tests import mvdepth_oracle as mo

pytestmark = pytest.mark.gpu

MIN_ANGLE = 1.5
MAX_COS = float(np.cos(np.deg2rad(MIN_ANGLE)))
SIZES = [(1, 1), (2, 3), (13, 20), (17, 23), (48, 64)]
DEPTH_CASES = [(s, K) for s in SIZES for K in (1, 2, 3, 7)] + [((13, 20), 31)]
FILTER_CASES = [(s, n) for s in SIZES for n in (2, 3, 5)] + [((13, 20), 32)]


def host(r):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def rough(sc, seed):
    """the scene's exact maps made rough: noise of 0.4 px, a sixth of the entries thrown 8 to 20 px off, a few NaN and inf"""
    rng = np.random.default_rng(seed)
    corr = sc['corr'].astype(np.float64) + rng.normal(0.0, 0.4, sc['corr'].shape)
    off = rng.random(corr.shape[:3]) < 1 / 6
    ang, r = rng.uniform(0, 2 * np.pi, off.shape), rng.uniform(8.0, 20.0, off.shape)
    corr[..., 0] += np.where(off, r * np.cos(ang), 0.0)
    corr[..., 1] += np.where(off, r * np.sin(ang), 0.0)
    corr = corr.astype(np.float32)
    bad = rng.random(off.shape)
    corr[bad < 0.01, 0] = np.nan
    corr[(bad >= 0.01) & (bad < 0.02), 1] = np.inf
    return corr


def device_depth(sc, corr, valid=None, found=None, **kw):
    args = dict(threshold=2.0, min_angle=MIN_ANGLE)
    args.update(kw)
    return host(depth_from_corr(corr, sc['Ks'][0], sc['c2ws'][0], sc['Ks'][1:], sc['c2ws'][1:], valid=valid, found=found, **args))


def oracle_depth(sc, corr, valid=None, found=None, **kw):
    args = dict(threshold=2.0, max_cos=MAX_COS)
    args.update(kw)
    return mo.corr_depth(corr, valid, sc['cams'], sc['poses'], found=found, **args)


def same_depth(d, o, what):
    for k in ('depth', 'views', 'err', 'info'):
        assert d[k].dtype == o[k].dtype and d[k].shape == o[k].shape, (what, k)
        assert np.array_equal(d[k], o[k], equal_nan=True), (what, k, int((d[k] != o[k]).sum()))
    assert np.array_equal(d['mask'], o['depth'] > 0)


# ---- the depth call: every shape and option ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', DEPTH_CASES, ids=lambda c: f'{c[0][0]}x{c[0][1]}-K{c[1]}')
def test_depth_bit_for_bit(case):
    (H, W), K = case
    sc = mo.scene(H, W, K)
    rng = np.random.default_rng(K)
    corr = rough(sc, 100 + K)
    mask = rng.random((K, H, W)) < 0.8
    flagged = depths = 0
    for valid in (None, mask):
        for refine_iters in (0, 1, 10):
            for min_views in (1, 2):
                kw = dict(refine_iters=refine_iters, min_views=min_views)
                o = oracle_depth(sc, corr, valid, **kw)
                same_depth(device_depth(sc, corr, valid, **kw), o, (case, valid is not None, kw))
                flagged, depths = flagged + o['ambiguous'], depths + int(o['info'][1])
    o = oracle_depth(sc, sc['corr'], sc['vis'])
    d = device_depth(sc, sc['corr'], sc['vis'])
    same_depth(d, o, (case, 'exact maps'))
    assert np.array_equal(d['K'], sc['Ks'][0])
    print(f'{case}: {depths} depths over 12 option sets, {flagged} pixels near a decision, exact maps info {o["info"].tolist()}')


# ---- bad data -------------------------------------------------------------------------------------------------------------------------
def test_bad_data():
    sc = mo.scene(17, 23, 3)
    corr = sc['corr'].copy()
    base = oracle_depth(sc, corr)
    assert base['info'][1] > 100
    # every entry of one neighbour NaN or infinite: it takes no part
    for value in (np.nan, np.inf, -np.inf):
        c = corr.copy()
        c[1, ..., 0] = value
        o = oracle_depth(sc, c)
        same_depth(device_depth(sc, c), o, ('not finite', value))
        assert not (o['U'] >> 2 & 1).any() and o['info'][1] > 0
    # a neighbour in the reference's place looking the reference's way: parallel rays, no parallax, no candidate
    twin = dict(sc, Ks=sc['Ks'][[0, 0]], c2ws=sc['c2ws'][[0, 0]], cams=sc['cams'][[0, 0]], poses=sc['poses'][[0, 0]])
    ys, xs = np.mgrid[0:17, 0:23].astype(np.float32)
    same = np.stack([xs, ys], -1)[None]
    o = oracle_depth(twin, same)
    same_depth(device_depth(twin, same), o, 'parallel rays')
    assert o['info'].tolist() == [1, 0, 0, 17 * 23, 0, 0, 0, 0]
    # a neighbour turned about its own centre to look away: the points lie behind it
    away = sc['c2ws'].copy()
    away[2, :3, :3] = away[2, :3, :3] @ np.diag([-1.0, 1.0, -1.0])
    back = dict(sc, c2ws=away, poses=mo.w2c_rows(away))
    o = oracle_depth(back, corr)
    same_depth(device_depth(back, corr), o, 'behind a neighbour')
    assert not (o['U'] >> 2 & 1).any() and o['info'][1] > 0
    # a pose that is not finite: the view takes no part; the reference's: nothing comes out; found = 0 likewise
    for view in (2, 0):   # (through the C ABI: the wrapper refuses such a pose on the host)
        poses = sc['poses'].copy()
        poses[view, 7] = np.nan
        o = oracle_depth(dict(sc, poses=poses), corr)
        d = raw_depth(sc['cams'], poses, corr, None, None)
        same_depth(dict(d, mask=d['depth'] > 0), o, ('pose not finite', view))
        assert (o['info'][1] > 0) == (view != 0)
    cams = sc['cams'].copy()
    cams[0, 0] = 0.0
    d = raw_depth(cams, sc['poses'], corr, None, None)
    o = mo.corr_depth(corr, None, cams, sc['poses'], max_cos=MAX_COS)
    same_depth(dict(d, mask=d['depth'] > 0), o, 'a reference camera with focal length 0')
    assert not o['info'][1:].any() and np.isnan(d['err']).all()
    for found in (np.zeros(1, np.int32), torch.zeros(1, dtype=torch.int32, device='cuda'), np.ones(1, np.int32)):
        f = found.cpu().numpy() if torch.is_tensor(found) else found
        o = oracle_depth(sc, corr, found=f)
        same_depth(device_depth(sc, corr, found=found), o, ('found', int(f[0])))
        assert o['info'][0] == int(f[0]) and (o['info'][1] > 0) == bool(f[0])


# ---- the filter: every shape and option -------------------------------------------------------------------------------------------------
def filter_scene(H, W, n, seed=0):
    from cotr_amd.utils.synth import synth_scene
    caps = synth_scene(seed, n + 2, H, W)[:n]
    return dict(caps=caps, depths=np.stack([c.depth for c in caps]), Ks=np.stack([c.K for c in caps]), c2ws=np.stack([c.c2w for c in caps]))


def same_filter(d, o, what):
    for k in ('depth', 'count', 'info'):
        assert d[k].dtype == o[k].dtype and d[k].shape == o[k].shape, (what, k)
        assert np.array_equal(d[k], o[k]), (what, k, int((d[k] != o[k]).sum()))


@pytest.mark.parametrize('case', FILTER_CASES, ids=lambda c: f'{c[0][0]}x{c[0][1]}-n{c[1]}')
def test_filter_bit_for_bit(case):
    (H, W), n = case
    sc = filter_scene(H, W, n)
    rng = np.random.default_rng(n)
    depths = sc['depths'].copy()
    depths *= (1.0 + np.where(rng.random(depths.shape) < 0.3, rng.normal(0.0, 0.02, depths.shape), 0.0)).astype(np.float32)   # some off by percents
    depths[rng.random(depths.shape) < 0.01] = np.inf
    depths[rng.random(depths.shape) < 0.01] = np.nan
    depths[rng.random(depths.shape) < 0.01] = -1.0
    pairs = (rng.random((n, n)) < 0.7).astype(np.uint8)
    flagged = kept = 0
    for kw in (dict(), dict(min_views=1), dict(min_views=0, max_violations=0), dict(min_views=1, max_violations=1, px_thresh=0.5, rel_thresh=0.02),
               dict(pairs=pairs, min_views=1), dict(pairs=torch.from_numpy(pairs).cuda(), min_views=1, max_violations=0)):
        okw = dict(kw)
        if torch.is_tensor(okw.get('pairs')):
            okw['pairs'] = pairs
        o = mo.depth_consistency(depths, sc['Ks'], sc['c2ws'], **okw)
        same_filter(host(filter_depths(depths, sc['Ks'], sc['c2ws'], **kw)), o, (case, kw))
        flagged, kept = flagged + o['ambiguous'], kept + int(o['info'][:, 2].sum())
    o = mo.depth_consistency(sc['depths'], sc['Ks'], sc['c2ws'], min_views=1)
    same_filter(host(filter_depths(torch.from_numpy(sc['depths']).cuda(), sc['Ks'], torch.from_numpy(sc['c2ws']).cuda(), min_views=1)), o, (case, 'true depths'))
    print(f'{case}: {kept} pixels kept over 6 option sets, {flagged} near a decision, true depths info {o["info"][:3].tolist()}')


def test_filter_bad_data_and_found():
    sc = filter_scene(17, 23, 4)
    depths = sc['depths'].copy()
    depths[2] = 0.0                                           # an all-zero map
    o = mo.depth_consistency(depths, sc['Ks'], sc['c2ws'], min_views=1)
    same_filter(host(filter_depths(depths, sc['Ks'], sc['c2ws'], min_views=1)), o, 'an all-zero map')
    assert o['info'][2].tolist() == [1, 0, 0, 0] and o['info'][0, 2] > 0
    zero = np.zeros_like(depths)
    o = mo.depth_consistency(zero, sc['Ks'], sc['c2ws'], min_views=0)
    same_filter(host(filter_depths(zero, sc['Ks'], sc['c2ws'], min_views=0)), o, 'every map zero')
    assert not o['depth'].any() and not o['info'][:, 1:].any()
    c2ws = sc['c2ws'].copy()
    c2ws[1, 0, 3] = np.nan                                    # a pose that is not finite (the wrapper refuses it on the host: device tensor)
    o = mo.depth_consistency(sc['depths'], sc['Ks'], c2ws, min_views=1)
    same_filter(host(filter_depths(sc['depths'], sc['Ks'], torch.from_numpy(c2ws).cuda(), min_views=1)), o, 'a pose that is not finite')
    assert o['info'][1].tolist()[2:] == [0, 0] and not o['depth'][1].any() and o['info'][0, 2] > 0
    for found in ([1, 0, 1, 1], [0, 0, 0, 0], [0, 1, 1, 0]):
        f = np.array(found, np.int32)
        o = mo.depth_consistency(sc['depths'], sc['Ks'], sc['c2ws'], found=f, min_views=1)
        same_filter(host(filter_depths(sc['depths'], sc['Ks'], sc['c2ws'], found=f, min_views=1)), o, ('found', found))
        same_filter(host(filter_depths(sc['depths'], sc['Ks'], sc['c2ws'], found=torch.from_numpy(f).cuda(), min_views=1)), o, ('found on the device', found))
        assert o['info'][:, 0].tolist() == found


def test_filter_captures_with_min_overlap():
    from cotr_amd.scene import overlap_matrix
    sc = filter_scene(24, 32, 5)
    caps = sc['caps']
    dist = overlap_matrix(caps).cpu().numpy()
    cells = np.sort(dist[~np.eye(5, dtype=bool)])
    cut = float((cells[5] + cells[6]) / 2)
    pairs = (dist > np.float32(cut)).astype(np.uint8)
    assert 0 < pairs[~np.eye(5, dtype=bool)].sum() < 20
    out, r = filter_captures(caps, min_overlap=cut, min_views=1)
    o = mo.depth_consistency(sc['depths'], sc['Ks'], sc['c2ws'], pairs=pairs, min_views=1)
    same_filter(host(r), o, 'min_overlap')
    assert len(out) == 5 and all(torch.equal(c.depth, r['depth'][i]) and c.image is caps[i].image and c.K is caps[i].K for i, c in enumerate(out))
    out2, r2 = filter_captures(caps, pairs=pairs, min_views=1)
    assert torch.equal(r2['depth'], r['depth'])


# ---- the same bits, and nothing outside the outputs -----------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def raw_depth(cams, poses, corr, valid, found, stream=None, out=None, refine_iters=10, min_views=1):
    """cotr_corr_depth through the C ABI -> host dict; ``out``: the four output tensors to write"""
    lib = _lib.load_library()
    K, H, W = corr.shape[:3]
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None for x in (corr, valid, cams, poses, found)]
    if out is None:
        out = [torch.empty((H, W), dtype=torch.float32, device='cuda'), torch.empty((H, W), dtype=torch.uint8, device='cuda'),
               torch.empty((H, W), dtype=torch.float32, device='cuda'), torch.empty(8, dtype=torch.int32, device='cuda')]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    rc = lib.cotr_corr_depth(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), K + 1, H, W, _p(t[4]), 2.0, MAX_COS, 50.0, min_views, refine_iters, *[_p(x) for x in out], s)
    assert rc == 0, lib.cotr_raster_last_error()
    torch.cuda.synchronize()
    return dict(zip(('depth', 'views', 'err', 'info'), [x.cpu().numpy() for x in out]))


def test_same_bits_across_calls_streams_garbage_and_graph_replay():
    lib = _lib.load_library()
    sc = mo.scene(48, 64, 3)
    corr = rough(sc, 7)
    K, H, W = 3, 48, 64
    fs = filter_scene(48, 64, 4)
    n = 4
    want_d = oracle_depth(sc, corr, sc['vis'])
    want_f = mo.depth_consistency(fs['depths'], fs['Ks'], fs['c2ws'], min_views=1, max_violations=2)
    same_depth(device_depth(sc, corr, sc['vis']), want_d, 'first')
    same_depth(device_depth(sc, corr, sc['vis']), want_d, 'again')
    t = dict(corr=torch.from_numpy(corr).cuda(), valid=torch.from_numpy(sc['vis'].astype(np.uint8)).cuda(), cams=torch.from_numpy(sc['cams']).cuda(),
             poses=torch.from_numpy(sc['poses']).cuda(), depths=torch.from_numpy(fs['depths']).cuda(), c2w=torch.from_numpy(fs['c2ws']).cuda())
    Ks = (ctypes.c_double * (9 * n))(*fs['Ks'].reshape(-1))

    def buffers():
        f = lambda shape: torch.full(shape, -7.0, dtype=torch.float32, device='cuda')   # noqa: E731
        u = lambda shape: torch.full(shape, 0x5A, dtype=torch.uint8, device='cuda')     # noqa: E731
        i = lambda shape: torch.full(shape, -3, dtype=torch.int32, device='cuda')       # noqa: E731
        return dict(depth=f((H, W)), views=u((H, W)), err=f((H, W)), info=i((8,)), fdepth=f((n, H, W)), count=u((n, H, W)), finfo=i((n, 4)))

    def enqueue(b, stream):
        rc = lib.cotr_corr_depth(_p(t['corr']), _p(t['valid']), _p(t['cams']), _p(t['poses']), K + 1, H, W, None, 2.0, MAX_COS, 50.0, 1, 10, _p(b['depth']),
                                 _p(b['views']), _p(b['err']), _p(b['info']), stream)
        assert rc == 0, lib.cotr_raster_last_error()
        rc = lib.cotr_depth_consistency(_p(t['depths']), n, H, W, Ks, _p(t['c2w']), None, None, 1.0, 0.01, 1, 2, _p(b['fdepth']), _p(b['count']), _p(b['finfo']),
                                        stream)
        assert rc == 0, lib.cotr_raster_last_error()

    def same(b):
        for k, want in (('depth', want_d['depth']), ('views', want_d['views']), ('err', want_d['err']), ('info', want_d['info']), ('fdepth', want_f['depth']),
                        ('count', want_f['count']), ('finfo', want_f['info'])):
            assert np.array_equal(b[k].cpu().numpy(), want, equal_nan=True), k
    b = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    enqueue(b, ctypes.c_void_p(side.cuda_stream))
    side.synchronize()
    same(b)
    # captured once (a single linear chain on the capture stream), replayed once
    b = buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue(b, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    graph.replay()
    torch.cuda.synchronize()
    same(b)


@pytest.mark.parametrize('size', [(1, 1), (13, 20), (17, 23)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_guard_bands_around_every_output(size):
    """every output sits between bands of 0xA5 in one arena: the bands come back untouched and the outputs hold the restatement's bits"""
    lib = _lib.load_library()
    H, W = size
    K = n = 3
    sc, fs = mo.scene(H, W, K), filter_scene(H, W, n)
    corr = rough(sc, 3)
    BAND = 512
    sizes = dict(depth=H * W * 4, views=H * W, err=H * W * 4, info=32, fdepth=n * H * W * 4, count=n * H * W, finfo=n * 16)
    offsets, total = {}, BAND
    for k, nbytes in sizes.items():
        offsets[k] = total
        total += -(-nbytes // 256) * 256 + BAND
    arena = torch.full((total,), 0xA5, dtype=torch.uint8, device='cuda')
    at = lambda k: ctypes.c_void_p(arena.data_ptr() + offsets[k])   # noqa: E731
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (corr, sc['cams'], sc['poses'], fs['depths'], fs['c2ws'])]
    Ks = (ctypes.c_double * (9 * n))(*fs['Ks'].reshape(-1))
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.cotr_corr_depth(_p(t[0]), None, _p(t[1]), _p(t[2]), K + 1, H, W, None, 2.0, MAX_COS, 50.0, 1, 10, at('depth'), at('views'), at('err'), at('info'), s)
    assert rc == 0, lib.cotr_raster_last_error()
    rc = lib.cotr_depth_consistency(_p(t[3]), n, H, W, Ks, _p(t[4]), None, None, 1.0, 0.01, 1, -1, at('fdepth'), at('count'), at('finfo'), s)
    assert rc == 0, lib.cotr_raster_last_error()
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    outside = np.ones(total, bool)
    for k, nbytes in sizes.items():
        outside[offsets[k]:offsets[k] + nbytes] = False
    assert (got[outside] == 0xA5).all(), 'a byte outside the outputs was written'
    od = oracle_depth(sc, corr)
    of = mo.depth_consistency(fs['depths'], fs['Ks'], fs['c2ws'], min_views=1)
    for k, want in (('depth', od['depth']), ('views', od['views']), ('err', od['err']), ('info', od['info']), ('fdepth', of['depth']), ('count', of['count']),
                    ('finfo', of['info'])):
        assert np.array_equal(got[offsets[k]:offsets[k] + sizes[k]].view(want.dtype).reshape(want.shape), want, equal_nan=True), k


# ---- the chain into the volume ----------------------------------------------------------------------------------------------------
# |raycast - truth| of a volume of voxel 0.1 and trunc 0.3 fused from maps of 48 x 64: median, p90, largest
TSDF_MEDIAN, TSDF_P90, TSDF_MAX = 2.13e-3, 2.08e-2, 1.04e-1


def away_from_rims(truth, R, jump):
    """the pixels with a depth that have no pixel within R (Chebyshev) whose depth differs from theirs by more than ``jump``"""
    H, W = truth.shape
    out = truth > 0
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            sh = np.zeros_like(truth)
            ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H + min(0, -dy))
            xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W + min(0, -dx))
            sh[yd, xd] = truth[ys, xs]
            out &= ~((sh > 0) & (np.abs(sh - truth) > jump))
    return out


def test_chain_from_correspondences_to_a_raycast():
    """depth_from_corr on every view of a ``synth_scene`` -> filter_depths -> fuse_captures -> raycast_volume from the middle view's
    pose, held against the scene's true depth within the volume's own figures of DESIGN.md 3h-11 (voxel 0.1, trunc 0.3, maps of
    48 x 64: median 2.13e-3, p90 2.08e-2, largest 1.04e-1, about a voxel).  Those were measured on the three-plane corner, which has
    creases and no occluding rim; ``synth_scene`` has a near patch in front of the background, and a ray that grazes its rim ends on
    the other surface, metres off, whatever the depth maps are (the same volume fused from the TRUE maps: 39 pixels beyond a voxel,
    the largest 4.54).  So the three figures are asserted on the pixels farther from a rim than the truncation band reaches - R =
    ceil(trunc / the smallest pixel footprint) = 4 pixels, a rim being a depth step above 0.5 - and on all pixels the count beyond
    a voxel may not exceed that of the true-map volume.  Measured on an MI355X (and by the restatements on the host): 1356 pixels
    away from rims, median 2.06e-3, p90 5.12e-3, largest 1.10e-2; 23 pixels beyond a voxel against 39."""
    H, W, n = 48, 64, 5
    fs = filter_scene(H, W, n)
    caps = fs['caps']
    maps = []
    for i in range(n):
        others = [j for j in range(n) if j != i]
        both = [mo.reproject(caps[i].depth, caps[i].K, caps[i].c2w, caps[j].K, caps[j].c2w, caps[j].depth) for j in others]
        corr = np.stack([b[0] for b in both]).astype(np.float32)
        r = depth_from_corr(corr, caps[i].K, caps[i].c2w, fs['Ks'][others], fs['c2ws'][others], valid=np.stack([b[1] for b in both]))
        assert np.array_equal(r['K'], caps[i].K)
        maps.append(r['depth'])
    est = torch.stack(maps)
    has = (est > 0).cpu().numpy()
    rel = np.abs(est.cpu().numpy()[has].astype(np.float64) - fs['depths'][has]) / fs['depths'][has]
    assert has.sum() > 0.6 * has.size and rel.max() <= 4 * 3.6e-7
    kept = filter_depths(est, fs['Ks'], fs['c2ws'], min_views=1)
    assert int(kept['info'][:, 2].sum()) > 0.8 * has.sum()
    voxel, trunc = 0.1, 0.3
    make = lambda: TsdfVolume((-4.0, -3.2, 3.0), voxel, (80, 64, 64), trunc=trunc)   # noqa: E731
    vol, _ = fuse_captures([c._replace(depth=kept['depth'][i]) for i, c in enumerate(caps)], make())
    ref, _ = fuse_captures(caps, make())
    mid = n // 2
    ray = lambda v: raycast_volume(v, caps[mid].K, caps[mid].c2w, (H, W), near=0.5, far=12.0, step=trunc / 2)['depth'].cpu().numpy().astype(np.float64)   # noqa: E731
    got, own = ray(vol), ray(ref)
    truth = caps[mid].depth.astype(np.float64)
    hit = (got > 0) & (own > 0) & (truth > 0)
    R = int(np.ceil(trunc / (truth[truth > 0].min() / caps[mid].K[0, 0])))
    calm = hit & away_from_rims(truth, R, 0.5)
    e_got, e_own = np.abs(got - truth), np.abs(own - truth)
    beyond_got, beyond_own = int((e_got[hit] > voxel).sum()), int((e_own[hit] > voxel).sum())
    median, p90, largest = np.median(e_got[calm]), np.percentile(e_got[calm], 90), e_got[calm].max()
    print(f'raycast from view {mid}: {hit.sum()} pixels hit, {calm.sum()} farther than {R} px from a rim: |depth - truth| median {median:.2e} p90 {p90:.2e} '
          f'largest {largest:.2e} there (the true-map volume: {np.median(e_own[calm]):.2e} / {np.percentile(e_own[calm], 90):.2e} / {e_own[calm].max():.2e}); '
          f'beyond a voxel on all hit pixels: {beyond_got} against {beyond_own} of the true-map volume')
    assert R == 4 and hit.sum() > 0.5 * H * W and calm.sum() > 0.4 * H * W
    assert median <= TSDF_MEDIAN and p90 <= TSDF_P90 and largest <= TSDF_MAX
    assert beyond_got <= beyond_own


# ---- the engine ---------------------------------------------------------------------------------------------------------------------
def test_engine_depth_map_and_fuse_images_equal_the_free_functions():
    import cotr_amd
    from cotr_amd.models import build_model
    from cotr_amd.utils.synth import synth_state_dict
    hip = build_model(cotr_amd.default_args()).cuda().eval()
    hip.load_state_dict(synth_state_dict(0))
    eng = ZoomEngine(hip)
    fs = filter_scene(64, 64, 3)
    imgs = [c.image for c in fs['caps']]
    with torch.no_grad():
        r = eng.depth_map(imgs[1], [imgs[0], imgs[2]], fs['Ks'][1], fs['Ks'][[0, 2]], fs['c2ws'][1], fs['c2ws'][[0, 2]], max_cycle=10.0, threshold=4.0)
        maps = []
        for img in (imgs[0], imgs[2]):
            corr, con = eng.flow(imgs[1], img, resample=False)[:2]
            maps.append(flow_to_corr(corr, con, img.shape, 10.0))
    corr, valid = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    assert np.array_equal(r['corr'].cpu().numpy(), corr) and np.array_equal(r['valid'].cpu().numpy(), valid) and valid.any()
    want = depth_from_corr(corr, fs['Ks'][1], fs['c2ws'][1], fs['Ks'][[0, 2]], fs['c2ws'][[0, 2]], valid=valid, threshold=4.0)
    for k in ('depth', 'views', 'err', 'mask', 'info'):
        assert np.array_equal(r[k].cpu().numpy(), want[k].cpu().numpy(), equal_nan=True), k
    assert np.array_equal(r['K'], fs['Ks'][1])
    o = mo.corr_depth(corr, valid, mo.cam_rows(fs['Ks'][[1, 0, 2]]), mo.w2c_rows(fs['c2ws'][[1, 0, 2]]), threshold=4.0, max_cos=MAX_COS)
    assert np.array_equal(r['info'].cpu().numpy(), o['info'])
    make = lambda: TsdfVolume((-4.0, -3.2, 3.0), 0.2, (40, 32, 32), trunc=0.6, color=True)   # noqa: E731
    with torch.no_grad():
        vol, depths, info = eng.fuse_images(imgs, fs['Ks'], fs['c2ws'], make(), neighbours=2, filter_kw=dict(min_views=1), max_cycle=10.0, threshold=4.0)
        centres = fs['c2ws'][:, :3, 3]
        single = []
        for i in range(3):   # the two nearest cameras, the nearer first
            d = np.linalg.norm(centres - centres[i], axis=1)
            d[i] = np.inf
            near = [int(j) for j in np.argsort(d, kind='stable')[:2]]
            single.append(eng.depth_map(imgs[i], [imgs[j] for j in near], fs['Ks'][i], fs['Ks'][near], fs['c2ws'][i], fs['c2ws'][near], max_cycle=10.0,
                                        threshold=4.0))
    kept = filter_depths(torch.stack([s['depth'] for s in single]), fs['Ks'], fs['c2ws'], min_views=1)
    assert torch.equal(depths, kept['depth']) and torch.equal(info['filter'], kept['info'])
    assert all(torch.equal(a, s['info']) for a, s in zip(info['depth'], single))
    ref, fused = fuse_captures([Capture(imgs[i], kept['depth'][i], fs['Ks'][i], fs['c2ws'][i]) for i in range(3)], make())
    assert torch.equal(vol.tsdf, ref.tsdf) and torch.equal(vol.weight, ref.weight) and torch.equal(vol.color, ref.color) and info['fused'] == fused


def test_engine_depth_map_sparse(monkeypatch):
    from cotr_amd.inference import triangulate_corr
    sc = mo.scene(48, 64, 2)
    caps = sc['caps']
    rng = np.random.default_rng(5)
    sparse = []
    for k in range(2):
        xs, ys = rng.uniform(1, 62, 300), rng.uniform(1, 46, 300)
        iy, ix = np.rint(ys - 0.5).astype(int), np.rint(xs - 0.5).astype(int)
        ok = caps[0].depth[iy, ix] > 0
        # the scene's map at the pixel whose centre the query sits nearest; exact enough for an equality test of two code paths
        sparse.append(np.concatenate([np.stack([xs, ys], 1), sc['corr64'][k][iy, ix] + 0.5], axis=1)[ok])
    calls = iter(sparse)
    eng = ZoomEngine.__new__(ZoomEngine)
    eng.model = torch.nn.Linear(1, 1).cuda()
    monkeypatch.setattr(ZoomEngine, 'cotr_corr_multiscale', lambda self, a, b, *args, **kw: next(calls))
    imgs = [c.image for c in caps]
    r = eng.depth_map(imgs[0], imgs[1:], sc['Ks'][0], sc['Ks'][1:], sc['c2ws'][0], sc['c2ws'][1:], dense='sparse', threshold=4.0)
    dense = [triangulate_corr(s, imgs[0].shape, imgs[k + 1].shape, simplices='device', return_mask=True, as_tensor=True) for k, s in enumerate(sparse)]
    corr, valid = torch.stack([d[0].float() for d in dense]), torch.stack([d[1] for d in dense])
    assert torch.equal(r['corr'], corr) and torch.equal(r['valid'], valid) and valid.any()
    want = depth_from_corr(corr, sc['Ks'][0], sc['c2ws'][0], sc['Ks'][1:], sc['c2ws'][1:], valid=valid, centres=0.5, threshold=4.0)
    for k in ('depth', 'views', 'err', 'mask', 'info'):
        assert torch.equal(r[k], want[k]) or (k == 'err' and np.array_equal(r[k].cpu().numpy(), want[k].cpu().numpy(), equal_nan=True)), k
    K05 = sc['Ks'][0].copy()
    K05[:2, 2] -= 0.5
    assert np.array_equal(r['K'], K05) and int(r['info'][1]) > 0
