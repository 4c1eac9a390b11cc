"""cotr_photo_depth on the device against the numpy restatement tests/photodepth_oracle.py: every output bit for
bit on every pixel the restatement does not call ambiguous, at every listed shape and every value of every option; bad data; the
same bits across calls, streams, pre-filled outputs and a graph replay; 0xA5 bands around every output; the quality of the
refined depth on a noisy scene; ``to_grey``; the engine's ``depth_map(photo_sweeps=...)``."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.data import Capture
from cotr_amd.inference import ZoomEngine, depth_from_corr, refine_captures_photo, refine_depth_photo, to_grey
from tests import mvdepth_oracle as mo
from tests import photodepth_oracle as po

pytestmark = pytest.mark.gpu

# (H, W), K, radius, steps, sweeps, min_views (0: K): every listed shape, and every value of K in {1, 2, 5, 31}, radius in {1, 2, 4},
# steps in {1, 4, 16}, sweeps in {1, 3, 8} and min_views in {1, K}
CASES = [((1, 1), 1, 1, 1, 1, 1),        # nothing but rim
         ((3, 3), 1, 1, 4, 3, 1),        # only the centre is off the rim
         ((7, 9), 2, 2, 1, 8, 0),        # smaller than a tile
         ((17, 23), 5, 1, 16, 1, 1),     # across tile edges in both directions
         ((33, 20), 2, 4, 4, 3, 1),
         ((17, 23), 31, 2, 1, 1, 1),
         ((33, 20), 5, 2, 4, 3, 0)]
SEEDS = {(1, 1): 0, (3, 3): 0, (7, 9): 2, (17, 23): 0, (33, 20): 0}   # chosen on the host: the restatement alone stays within AMBIGUOUS
AMBIGUOUS = 0.01   # the share of a case's pixels the restatement may call ambiguous


def host(r):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def start_depth(sc, seed=0):
    """the truth times a smooth perturbation of about 1 %"""
    return po.perturbed(sc['depth'], 0.01, seed)


def device_photo(sc, depth, found=None, **kw):
    return host(refine_depth_photo(depth, sc['grey'][0], sc['grey'][1:], sc['Ks'][0], sc['c2ws'][0], sc['Ks'][1:], sc['c2ws'][1:], found=found, **kw))


def oracle_photo(sc, depth, found=None, **kw):
    return po.photo_depth(sc['grey'], depth, sc['cams'], sc['poses'], found=found, **kw)


def same_photo(d, o, what):
    """every output on every pixel the restatement does not call ambiguous; info when there is none"""
    sure = ~o['amb']
    for k in ('depth', 'score', 'views'):
        assert d[k].dtype == o[k].dtype and d[k].shape == o[k].shape, (what, k)
        assert np.array_equal(d[k][sure], o[k][sure], equal_nan=True), (what, k, int((d[k][sure] != o[k][sure]).sum()))
    assert d['info'].dtype == o['info'].dtype and d['info'][0] == o['info'][0] and d['info'][1:].sum() == o['info'][1:].sum(), what
    if o['ambiguous'] == 0:
        assert np.array_equal(d['info'], o['info']), (what, d['info'].tolist(), o['info'].tolist())
    if 'mask' in d:
        assert np.array_equal(d['mask'], d['views'] > 0)


# ---- every shape and option -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=lambda c: f'{c[0][0]}x{c[0][1]}-K{c[1]}-R{c[2]}-S{c[3]}-sweeps{c[4]}-views{c[5] or "K"}')
def test_photo_bit_for_bit(case):
    (H, W), K, R, S, sweeps, min_views = case
    sc = po.scene(H, W, K, SEEDS[(H, W)])
    depth = start_depth(sc) if (H, W) != (1, 1) else np.full((1, 1), 5.0, np.float32)   # (the scene's only pixel is a hole)
    flagged = 0
    for keep in (True, False):
        # min_score 0: at these sizes the images are coarse, and a score of 0.5 would leave the smallest cases without a refined pixel
        kw = dict(radius=R, steps=S, sweeps=sweeps, min_views=min_views or K, keep_input=keep, rel_step=0.004 if S < 16 else 0.001, min_score=0.0)
        o = oracle_photo(sc, depth, **kw)
        assert o['ambiguous'] <= AMBIGUOUS * H * W, (case, o['ambiguous'])
        same_photo(device_photo(sc, depth, **kw), o, (case, keep))
        flagged += o['ambiguous']
    print(f'{case}: info {o["info"].tolist()}, {flagged} pixels near a decision over both values of keep_input')
    if (H, W) == (1, 1):
        assert o['info'].tolist() == [1, 0, 0, 1, 0, 0, 0, 0]
    if (H, W) == (3, 3):
        assert o['info'][2] + o['info'][3] == 8 and o['what'][1, 1] == 0
    if H > 3:
        assert o['info'][1] > 0


# ---- bad data -------------------------------------------------------------------------------------------------------------------------
def raw_photo(grey, depth, cams, poses, found=None, stream=None, out=None, radius=2, steps=4, sweeps=3, rel_step=0.004, min_var=4.0, min_score=0.5,
              min_views=1, dist=50.0, keep=1):
    """cotr_photo_depth through the C ABI -> host dict; ``out``: the four output tensors to write"""
    lib = _lib.load_library()
    V, H, W = grey.shape
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None for x in (grey, depth, cams, poses, found)]
    if out is None:
        out = [torch.empty((H, W), dtype=torch.float32, device='cuda'), torch.empty((H, W), dtype=torch.float32, device='cuda'),
               torch.empty((H, W), dtype=torch.uint8, device='cuda'), torch.empty(8, dtype=torch.int32, device='cuda')]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    rc = lib.cotr_photo_depth(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), V, H, W, _p(t[4]), radius, steps, sweeps, rel_step, min_var, min_score, min_views, dist, keep,
                              *[_p(x) for x in out], s)
    assert rc == 0, lib.cotr_raster_last_error()
    torch.cuda.synchronize()
    return dict(zip(('depth', 'score', 'views', 'info'), [x.cpu().numpy() for x in out]))


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def test_bad_data():
    sc = po.scene(17, 23, 3)
    H, W = 17, 23
    depth = start_depth(sc)
    base = oracle_photo(sc, depth)
    assert base['info'][1] > 100 and base['ambiguous'] <= AMBIGUOUS * H * W
    # depths that are NaN, infinite, negative or 0: counted, and empty whatever keep_input says
    bad = depth.copy()
    bad[4, 4:8], bad[5, 4:8], bad[6, 4:8], bad[7, 4:8] = np.nan, -1.5, 0.0, np.inf
    for keep in (True, False):
        o = oracle_photo(sc, bad, keep_input=keep)
        same_photo(device_photo(sc, bad, keep_input=keep), o, ('bad depths', keep))
        assert (o['what'][4:8, 4:8] == 1).all() and not o['depth'][4:8, 4:8].any() and o['info'][2] >= 16
    # a pose that is not finite: the view takes no part; the reference's: nothing comes out (through the C ABI: the wrapper refuses such a pose)
    for view in (2, 0):
        poses = sc['poses'].copy()
        poses[view, 7] = np.nan
        o = po.photo_depth(sc['grey'], depth, sc['cams'], poses)
        same_photo(raw_photo(sc['grey'], depth, sc['cams'], poses), o, ('pose not finite', view))
        assert (o['info'][1] > 0) == (view != 0)
        if view == 0:
            assert o['info'].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and np.isnan(o['score']).all() and not o['depth'].any()
    cams = sc['cams'].copy()
    cams[2, 0] = 0.0
    o = po.photo_depth(sc['grey'], depth, cams, sc['poses'])
    same_photo(raw_photo(sc['grey'], depth, cams, sc['poses']), o, 'a neighbour camera with focal length 0')
    two = po.photo_depth(sc['grey'][[0, 1, 3]], depth, sc['cams'][[0, 1, 3]], sc['poses'][[0, 1, 3]])
    assert np.array_equal(o['depth'], two['depth']) and np.array_equal(o['info'], two['info'])
    # a neighbour turned about its own centre to look away: the points lie behind it
    away = sc['c2ws'].copy()
    away[2, :3, :3] = away[2, :3, :3] @ np.diag([-1.0, 1.0, -1.0])
    back = dict(sc, c2ws=away, poses=mo.w2c_rows(away))
    o = oracle_photo(back, depth)
    same_photo(device_photo(back, depth), o, 'behind a neighbour')
    assert np.array_equal(o['depth'], two['depth']) and np.array_equal(o['views'], two['views'])
    # every neighbour behind: nothing scores
    both = sc['c2ws'].copy()
    for j in (1, 2, 3):
        both[j, :3, :3] = both[j, :3, :3] @ np.diag([-1.0, 1.0, -1.0])
    o = oracle_photo(dict(sc, c2ws=both, poses=mo.w2c_rows(both)), depth)
    same_photo(device_photo(dict(sc, c2ws=both), depth), o, 'behind every neighbour')
    assert o['info'][1] == 0 and o['info'][5] == base['info'][1] + base['info'][5] + base['info'][6] + base['info'][7]
    for found in (np.zeros(1, np.int32), torch.zeros(1, dtype=torch.int32, device='cuda'), np.ones(1, np.int32)):
        f = found.cpu().numpy() if torch.is_tensor(found) else found
        o = oracle_photo(sc, depth, found=f)
        same_photo(device_photo(sc, depth, found=found), o, ('found', int(f[0])))
        assert o['info'][0] == int(f[0]) and (o['info'][1] > 0) == bool(f[0])
    # a constant image: every pixel off the rim is flat
    flat = dict(sc, grey=np.full_like(sc['grey'], 93))
    o = oracle_photo(flat, depth)
    same_photo(device_photo(flat, depth), o, 'constant images')
    assert o['info'][1] == 0 and o['info'][4] > 0 and o['info'][2] + o['info'][3] + o['info'][4] == H * W
    # a constant neighbour beside a textured one: it never scores
    one = sc['grey'].copy()
    one[2] = 200
    o = po.photo_depth(one, depth, sc['cams'], sc['poses'])
    same_photo(raw_photo(one, depth, sc['cams'], sc['poses']), o, 'a constant neighbour')
    assert np.array_equal(o['depth'], two['depth'])


# ---- the same bits, and nothing outside the outputs -----------------------------------------------------------------------------------
def test_same_bits_across_calls_streams_garbage_and_graph_replay():
    lib = _lib.load_library()
    H, W, K = 33, 40, 3
    sc = po.scene(H, W, K)
    depth = start_depth(sc)
    want = oracle_photo(sc, depth)
    first = device_photo(sc, depth)
    same_photo(first, want, 'first')
    again = device_photo(sc, depth)
    for k in ('depth', 'score', 'views', 'info'):
        assert np.array_equal(first[k], again[k], equal_nan=True), k
    t = dict(grey=torch.from_numpy(sc['grey']).cuda(), depth=torch.from_numpy(depth).cuda(), cams=torch.from_numpy(sc['cams']).cuda(),
             poses=torch.from_numpy(sc['poses']).cuda())

    def buffers():
        return dict(depth=torch.full((H, W), -7.0, dtype=torch.float32, device='cuda'), score=torch.full((H, W), -7.0, dtype=torch.float32, device='cuda'),
                    views=torch.full((H, W), 0x5A, dtype=torch.uint8, device='cuda'), info=torch.full((8,), -3, dtype=torch.int32, device='cuda'))

    def enqueue(b, stream):
        rc = lib.cotr_photo_depth(_p(t['grey']), _p(t['depth']), _p(t['cams']), _p(t['poses']), K + 1, H, W, None, 2, 4, 3, 0.004, 4.0, 0.5, 1, 50.0, 1,
                                  _p(b['depth']), _p(b['score']), _p(b['views']), _p(b['info']), stream)
        assert rc == 0, lib.cotr_raster_last_error()

    def same(b):
        for k in ('depth', 'score', 'views', 'info'):
            assert np.array_equal(b[k].cpu().numpy(), first[k], equal_nan=True), k
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
    K = 3
    sc = po.scene(H, W, K)
    depth = start_depth(sc)
    BAND = 512
    sizes = dict(depth=H * W * 4, score=H * W * 4, views=H * W, info=32)
    offsets, total = {}, BAND
    for k, nbytes in sizes.items():
        offsets[k] = total
        total += -(-nbytes // 256) * 256 + BAND
    arena = torch.full((total,), 0xA5, dtype=torch.uint8, device='cuda')
    at = lambda k: ctypes.c_void_p(arena.data_ptr() + offsets[k])   # noqa: E731
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (sc['grey'], depth, sc['cams'], sc['poses'])]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.cotr_photo_depth(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), K + 1, H, W, None, 2, 4, 3, 0.004, 4.0, 0.5, 1, 50.0, 1, at('depth'), at('score'), at('views'),
                              at('info'), s)
    assert rc == 0, lib.cotr_raster_last_error()
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    outside = np.ones(total, bool)
    for k, nbytes in sizes.items():
        outside[offsets[k]:offsets[k] + nbytes] = False
    assert (got[outside] == 0xA5).all(), 'a byte outside the outputs was written'
    o = oracle_photo(sc, depth)
    assert o['ambiguous'] <= AMBIGUOUS * H * W
    same_photo({k: got[offsets[k]:offsets[k] + sizes[k]].view(o[k].dtype).reshape(o[k].shape) for k in sizes}, o, size)


# ---- quality --------------------------------------------------------------------------------------------------------------------------
# the restatement on the host at 48 x 64, K = 4, radius 4, on the refined pixels more than radius + 2 pixels from a
# depth step: median |depth - truth| / truth 7.00e-3 before and QUALITY_AFTER after; the bound is twice that, which leaves room for
# another seed, not for a broken kernel
QUALITY_AFTER = 3.67e-3
QUALITY_BOUND = 2 * QUALITY_AFTER


def away_from_steps(truth, R, jump):
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


def quality_input(sc):
    """the truth times 1 + 0.01 cos(a slow phase over the map): about 1 %"""
    H, W = sc['depth'].shape
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    return (sc['depth'].astype(np.float64) * (1.0 + 0.01 * np.cos(2 * np.pi * (xs / W * 1.3 + ys / H * 0.9) + 0.5))).astype(np.float32)


def test_quality_on_a_noisy_scene():
    """48 x 64, K = 4, images with noise of 8 levels a channel and disparities of 7 to 14 pixels, so that 1 % of depth is a tenth of a
    pixel: the patch is the widest (radius 4, 81 taps to average the noise over)"""
    H, W, K, R = 48, 64, 4, 4
    sc = po.scene(H, W, K)
    truth = sc['depth'].astype(np.float64)
    start = quality_input(sc)
    d = device_photo(sc, start, radius=R)
    calm = d['mask'] & away_from_steps(truth, R + 2, 0.5)
    before = np.median(np.abs(start[calm].astype(np.float64) - truth[calm]) / truth[calm])
    after = np.median(np.abs(d['depth'][calm].astype(np.float64) - truth[calm]) / truth[calm])
    print(f'{calm.sum()} refined pixels more than {R + 2} px from a depth step: median relative error {before:.3e} before, {after:.3e} after (bound {QUALITY_BOUND:.3e})')
    assert calm.sum() > 0.25 * H * W
    assert after < before
    assert after <= QUALITY_BOUND


# ---- the wrappers and the engine --------------------------------------------------------------------------------------------------------
def test_to_grey_and_colour_images():
    sc = po.scene(24, 32, 2)
    rgb = np.stack([c.image for c in sc['caps']])
    for images in (rgb, torch.from_numpy(rgb).cuda(), rgb[0], rgb[:, :, :, 0]):
        g = to_grey(images)
        arr = images.cpu().numpy() if torch.is_tensor(images) else images
        assert g.is_cuda and g.dtype == torch.uint8
        assert np.array_equal(g.cpu().numpy(), po.grey_of(arr) if arr.shape[-1] == 3 else arr)
    depth = start_depth(sc)
    want = device_photo(sc, depth)
    got = host(refine_depth_photo(torch.from_numpy(depth).cuda(), rgb[0], [torch.from_numpy(rgb[1]).cuda(), sc['grey'][2]], sc['Ks'][0], sc['c2ws'][0],
                                  sc['Ks'][1:], sc['c2ws'][1:]))
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    caps = [Capture(c.image, depth if i == 0 else c.depth, c.K, c.c2w) for i, c in enumerate(sc['caps'])]
    out, results = refine_captures_photo(caps, neighbours=2)
    assert len(out) == len(results) == 3 and all(torch.equal(c.depth, r['depth']) and c.image is caps[i].image for i, (c, r) in enumerate(zip(out, results)))
    # capture 0 is the middle of the arc: its two nearest are the other two, the nearer first
    dist = [np.linalg.norm(sc['c2ws'][j][:3, 3] - sc['c2ws'][0][:3, 3]) for j in (1, 2)]
    order = [1, 2] if dist[0] <= dist[1] else [2, 1]
    ref = po.photo_depth(sc['grey'][[0] + order], depth, sc['cams'][[0] + order], sc['poses'][[0] + order])
    same_photo(host(results[0]), ref, 'refine_captures_photo')


def test_engine_depth_map_with_photo_sweeps(monkeypatch):
    from cotr_amd.inference import depth as depth_module
    H, W, K = 48, 64, 2
    sc = mo.scene(H, W, K)
    imgs = [c.image for c in sc['caps']]
    # flow's answer: the exact maps in its own convention (x, y in [-1, 1] over image B), a cycle error of 0 where B sees the pixel
    norm = [np.stack([(2.0 * m[..., 0] + 1.0) / W - 1.0, (2.0 * m[..., 1] + 1.0) / H - 1.0], -1).astype(np.float32) for m in sc['corr64']]
    con = [np.where(v, 0.0, 100.0).astype(np.float32) for v in sc['vis']]
    eng = ZoomEngine.__new__(ZoomEngine)
    eng.model = torch.nn.Linear(1, 1).cuda()
    calls = []
    enqueue = depth_module._enqueue_photo_depth
    monkeypatch.setattr(depth_module, '_enqueue_photo_depth', lambda *a, **kw: calls.append(1) or enqueue(*a, **kw))

    def run(**kw):
        answers = iter(zip(norm, con))
        monkeypatch.setattr(ZoomEngine, 'flow', lambda self, a, b, resample=True: next(answers))
        return eng.depth_map(imgs[0], imgs[1:], sc['Ks'][0], sc['Ks'][1:], sc['c2ws'][0], sc['c2ws'][1:], threshold=4.0, **kw)
    plain = run()
    assert not calls and 'photo' not in plain and 'depth_corr' not in plain
    want = depth_from_corr(plain['corr'], sc['Ks'][0], sc['c2ws'][0], sc['Ks'][1:], sc['c2ws'][1:], valid=plain['valid'], threshold=4.0)
    assert torch.equal(plain['depth'], want['depth']) and int(want['info'][1]) > 0.5 * H * W
    r = run(photo_sweeps=2, photo_kw=dict(radius=3, min_score=0.6))
    assert len(calls) == 1 and torch.equal(r['depth_corr'], want['depth'])
    photo = refine_depth_photo(want['depth'], imgs[0], imgs[1:], want['K'], sc['c2ws'][0], sc['Ks'][1:], sc['c2ws'][1:], sweeps=2, radius=3, min_score=0.6)
    assert len(calls) == 2
    for k in ('depth', 'score', 'views', 'mask', 'info'):
        assert np.array_equal(r['photo'][k].cpu().numpy(), photo[k].cpu().numpy(), equal_nan=True), k
    assert torch.equal(r['depth'], photo['depth']) and torch.equal(r['mask'], photo['mask']) and int(photo['info'][1]) > 0
    for k in ('views', 'err', 'corr', 'valid'):
        assert np.array_equal(r[k].cpu().numpy(), plain[k].cpu().numpy(), equal_nan=True), k
    o = po.photo_depth(po.grey_of(np.stack(imgs)), want['depth'].cpu().numpy(), sc['cams'], sc['poses'], sweeps=2, radius=3, min_score=0.6)
    same_photo(host(photo), o, 'the engine against the restatement')
