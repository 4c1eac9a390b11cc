"""The rule of cotr_photo_depth on its numpy restatement tests/photodepth_oracle.py, which the GPU tests hold
the device against bit for bit: the truth as a fixed point and a perturbed depth drawn to it on noise-free images, the tie order
and the sub-step of a sweep's winner, rim, flat and range handling, keep_input both ways; then every argument error of the entry
point and of the wrappers, and ``to_grey``'s integer rule, without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.build import declared_symbols
from cotr_amd.inference import refine_captures_photo, refine_depth_photo, to_grey
from tests import photodepth_oracle as po

REL_STEP, SWEEPS = 0.004, 3
LAST_STEP = REL_STEP / 2 ** (SWEEPS - 1)   # the spacing of the last sweep's hypotheses, relative


def plane():
    return po.plane_scene(32, 48, 2)


def run(sc, depth, **kw):
    return po.photo_depth(sc['grey'], depth, sc['cams'], sc['poses'], **kw)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_truth_is_a_fixed_point_on_noise_free_images():
    """a fronto-parallel textured plane without noise: from the true depth every refined pixel ends within one step of the last
    sweep of it (what is left is the bilinear sampling of a texture of 7 pixels' period, rounded to 8 bits)"""
    sc = plane()
    o = run(sc, sc['depth'])
    ref = o['what'] == 0
    rel = np.abs(o['depth'][ref].astype(np.float64) / 6.0 - 1.0)
    print(f'info {o["info"].tolist()}: from the truth, relative error median {np.median(rel):.2e} largest {rel.max():.2e} (one last step: {LAST_STEP:.1e})')
    assert ref.sum() > 1000 and o['info'][1] == ref.sum()
    assert rel.max() < LAST_STEP
    assert (o['score'][ref] > 0.99).all() and (o['views'][ref] >= 1).all()


@pytest.mark.parametrize('amount', [0.01, -0.008])
def test_a_perturbed_depth_moves_toward_the_truth(amount):
    sc = plane()
    start = (sc['depth'].astype(np.float64) * (1.0 + amount)).astype(np.float32)
    o = run(sc, start)
    ref = o['what'] == 0
    rel = np.abs(o['depth'][ref].astype(np.float64) / 6.0 - 1.0)
    print(f'from {amount:+.3f}: {ref.sum()} refined, relative error median {np.median(rel):.2e} largest {rel.max():.2e}')
    assert ref.sum() > 1000
    assert rel.max() < LAST_STEP < abs(amount)          # every refined pixel ends nearer the truth than it started
    one = run(sc, start, sweeps=1)                      # and one sweep alone already moves every one of them the right way
    moved = (one['centre'][ref] - start[ref].astype(np.float64)) * np.sign(amount)
    assert (moved < 0).all()


def test_more_sweeps_reach_farther():
    """the reach of the sweeps is steps * rel_step * (2 - 2^(1 - sweeps)): a start 2.5 % off is within reach of three sweeps of four steps of 0.4 %
    (2.8 %), not of one (1.6 %)"""
    sc = plane()
    start = (sc['depth'].astype(np.float64) * 1.025).astype(np.float32)
    one, three = run(sc, start, sweeps=1), run(sc, start, sweeps=3)
    ref = (one['what'] == 0) & (three['what'] == 0)
    e1 = np.abs(one['depth'][ref].astype(np.float64) / 6.0 - 1.0)
    e3 = np.abs(three['depth'][ref].astype(np.float64) / 6.0 - 1.0)
    assert ref.sum() > 500 and np.median(e1) > 0.008 and np.median(e3) < LAST_STEP


def test_winner_tie_order():
    nan = np.nan
    F = np.array([[0.5, 0.9, 0.9, 0.2, nan, 0.7],     # k = -2
                  [0.9, 0.1, 0.3, 0.9, nan, nan],     # k = -1
                  [0.9, 0.2, 0.3, 0.1, nan, nan],     # k = 0
                  [0.9, 0.9, 0.3, 0.9, nan, nan],     # k = 1
                  [0.9, 0.9, 0.9, 0.2, nan, 0.7]])    # k = 2
    have, k, f, d, near = po.winner(F, 2)
    assert have.tolist() == [True, True, True, True, False, True]
    # equal f: the smallest |k|; then the negative one
    assert k[[0, 1, 2, 3, 5]].tolist() == [0, 1, -2, -1, -2]
    assert f[[0, 1, 2, 3, 5]].tolist() == [0.9, 0.9, 0.9, 0.9, 0.7] and np.isnan(f[4])
    assert near[[0, 1, 2, 3, 5]].all() and not near[4]          # every one of these is a tie
    assert (d[[2, 5]] == 0).all()                               # |k*| = S: no sub-step


def test_winner_sub_step():
    nan = np.nan
    F = np.array([[0.1, 0.1, 0.1, 0.81, 0.1, 0.5],    # k = -1
                  [0.8, 0.8, 0.8, 0.80, 0.8, 0.5],    # k = 0
                  [0.6, 0.2, nan, 0.79, 0.8, 0.5]])   # k = 1
    F = np.concatenate([np.full((1, 6), nan), F, np.full((1, 6), nan)])    # S = 2 with the outer hypotheses missing
    F[0, 4] = F[4, 4] = 0.0
    have, k, f, d, near = po.winner(F, 2)
    assert have.all() and k.tolist() == [0, 0, 0, -1, 0, 0]
    # the vertex of the parabola through (-1, f-), (0, f0), (1, f+): 0.5 (f- - f+) / (f- - 2 f0 + f+)
    assert d[0] == 0.5 * (0.1 - 0.6) / ((0.1 - 2.0 * 0.8) + 0.6) and 0 < d[0] < 0.5
    assert d[1] == 0.5 * (0.1 - 0.2) / ((0.1 - 2.0 * 0.8) + 0.2) and 0 < d[1] < d[0]
    assert d[2] == 0                       # f+ does not exist
    assert d[3] == 0                       # k* = -1 with f(-2) missing
    assert d[4] == 0.5                     # f0 = f+ > f-: the vertex lies half a step up, the clip's bound
    assert d[5] == 0 and near[5]           # den = 0: flat, no sub-step
    # a vertex beyond half a step is clipped (f+ > f0 cannot win, so only rounding can carry it there): by hand
    F2 = np.array([[nan], [0.0], [1.0], [1.0 - 1e-17], [nan]])
    assert po.winner(F2, 2)[3][0] == 0.5


def test_rim_flat_range_and_keep_input():
    sc = plane()
    H, W = sc['depth'].shape
    grey = sc['grey'].copy()
    grey[0, 8:20, 8:24] = 128                     # a patch of the reference without texture
    depth = sc['depth'].copy()
    depth[5, 5], depth[6, 6], depth[7, 7], depth[8, 30] = 0.0, np.nan, -2.0, np.inf
    R = 2
    for keep in (True, False):
        o = po.photo_depth(grey, depth, sc['cams'], sc['poses'], radius=R, keep_input=keep)
        w = o['what']
        assert (w[[5, 6, 7, 8], [5, 6, 7, 30]] == 1).all() and o['info'][2] == 4
        rim = np.ones((H, W), bool)
        rim[R:H - R, R:W - R] = False
        assert ((w == 2) == (rim & (w != 1))).all() and o['info'][3] == rim.sum()
        assert (w[8 + R:20 - R, 8 + R:24 - R] == 3).all() and o['info'][4] == (w == 3).sum() >= (12 - 2 * R) * (16 - 2 * R)
        assert o['info'][1:].sum() == H * W and o['info'][0] == 1
        unrefined = w != 0
        assert np.isnan(o['score'][unrefined]).all() and (o['views'][unrefined] == 0).all()
        assert not np.isnan(o['score'][~unrefined]).any() and (o['views'][~unrefined] > 0).all()
        held = unrefined & (w != 1)
        assert (o['depth'][w == 1] == 0).all()
        assert np.array_equal(o['depth'][held], depth[held] if keep else np.zeros(held.sum(), np.float32))
        assert (o['depth'][~unrefined] > 0).all()
    # the range: a threshold below the plane drops every pixel that would have been refined; they hold their input or 0
    full = po.photo_depth(grey, depth, sc['cams'], sc['poses'])
    for keep in (True, False):
        o = po.photo_depth(grey, depth, sc['cams'], sc['poses'], distance_thresh=5.0, keep_input=keep)
        assert o['info'][1] == 0 and o['info'][7] == full['info'][1] and np.array_equal(o['info'][2:7], full['info'][2:7])
        was = full['what'] == 0
        assert np.array_equal(o['depth'][was], depth[was] if keep else np.zeros(was.sum(), np.float32))
    # min_score above every score: below min_score
    o = po.photo_depth(grey, depth, sc['cams'], sc['poses'], min_score=1.0)
    assert o['info'][1] == 0 and o['info'][6] == full['info'][1] + full['info'][6]
    # min_views beyond the views that see a pixel: nothing scored there
    o = po.photo_depth(grey, depth, sc['cams'], sc['poses'], min_views=2)
    assert 0 < o['info'][1] < full['info'][1] and o['info'][5] > full['info'][5] and (o['views'][o['what'] == 0] == 2).all()


def test_found_and_an_invalid_reference_empty_the_call():
    sc = plane()
    for kw, flag in ((dict(found=np.zeros(1, np.int32)), 0), (dict(), 1)):
        cams = sc['cams'].copy()
        if not kw:
            cams[0, 1] = 0.0
        o = po.photo_depth(sc['grey'], sc['depth'], cams, sc['poses'], **kw)
        assert o['info'].tolist() == [flag, 0, 0, 0, 0, 0, 0, 0]
        assert not o['depth'].any() and np.isnan(o['score']).all() and not o['views'].any()


# ---- the ABI and the wrappers, without a GPU ---------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_takes_no_scratch():
    import re
    header = open(_lib.LIB.replace('cotr_amd/csrc/libcotr_hip.so', 'include/cotr_hip.h')).read()
    name = 'cotr_photo_depth'
    assert name in _lib.EXPORTED_SYMBOLS and name in declared_symbols()
    assert getattr(_lib.load_library(), name) is not None
    proto = re.search(r'\nint ' + name + r'\((.*?)\);', header, re.S).group(1)
    assert 'scratch' not in proto and name + '_scratch_bytes' not in header


def test_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    P, Q, R, S = (ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20), ctypes.c_void_p(4 << 20))   # never dereferenced
    G, D, C, M = ctypes.c_void_p(8 << 20), ctypes.c_void_p(9 << 20), ctypes.c_void_p(10 << 20), ctypes.c_void_p(11 << 20)
    nan, inf = float('nan'), float('inf')
    odd8, odd4 = ctypes.c_void_p((12 << 20) + 4), ctypes.c_void_p((12 << 20) + 2)

    def call(grey=G, depth_in=D, cams=C, poses=M, V=3, H=24, W=32, found=None, radius=2, steps=4, sweeps=3, rel_step=0.004, min_var=4.0, min_score=0.5,
             min_views=1, dist=50.0, keep=1, d=P, s=Q, v=R, info=S):
        return lib.cotr_photo_depth(grey, depth_in, cams, poses, V, H, W, found, radius, steps, sweeps, rel_step, min_var, min_score, min_views, dist, keep,
                                    d, s, v, info, None)

    for kw, word in ((dict(V=1), b'V must'), (dict(V=33), b'V must'), (dict(H=0), b'2^28'), (dict(W=0), b'2^28'), (dict(H=1 << 14, W=(1 << 14) + 1), b'2^28'),
                     (dict(radius=0), b'radius'), (dict(radius=5), b'radius'), (dict(steps=0), b'steps must'), (dict(steps=17), b'steps must'),
                     (dict(sweeps=0), b'sweeps'), (dict(sweeps=9), b'sweeps'), (dict(rel_step=0.0), b'rel_step'), (dict(rel_step=-0.1), b'rel_step'),
                     (dict(rel_step=nan), b'rel_step'), (dict(rel_step=inf), b'rel_step'), (dict(rel_step=0.25), b'rel_step'),
                     (dict(steps=16, rel_step=0.0625), b'rel_step'), (dict(min_var=0.0), b'min_var'), (dict(min_var=nan), b'min_var'),
                     (dict(min_var=inf), b'min_var'), (dict(min_score=1.5), b'min_score'), (dict(min_score=-1.5), b'min_score'), (dict(min_score=nan), b'min_score'),
                     (dict(min_views=0), b'min_views'), (dict(min_views=3), b'min_views'), (dict(dist=0.0), b'distance_thresh'), (dict(dist=inf), b'distance_thresh'),
                     (dict(dist=nan), b'distance_thresh'), (dict(keep=2), b'keep_input'), (dict(keep=-1), b'keep_input'), (dict(grey=None), b'NULL'),
                     (dict(depth_in=None), b'NULL'), (dict(cams=None), b'NULL'), (dict(poses=None), b'NULL'), (dict(d=None), b'NULL'), (dict(s=None), b'NULL'),
                     (dict(v=None), b'NULL'), (dict(info=None), b'NULL'), (dict(cams=odd8), b'aligned'), (dict(poses=odd8), b'aligned'),
                     (dict(depth_in=odd4), b'aligned'), (dict(d=odd4), b'aligned'), (dict(s=odd4), b'aligned'), (dict(info=odd4), b'aligned'),
                     (dict(found=odd4), b'aligned'), (dict(d=Q), b'overlap'), (dict(s=ctypes.c_void_p((1 << 20) + 24 * 32 * 4 - 4)), b'overlap'),
                     (dict(v=ctypes.c_void_p((2 << 20) + 5)), b'overlap'), (dict(info=ctypes.c_void_p((1 << 20) + 64)), b'overlap'), (dict(d=D), b'overlap'),
                     (dict(d=G), b'overlap'), (dict(v=ctypes.c_void_p((8 << 20) + 3 * 24 * 32 - 1)), b'overlap'), (dict(s=ctypes.c_void_p((10 << 20) + 116)), b'overlap'),
                     (dict(info=ctypes.c_void_p((11 << 20) + 284)), b'overlap'), (dict(found=S), b'overlap')):
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error() and b'cotr_photo_depth' in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())


K3 = np.array([[30.0, 0.1, 16.0], [0.0, 30.0, 12.0], [0.0, 0.0, 1.0]])
POSES = np.stack([np.eye(4)] * 3)
D = np.ones((24, 32), np.float32)
IMG = np.zeros((24, 32, 3), np.uint8)


def test_wrapper_argument_errors_without_a_gpu():
    for kw, word in ((dict(depth=D.astype(np.float64)), 'float32'), (dict(depth=D[0]), r'\[H, W\]'), (dict(imgs=[]), 'between 1 and 31'),
                     (dict(imgs=[IMG] * 32, Ks=K3), 'between 1 and 31'), (dict(img_ref=IMG[:, :31]), 'img_ref'), (dict(imgs=[IMG, IMG[:23]]), r'imgs\[1\]'),
                     (dict(imgs=[IMG, np.zeros((24, 32, 4), np.uint8)]), r'imgs\[1\]'), (dict(K_ref=np.eye(4)), r'\[3, 3\]'),
                     (dict(K_ref=np.diag([0.0, 1.0, 1.0])), 'focal'), (dict(Ks=np.stack([K3] * 3)), r'\[2, 3, 3\]'), (dict(c2w_ref=np.eye(3)), r'\[4, 4\]'),
                     (dict(c2w_ref=None), r'\[4, 4\]'), (dict(c2ws=POSES), 'c2ws'), (dict(c2ws=np.stack([np.eye(3)] * 2)), r'\[4, 4\]'),
                     (dict(radius=0), 'radius'), (dict(radius=5), 'radius'), (dict(radius=1.5), 'radius'), (dict(steps=0), 'steps'), (dict(steps=17), 'steps'),
                     (dict(sweeps=0), 'sweeps'), (dict(sweeps=9), 'sweeps'), (dict(rel_step=0.0), 'rel_step'), (dict(rel_step=float('nan')), 'rel_step'),
                     (dict(rel_step=0.25), 'rel_step must be < 1'), (dict(min_var=0.0), 'min_var'), (dict(min_var=float('inf')), 'min_var'),
                     (dict(min_score=1.5), 'min_score'), (dict(min_score=float('nan')), 'min_score'), (dict(min_views=0), 'min_views'),
                     (dict(min_views=3), 'min_views'), (dict(distance_thresh=0.0), 'distance_thresh'), (dict(distance_thresh=float('inf')), 'distance_thresh'),
                     (dict(found=np.ones(2, np.int32)), 'found'), (dict(img_ref=IMG.astype(np.float32)), 'uint8')):
        args = dict(depth=D, img_ref=IMG, imgs=[IMG, IMG[..., 0]], K_ref=K3, c2w_ref=np.eye(4), Ks=np.stack([K3] * 2), c2ws=POSES[:2])
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            refine_depth_photo(**args)
    from cotr_amd.data import Capture
    caps = [Capture(IMG, D, K3, np.eye(4)) for _ in range(3)]
    for args, kw, word in (((caps[:1],), {}, 'two captures'), ((caps,), dict(neighbours=3), 'neighbours'), ((caps,), dict(neighbours=0), 'neighbours'),
                           ((caps[:2] + [caps[0]._replace(image=None)],), {}, 'image'), ((caps[:2] + [caps[0]._replace(c2w=None)],), {}, r'\[4, 4\]'),
                           ((caps[:2] + [caps[0]._replace(depth=np.ones((24, 33), np.float32))],), {}, 'one depth-map size'), ((caps,), dict(radius=7), 'radius')):
        with pytest.raises(ValueError, match=word):
            refine_captures_photo(*args, **kw)
    for bad, word in ((np.zeros((4, 4, 3), np.float32), 'uint8'), (np.zeros(5, np.uint8), r'\[\.\.\., H, W\]')):
        with pytest.raises(ValueError, match=word):
            to_grey(bad)


def test_cpu_tensors_are_refused():
    for kw in (dict(depth=torch.from_numpy(D)), dict(img_ref=torch.from_numpy(IMG)), dict(imgs=[IMG, torch.from_numpy(IMG)]),
               dict(found=torch.ones(1, dtype=torch.int32))):
        args = dict(depth=D, img_ref=IMG, imgs=[IMG, IMG], K_ref=K3, c2w_ref=np.eye(4), Ks=K3, c2ws=POSES[:2])
        args.update(kw)
        with pytest.raises(_lib.CotrHipError, match='MI355X only'):
            refine_depth_photo(**args)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        to_grey(torch.zeros((4, 4, 3), dtype=torch.uint8))


def test_grey_rule():
    """(77 R + 150 G + 29 B + 128) >> 8 on every corner of the colour cube and on random colours, by the wrapper's rule and by the
    restatement's; the weights sum to 256, so grey stays grey"""
    from cotr_amd.inference.depth import grey_rule
    rng = np.random.default_rng(0)
    rgb = np.concatenate([np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8), rng.integers(0, 256, (500, 3), dtype=np.uint8)])
    want = np.array([(77 * int(r) + 150 * int(g) + 29 * int(b) + 128) >> 8 for r, g, b in rgb], np.uint8)
    assert np.array_equal(po.grey_of(rgb[None]), want[None])
    got = grey_rule(torch.from_numpy(rgb).reshape(2, 254, 3))
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy().reshape(-1), want)
    same = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    assert np.array_equal(grey_rule(torch.from_numpy(same)).numpy(), np.arange(256, dtype=np.uint8))


def test_depth_map_makes_no_photo_call_by_default():
    """photo_sweeps defaults to 0 (that no cotr_photo_depth call is then made is checked on the device)"""
    import inspect
    from cotr_amd.inference import ZoomEngine
    sig = inspect.signature(ZoomEngine.depth_map)
    assert sig.parameters['photo_sweeps'].default == 0 and sig.parameters['photo_kw'].default is None
