"""The 3D-3D registration without a GPU: the numpy restatement (tests/rigid3d_oracle.py) against ground truth, its two
numerical routes against each other and its selection against the literal loop, the order noise behind the GPU tests' refit
bound, degenerate samples, and the argument checks of the C ABI (they run before any HIP call) and of the Python wrappers."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.build import declared_symbols
from cotr_amd.inference import ransac_rigid3d, register_captures, register_points
from tests import rigid3d_oracle as go

NAMES = ['cotr_ransac_rigid3d_scratch_bytes', 'cotr_ransac_rigid3d']


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_sampler_is_the_f_paths_draws_with_model_size_3():
    from tests import guided_oracle as fo
    assert np.array_equal(go.samples(40, 300, 3), fo.samples(40, 300, 3)[:, :3])
    assert all(sorted(r) == [0, 1, 2] for r in go.samples(3, 50, 1))
    assert (go.samples(2, 10, 0)[:, 2] == -1).all()


@pytest.mark.parametrize('case', go.CASES, ids=go.case_id)
def test_the_two_routes_agree_and_every_candidate_is_a_rotation(case):
    # route A (Umeyama by SVD) against route B (Horn's N by eigh): the bound of DESIGN.md 3h, the family's cap of 1 % of the
    # iterations.  This keeps the GPU test's cap honest: the reference alone must stay within it.
    scene, ws = case
    ref = go.reference(scene, ws)
    o = ref['ransac']
    iters = scene[5]
    tA, hasA = go.candidates(ref['src'], ref['dst'], o['samples'], ws, 'svd')
    bad, worst = 0, 0.0
    for it in range(iters):
        if hasA[it] != o['has'][it]:
            bad += 1
        elif hasA[it]:
            d = go.candidate_distance(tA[it], o['hyp_model'][it], ws)
            bad += d > 1e-7
            worst = max(worst, d) if d <= 1e-7 else worst
    print(f'{go.case_id(case)}: {bad} of {iters} iterations outside 1e-7, worst agreement {worst:.2e}')
    assert bad <= iters // 100
    sR, _, s = go.expand(o['hyp_model'][o['has']], ws)
    R = sR / s[:, None, None]
    assert np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(R) - 1).max() < 1e-12
    if not ws:
        assert (s == 1.0).all()


@pytest.mark.parametrize('ws', [False, True], ids=['rigid', 'similarity'])
def test_noise_free_scenes_recover_the_scene(ws):
    # float64 points without rounding or noise: the closed form is exact up to the rounding of the moments; the clouds'
    # coordinates are below 32, so 1e-12 allows a condition number of about 1e3 on top of the 1e-16 of a sum
    for seed in range(4):
        rng = np.random.default_rng(seed)
        R, t = go.rotation(rng.normal(size=3), rng.uniform(0.2, 2.5)), rng.uniform(-3, 3, 3)
        s = float(rng.uniform(0.5, 2.0)) if ws else 1.0
        src = go.CENTRE + rng.uniform(-2, 2, (200, 3))
        dst = s * (src @ R.T) + t
        o = go.ransac(src, dst, 0.01, 0.99, 50, seed, ws, 2)
        assert o['info'][0] and o['info'][1] == 200 and o['mask'].all() and o['info'][4] == 2
        assert np.abs(o['R'] - R).max() < 1e-12 and np.abs(o['t'] - t).max() < 1e-12 and abs(o['scale'] - s) < 1e-12
        cand = o['hyp_model'][o['info'][3]]
        sR, tc, sc = go.expand(cand, ws)
        assert np.abs(sR - s * R).max() < 1e-11 and np.abs(tc - t).max() < 1e-10
    # the float32-rounded scenes of the GPU tests: within the rounding of the points
    for scene in (go.SCENES[2], go.SCENES[3], go.EDGES[0]):
        ref = go.reference(scene, ws)
        e = go.scene_errors(ref['ransac']['R'], ref['ransac']['t'], ref['ransac']['scale'], ref)
        assert max(e) < 1e-6, e


@pytest.mark.parametrize('case', go.CASES, ids=go.case_id)
def test_selection_equals_the_literal_loop_and_a_model_is_found(case):
    scene, ws = case
    n, outl, noise, thr, conf, iters, seed = scene
    o = go.reference(scene, ws)['ransac']
    assert tuple(o['info'][:4]) == go.select_sequential(o['hyp_count'], iters, n, conf) == go.select(o['hyp_count'], iters, n, conf)
    assert o['info'][0] == 1 and o['info'][4] == 2 and o['info'][5] == o['mask'].sum() >= 3


def test_order_noise_stays_below_the_recorded_constant():
    worst = max(go.order_noise(scene, ws) for scene, ws in go.CASES)
    print(f'order noise {worst:.3e} (recorded {go.ORDER_NOISE:.1e})')
    assert worst <= go.ORDER_NOISE and go.REFIT_BOUND == 1000 * go.ORDER_NOISE


def test_collinear_and_nan_samples_give_no_candidate():
    # exactly collinear integer points: the cross product is exactly 0
    line = np.array([1.0, -2.0, 3.0]) + np.arange(40)[:, None] * np.array([2.0, 1.0, -3.0])
    cloud = go.rigid_scene(40, 0.0, 0, 0.0, False)[0]
    smp = go.samples(40, 64, 0)
    for src, dst in ((line, cloud), (cloud, line), (line, line)):
        for ws in (False, True):
            table, has = go.candidates(src, dst, smp, ws)
            assert not has.any() and np.isnan(table).all()
            o = go.ransac(src, dst, 0.1, 0.99, 64, 0, ws)
            assert list(o['info']) == [0, 0, 64, -1, 0, 0, 0, 0] and (o['hyp_count'] == -1).all()
    bad = cloud.copy()
    bad[7] = np.nan
    _, has = go.candidates(bad, cloud, smp, False)
    assert np.array_equal(has, ~(smp == 7).any(axis=1))
    # a short draw (n = 2 cannot fill a sample)
    _, has = go.candidates(cloud[:2], cloud[:2], go.samples(2, 8, 0), False)
    assert not has.any()


def test_skip_rule_of_the_refit():
    src, dst, R, t, s, good = go.rigid_scene(50, 0.0, 3, 0.0, False)
    sR, tt, ss, mask, run = go.refit(src, dst, np.arange(50) < 2, 0.01, False, R, t, 1.0, 2)   # 2 points: skipped, model kept
    assert run == 0 and sR is R and tt is t and mask.sum() == 2
    line = src[0] + np.arange(50)[:, None] * np.array([0.25, 0.5, -0.125])
    assert go.fit(line, line @ R.T + t, np.ones(50, bool), False) is None            # collinear inliers: degenerate moments
    assert go.fit(src, dst, np.ones(50, bool), False) is not None


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and name in declared_symbols()
        assert getattr(_lib.load_library(), name) is not None


def test_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    b = ctypes.c_size_t()
    P = ctypes.c_void_p(4096)           # never dereferenced: every call below fails its checks before any HIP call
    for n in (2, (1 << 24) + 1):
        assert lib.cotr_ransac_rigid3d_scratch_bytes(n, 100, ctypes.byref(b)) == -1 and b'[3, 2^24]' in lib.cotr_raster_last_error()
    for iters in (0, (1 << 16) + 1):
        assert lib.cotr_ransac_rigid3d_scratch_bytes(100, iters, ctypes.byref(b)) == -1 and b'max_iters' in lib.cotr_raster_last_error()
    assert lib.cotr_ransac_rigid3d_scratch_bytes(100, 100, None) == -1 and b'NULL' in lib.cotr_raster_last_error()
    assert lib.cotr_ransac_rigid3d_scratch_bytes(3, 1, ctypes.byref(b)) == 0 and b.value >= 76 + 11 * 8 + 3
    assert lib.cotr_ransac_rigid3d_scratch_bytes(1 << 24, 1 << 16, ctypes.byref(b)) == 0 and b.value >= 65536 * 76 + 8192 * 11 * 8 + (1 << 24)
    assert lib.cotr_ransac_rigid3d_scratch_bytes(100, 100, ctypes.byref(b)) == 0
    need = b.value

    def call(n=100, thr=0.05, conf=0.99, iters=100, ws=0, rounds=2, src=P, dst=P, R=P, t=P, scale=P, mask=P, info=P, scratch=P, nbytes=need,
             hyp=None, cnt=None, smp=None):
        return lib.cotr_ransac_rigid3d(src, dst, n, thr, conf, iters, 0, ws, rounds, R, t, scale, mask, info, hyp, cnt, smp, scratch, nbytes, None)
    for kw, word in ((dict(n=2), b'[3, 2^24]'), (dict(n=(1 << 24) + 1), b'[3, 2^24]'), (dict(iters=0), b'max_iters'),
                     (dict(iters=(1 << 16) + 1), b'max_iters'), (dict(thr=0.0), b'threshold'), (dict(thr=-1.0), b'threshold'),
                     (dict(thr=float('nan')), b'threshold'), (dict(thr=float('inf')), b'threshold'), (dict(thr=1e30), b'squared threshold'),
                     (dict(thr=1e-30), b'squared threshold'), (dict(conf=0.0), b'confidence'), (dict(conf=1.0), b'confidence'),
                     (dict(conf=float('nan')), b'confidence'), (dict(ws=-1), b'with_scale'), (dict(ws=2), b'with_scale'),
                     (dict(rounds=-1), b'rounds'), (dict(rounds=9), b'rounds'), (dict(src=None), b'NULL'), (dict(dst=None), b'NULL'),
                     (dict(R=None), b'NULL'), (dict(t=None), b'NULL'), (dict(scale=None), b'NULL'), (dict(mask=None), b'NULL'),
                     (dict(info=None), b'NULL'), (dict(scratch=None), b'NULL'), (dict(src=ctypes.c_void_p(4100)), b'aligned'),
                     (dict(R=ctypes.c_void_p(4100)), b'aligned'), (dict(t=ctypes.c_void_p(4100)), b'aligned'),
                     (dict(scale=ctypes.c_void_p(4100)), b'aligned'), (dict(info=ctypes.c_void_p(4098)), b'aligned'),
                     (dict(scratch=ctypes.c_void_p(4104)), b'aligned'), (dict(hyp=ctypes.c_void_p(4100)), b'aligned'),
                     (dict(cnt=ctypes.c_void_p(4098)), b'aligned'), (dict(smp=ctypes.c_void_p(4098)), b'aligned'), (dict(nbytes=need - 1), b'smaller')):
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())
        assert b'cotr_ransac_rigid3d' in lib.cotr_raster_last_error()


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
K = np.array([[800.0, 1.5, 320.0], [0.0, 780.0, 240.0], [0.0, 0.0, 1.0]])


def _capture(depth=None, K_=K, c2w=None):
    from cotr_amd.data import Capture
    return Capture(None, np.ones((10, 12), np.float32) if depth is None else depth, K_, np.eye(4) if c2w is None else c2w)


def test_wrapper_argument_errors_without_a_gpu():
    o, p = np.zeros((20, 3)), np.zeros((20, 2))
    for fn in (ransac_rigid3d, register_points):
        with pytest.raises(ValueError, match='at least 3'):
            fn(np.zeros((2, 3)), np.zeros((2, 3)), 0.1)
        with pytest.raises(ValueError, match='same length'):
            fn(o, np.zeros((21, 3)), 0.1)
        with pytest.raises(ValueError, match=r'src must be \[N, 3\]'):
            fn(p, o, 0.1)
        with pytest.raises(ValueError, match=r'dst must be \[N, 3\]'):
            fn(o, p, 0.1)
        for kw, word in ((dict(max_iters=0), 'max_iters'), (dict(max_iters=(1 << 16) + 1), 'max_iters'), (dict(threshold=0.0), 'threshold'),
                         (dict(threshold=float('inf')), 'threshold'), (dict(threshold=float('nan')), 'threshold'), (dict(threshold=1e30), 'squared'),
                         (dict(confidence=0.0), 'confidence'), (dict(confidence=1.0), 'confidence'), (dict(with_scale=2), 'with_scale'),
                         (dict(with_scale='yes'), 'with_scale'), (dict(rounds=-1), 'rounds'), (dict(rounds=9), 'rounds'), (dict(rounds=1.5), 'rounds')):
            args = dict(threshold=0.1)
            args.update(kw)
            with pytest.raises(ValueError, match=word):
                fn(o, o, **args)
            with pytest.raises(ValueError, match=word):
                register_captures(p, p, _capture(), _capture(), **args)
    with pytest.raises(ValueError, match='at least 3'):
        register_captures(np.zeros((2, 2)), np.zeros((2, 2)), _capture(), _capture())
    with pytest.raises(ValueError, match='same length'):
        register_captures(p, np.zeros((21, 2)), _capture(), _capture())
    with pytest.raises(ValueError, match=r'\[N, 2\]'):
        register_captures(o, p, _capture(), _capture())
    with pytest.raises(ValueError, match='float32'):
        register_captures(p, p, _capture(depth=np.ones((10, 12))), _capture())
    with pytest.raises(ValueError, match='float32'):
        register_captures(p, p, _capture(), _capture(depth=np.ones((10, 12))))
    with pytest.raises(ValueError, match=r'\[4, 4\]'):
        register_captures(p, p, _capture(c2w=np.eye(3)), _capture())
    with pytest.raises(ValueError, match='focal'):
        register_captures(p, p, _capture(), _capture(K_=np.diag([0.0, 1.0, 1.0])))
    with pytest.raises(TypeError, match='unexpected keyword'):
        register_captures(p, p, _capture(), _capture(), treshold=1.0)


def test_cpu_tensors_are_refused():
    o, p = torch.zeros((20, 3), dtype=torch.float64), torch.zeros((20, 2), dtype=torch.float64)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        ransac_rigid3d(o, o.numpy(), 0.1)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        register_points(o.numpy(), o, 0.1)
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        register_captures(p, p.numpy(), _capture(), _capture())
    with pytest.raises(_lib.CotrHipError, match='MI355X only'):
        register_captures(p.numpy(), p.numpy(), _capture(), _capture(depth=torch.ones((10, 12))))


def test_zoom_engine_register_host_logic(monkeypatch):
    from cotr_amd.inference import FasterSparseEngine, SparseEngine, ZoomEngine, rigid3d
    assert SparseEngine.register is ZoomEngine.register and FasterSparseEngine.register is ZoomEngine.register
    want = np.random.default_rng(0).uniform(0, 100, (12, 4))
    calls = []

    def fake(pa, pb, cap_a, cap_b, **kw):
        calls.append((pa.copy(), pb.copy(), cap_a, cap_b, kw))
        return 'c2w', 'mask'
    monkeypatch.setattr(rigid3d, 'register_captures', fake)

    class Spy(ZoomEngine):
        def __init__(self):
            self.calls = []

        def cotr_corr_multiscale(self, img_a, img_b, zoom_ins=(1.0,), converge_iters=1, max_corrs=1000, queries_a=None, **kw):
            self.calls.append((img_a, img_b, tuple(zoom_ins), converge_iters, max_corrs, None if queries_a is None else queries_a.shape, kw))
            return want
    from cotr_amd.data import Capture
    cap_a, cap_b = Capture('image a', 'depth', 'K', 'c2w'), Capture('image b', 'depth', 'K', None)
    spy, zooms = Spy(), np.linspace(0.5, 0.0625, 4)
    c2w, corrs, mask = spy.register(cap_a, cap_b, max_corrs=77, seed=3)
    assert (c2w, mask) == ('c2w', 'mask') and np.array_equal(corrs, want)
    c2w, corrs, mask = spy.register(cap_a, cap_b, queries_a=np.zeros((12, 2)), converge_iters=2, with_scale=True)
    assert (c2w, mask) == ('c2w', 'mask') and np.array_equal(corrs, want)
    assert spy.calls == [('image a', 'image b', tuple(zooms), 1, 77, None, {}), ('image a', 'image b', tuple(zooms), 2, 1000, (12, 2), {'force': True})]
    assert [c[2:] for c in calls] == [(cap_a, cap_b, {'seed': 3}), (cap_a, cap_b, {'with_scale': True})]
    assert all(np.array_equal(c[0], want[:, :2]) and np.array_equal(c[1], want[:, 2:]) for c in calls)
