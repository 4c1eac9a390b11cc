"""The homography estimator without a GPU: the numpy restatement (tests/homography_oracle.py) against literal loops and
LAPACK, the scenes the GPU tests use against the properties they were chosen for, the argument checks of the C ABI (they run
before any HIP call) and of the Python wrappers, and the host logic of ZoomEngine.homography / paste_by_homography."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.build import declared_symbols
from tests import homography_oracle as ho


def _rel(a, b):
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return min(np.abs(a - b).max(), np.abs(a + b).max())


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_sampler_is_the_f_paths_draws_with_model_size_4():
    from tests import guided_oracle as go
    s4, s7 = ho.samples(15, 300, 3), go.samples(15, 300, 3)
    assert np.array_equal(s4, s7[:, :4])                       # the first 4 of the same draws
    assert (s4 >= 0).all() and all(len(set(r)) == 4 for r in s4)
    s = ho.samples(4, 50, 1)
    assert all(sorted(r) == [0, 1, 2, 3] for r in s)


@pytest.mark.parametrize('seed', range(30))
def test_vectorised_selection_equals_the_sequential_loop(seed):
    rng = np.random.default_rng(seed)
    iters, n = int(rng.integers(1, 400)), int(rng.integers(4, 300))
    conf = [0.5, 0.995, 0.999999][seed % 3]
    cnt = rng.integers(0, n + 1, iters)
    cnt[rng.random(iters) < 0.5] = -1
    cnt[rng.random(iters) < 0.3] = 4
    if seed % 4 == 0:
        cnt = np.minimum(cnt, rng.integers(4, 9))
    if seed % 5 == 0:
        cnt[iters // 3] = n - 1
    assert ho.select(cnt, iters, n, conf) == ho.select_sequential(cnt, iters, n, conf)


def test_selection_details():
    cnt = np.full(10, 3)
    assert ho.select(cnt, 10, 100, 0.995) == (0, 0, 10, -1)     # nothing beats 3
    cnt[4] = cnt[5] = 4                                          # an equal count later: the first one is kept
    assert ho.select(cnt, 10, 100, 0.995) == (1, 4, 10, 4)
    cnt[6] = 100                                                 # every point: stop after this iteration
    assert ho.select(cnt, 10, 100, 0.995) == ho.select_sequential(cnt, 10, 100, 0.995) == (1, 100, 7, 6)


def test_degenerate_samples_have_no_model():
    sq = np.array([[0, 0], [10, 0], [0, 10], [10, 10]], np.float64)
    assert ho.sample_ok(sq, sq * 2 + 3)
    line = sq.copy()
    line[2] = [5, 0]                                             # three points on a line in one set
    assert not ho.sample_ok(line, sq) and not ho.sample_ok(sq, line)
    assert ho.four_point(line, sq) is None
    twisted = sq[[0, 1, 3, 2]]                                   # two corners exchanged: some triples flip, some do not
    assert not ho.sample_ok(sq, twisted)
    mirrored = sq * [-1, 1]                                      # a reflection flips all four: kept, as in cv2
    assert ho.sample_ok(sq, mirrored)
    assert ho.four_point(np.repeat(sq[:1], 4, 0), sq) is None


@pytest.mark.parametrize('seed', range(6))
def test_a_samples_own_four_points_have_no_error(seed):
    rng = np.random.default_rng(seed)
    checked = 0
    for _ in range(40):
        # a random perspective map of random points: about half of the samples pass the degeneracy check
        p1 = ho.f32(rng.uniform(0, 640, (4, 2)))
        Ht = np.array([[rng.uniform(0.7, 1.4), rng.uniform(-0.3, 0.3), rng.uniform(-60, 60)],
                       [rng.uniform(-0.3, 0.3), rng.uniform(0.7, 1.4), rng.uniform(-60, 60)],
                       [rng.uniform(-3e-4, 3e-4), rng.uniform(-3e-4, 3e-4), 1.0]])
        for p2 in (ho.f32(ho.apply(Ht, p1)), ho.f32(rng.uniform(0, 480, (4, 2)))):
            H = ho.four_point(p1, p2)
            if H is None:
                continue
            checked += 1
            assert H[8] == 1.0
            # float64 on coordinates of a few hundred px: 1e-6 px (measured: 3.7e-10 px at the most)
            assert ho.errors(H, p1, p2).max() < 1e-12
    assert checked >= 30


@pytest.mark.parametrize('scene', ho.SCENES + ho.EDGES, ids=lambda s: f'n{s[0]}-it{s[5]}')
def test_scenes_have_the_properties_they_were_chosen_for(scene):
    n, outl, noise, thr, conf, iters, seed = scene
    p1, p2, _, Ht = ho.planar_scene(n, outl, seed, noise)
    r = ho.ransac(p1, p2, thr, conf, iters, seed)
    assert r['info'][0] and r['info'][5] == 0
    # the full-pivot elimination and numpy.linalg.solve: the same candidates, model or no model per iteration
    other, has_other = ho.candidates(p1, p2, r['samples'], ho.solve_numpy)
    mine = r['hyp_H']
    na, nb = r['hyp_count'] < 0, ~has_other
    bad = sum(1 for i in range(iters) if na[i] != nb[i] or (not na[i] and _rel(mine[i], other[i]) > 1e-7))
    assert bad <= max(2, iters // 100) and bad == 0
    if outl > 0 and iters >= 63:
        assert 0.3 < na.mean() < 0.9                             # the degeneracy check removes a large share of the samples
    # the refit beats the best 4-point sample, and does not hinge on the summation order
    assert ho.corner_error(r['H'], Ht, p1) < ho.corner_error(r['H_ransac'], Ht, p1) or n == 4
    assert ho.order_noise(p1, p2, r['mask']) <= ho.ORDER_NOISE_PX
    # Jacobi + full pivot against LAPACK's eigh + solve
    lapack = ho.refit(p1, p2, r['mask'], 10, r['H_ransac'], eig=ho.eigh_smallest, solver=ho.solve_numpy)
    assert ho.corner_error(r['H'], lapack[0], p1) <= ho.REFIT_BOUND_PX
    # refinement never raises the squared error on the inliers, and refine_iters = 0 is the DLT
    H, kept, status, H_dlt = ho.refit(p1, p2, r['mask'], 10, r['H_ransac'])
    assert ho.sq_error(H, p1, p2, r['mask']) <= ho.sq_error(H_dlt, p1, p2, r['mask']) and 0 <= kept <= 10
    H0, kept0, status0, _ = ho.refit(p1, p2, r['mask'], 0, r['H_ransac'])
    assert np.array_equal(H0, H_dlt) and kept0 == 0 and status0 == 1


@pytest.mark.parametrize('seed', range(5))
def test_jacobi_against_eigh(seed):
    rng = np.random.default_rng(seed)
    L = rng.normal(size=(40, 9)) * rng.uniform(0.1, 10, 9)
    A = L.T @ L
    # an eigenvector is determined to about eps * lambda_max / (gap to the next eigenvalue): 100 times that
    tol = lambda M: 100 * np.finfo(float).eps * (lambda w: w[-1] / (w[1] - w[0]))(np.linalg.eigvalsh(M))   # noqa: E731
    e, ref = ho.jacobi_smallest(A), ho.eigh_smallest(A)
    assert abs(np.linalg.norm(e) - 1) < 1e-14 and _rel(e, ref) < tol(A) < 1e-10
    # an exact null vector (4 inliers: rank 8)
    p1, p2, _, _ = ho.planar_scene(4, 0.0, seed, 0.0)
    X, Y, U, V = p1[:, 0] / 300 - 1, p1[:, 1] / 300 - 1, p2[:, 0] / 300 - 1, p2[:, 1] / 300 - 1
    A = ho.dlt_matrix(X, Y, U, V)
    assert _rel(ho.jacobi_smallest(A), ho.eigh_smallest(A)) < tol(A)


def test_full_pivot_elimination_against_numpy():
    rng = np.random.default_rng(0)
    for _ in range(20):
        A, b = rng.normal(size=(8, 8)), rng.normal(size=8)
        assert np.abs(ho.solve_full_pivot(A, b) - np.linalg.solve(A, b)).max() < 1e-10
    A[3] = A[2]
    assert ho.solve_full_pivot(A, b) is None


def test_nothing_found_and_collinear_points():
    x = 2.0 * np.arange(50)                                     # exact in float32: the cross products are exactly 0
    p = np.stack([x, 0.5 * x + 7], 1)
    r = ho.ransac(p, p + 3, 3.0, 0.995, 200, 0)
    assert not r['info'][0] and (r['hyp_count'] == -1).all() and (r['H'] == 0).all() and not r['mask'].any()
    q = np.array([[0, 0], [10, 10], [20, 20], [5, 30]], np.float64)
    r = ho.ransac(q, q, 3.0, 0.995, 50, 0)
    assert not r['info'][0] and list(r['info'][:6]) == [0, 0, 50, -1, 0, 2]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    for name in ('cotr_ransac_homography', 'cotr_ransac_homography_scratch_bytes'):
        assert name in _lib.EXPORTED_SYMBOLS and name in declared_symbols()
        assert getattr(_lib.load_library(), name) is not None


def test_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    b = ctypes.c_size_t()
    P = ctypes.c_void_p(4096)           # never dereferenced: every call below fails its checks before any HIP call
    for n in (3, (1 << 24) + 1):
        assert lib.cotr_ransac_homography_scratch_bytes(n, 100, ctypes.byref(b)) == -1
        assert b'[4, 2^24]' in lib.cotr_raster_last_error()
    for iters in (0, 65537):
        assert lib.cotr_ransac_homography_scratch_bytes(100, iters, ctypes.byref(b)) == -1
        assert b'max_iters' in lib.cotr_raster_last_error()
    assert lib.cotr_ransac_homography_scratch_bytes(100, 100, None) == -1
    assert b'NULL' in lib.cotr_raster_last_error()
    assert lib.cotr_ransac_homography_scratch_bytes(4, 1, ctypes.byref(b)) == 0 and b.value > 0
    assert lib.cotr_ransac_homography_scratch_bytes(1 << 24, 65536, ctypes.byref(b)) == 0
    assert b.value >= 65536 * 76 + 8192 * 45 * 8
    assert lib.cotr_ransac_homography_scratch_bytes(100, 1000, ctypes.byref(b)) == 0
    need = b.value

    def call(n=100, thr=3.0, conf=0.995, iters=1000, refine=10, pts=P, out=P, scratch=P, nbytes=need, hyp=None):
        return lib.cotr_ransac_homography(pts, P, n, thr, conf, iters, refine, 0, out, P, P, None, hyp, None, None, scratch, nbytes, None)
    for kw, word in ((dict(n=3), b'[4, 2^24]'), (dict(n=(1 << 24) + 1), b'[4, 2^24]'), (dict(iters=0), b'max_iters'),
                     (dict(iters=65537), b'max_iters'), (dict(refine=-1), b'refine_iters'), (dict(refine=65), b'refine_iters'),
                     (dict(thr=0.0), b'threshold'), (dict(thr=-1.0), b'threshold'), (dict(thr=float('nan')), b'threshold'),
                     (dict(thr=float('inf')), b'threshold'), (dict(conf=0.0), b'confidence'), (dict(conf=1.0), b'confidence'),
                     (dict(conf=float('nan')), b'confidence'), (dict(pts=None), b'NULL'), (dict(out=None), b'NULL'),
                     (dict(scratch=None), b'NULL'), (dict(scratch=ctypes.c_void_p(4104)), b'aligned'),
                     (dict(hyp=ctypes.c_void_p(4100)), b'aligned'), (dict(nbytes=need - 1), b'smaller')):
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
def test_wrapper_argument_errors_without_a_gpu():
    from cotr_amd.inference import find_homography, ransac_homography
    z = np.zeros((20, 2))
    with pytest.raises(ValueError, match='at least 4'):
        find_homography(np.zeros((3, 2)), np.zeros((3, 2)))
    with pytest.raises(ValueError, match='same length'):
        find_homography(z, np.zeros((21, 2)))
    with pytest.raises(ValueError, match=r'\[N, 2\]'):
        find_homography(np.zeros((20, 3)), np.zeros((20, 3)))
    with pytest.raises(ValueError, match='max_iters'):
        find_homography(z, z, max_iters=0)
    with pytest.raises(ValueError, match='max_iters'):
        find_homography(z, z, max_iters=65537)
    with pytest.raises(ValueError, match='threshold'):
        find_homography(z, z, 0.0)
    with pytest.raises(ValueError, match='threshold'):
        find_homography(z, z, float('inf'))
    with pytest.raises(ValueError, match='confidence'):
        find_homography(z, z, confidence=1.0)
    for bad in (-1, 65):
        with pytest.raises(ValueError, match='refine_iters'):
            ransac_homography(z, z, refine_iters=bad)


def test_paste_by_homography_argument_checks():
    from cotr_amd.inference import paste_by_homography
    pic, img = np.zeros((20, 30, 3), np.uint8), np.zeros((40, 50, 3), np.uint8)
    pts = np.zeros((6, 2))
    with pytest.raises(ValueError, match='uint8'):
        paste_by_homography(pic.astype(np.float32), pts, pts, img)
    with pytest.raises(ValueError, match='img_b'):
        paste_by_homography(pic, pts, pts, np.zeros((40, 50, 2), np.uint8))
    with pytest.raises(ValueError, match=r'\[N, 2\]'):
        paste_by_homography(pic, pts, np.zeros((5, 2)), img)
    with pytest.raises(ValueError, match=r'\[N, 2\]'):
        paste_by_homography(pic, np.zeros((6, 3)), np.zeros((6, 3)), img)
    with pytest.raises(ValueError, match='at least 4'):
        paste_by_homography(pic, pts[:3], pts[:3], img)
    sq, sq_b = np.array([[0, 0], [30, 0], [0, 20], [30, 20]]), np.array([[5, 5], [40, 8], [6, 30], [44, 33]])
    with pytest.raises(TypeError, match='unexpected keyword'):  # the 4-point path makes no estimator call: keywords checked all the same
        paste_by_homography(pic, sq, sq_b, img, treshold=3.0)
    for kw, word in ((dict(max_iters=0), 'max_iters'), (dict(ransac_reproj_threshold=0.0), 'threshold'), (dict(confidence=1.0), 'confidence')):
        with pytest.raises(ValueError, match=word):
            paste_by_homography(pic, sq, sq_b, img, **kw)
    with pytest.raises(ValueError, match='singular'):           # four points, three on a line: get_perspective_transform's error
        paste_by_homography(pic, np.array([[0, 0], [1, 1], [2, 2], [0, 5]]), np.array([[0, 0], [1, 1], [2, 2], [0, 5]]), img)


@pytest.fixture
def oracle_device(monkeypatch):
    """find_homography answered by the restatement, on the host"""
    from cotr_amd.inference import homography
    calls = []

    def find_homography(src, dst, ransac_reproj_threshold=3.0, max_iters=2000, confidence=0.995, seed=0):
        if len(src) < 4:
            raise ValueError('a homography needs at least 4 correspondences')
        calls.append((ransac_reproj_threshold, max_iters, confidence, seed))
        r = ho.ransac(np.asarray(src), np.asarray(dst), ransac_reproj_threshold, confidence, max_iters, seed)
        if not r['info'][0]:
            return None, None
        return r['H'].reshape(3, 3), r['mask'].astype(np.uint8).reshape(-1, 1)
    monkeypatch.setattr(homography, 'find_homography', find_homography)
    return calls


def test_zoom_engine_homography_host_logic(oracle_device):
    from cotr_amd.inference import FasterSparseEngine, SparseEngine, ZoomEngine
    from oracle.dense_post import host_dense_post_factory
    from tests.engine_fixtures import FakeModel, pil_cropper_factory, synthetic_pair
    assert SparseEngine.homography is ZoomEngine.homography and FasterSparseEngine.homography is ZoomEngine.homography
    img_a, img_b = synthetic_pair(1)
    eng = ZoomEngine(FakeModel(), make_cropper=pil_cropper_factory, make_dense_post=host_dense_post_factory)
    rng = np.random.default_rng(0)
    q = np.stack([rng.uniform(5, img_a.shape[1] - 5, 12), rng.uniform(5, img_a.shape[0] - 5, 12)], 1).astype(np.float32)
    zooms = np.linspace(0.5, 0.0625, 4)
    with torch.no_grad():
        want = eng.cotr_corr_multiscale(img_a, img_b, zooms, 1, max_corrs=1000, queries_a=q, force=True)
        H, corrs, mask = eng.homography(img_a, img_b, queries_a=q, ransac_reproj_threshold=50.0, max_iters=100, seed=3)
    assert oracle_device == [(50.0, 100, 0.995, 3)]
    assert np.array_equal(corrs, want) and corrs.shape == (12, 4)
    ref = ho.ransac(want[:, :2], want[:, 2:], 50.0, 0.995, 100, 3)
    if ref['info'][0]:
        assert np.array_equal(H, ref['H'].reshape(3, 3)) and np.array_equal(mask[:, 0].astype(bool), ref['mask'])
        assert mask.shape == (12, 1) and mask.dtype == np.uint8
    else:
        assert H is None and mask is None

    class Spy(ZoomEngine):
        def __init__(self):
            self.calls = []

        def cotr_corr_multiscale(self, img_a, img_b, zoom_ins=(1.0,), converge_iters=1, max_corrs=1000, queries_a=None, **kw):
            self.calls.append((img_a, img_b, tuple(zoom_ins), converge_iters, max_corrs, None if queries_a is None else queries_a.shape, kw))
            return want[:3] if img_a == 'few' else want
    spy = Spy()
    spy.homography('a', 'b', max_corrs=77)
    spy.homography('a', 'b', queries_a=q, converge_iters=2)
    assert spy.calls == [('a', 'b', tuple(zooms), 1, 77, None, {}), ('a', 'b', tuple(zooms), 2, 1000, (12, 2), {'force': True})]
    with pytest.raises(ValueError, match='at least 4'):
        spy.homography('few', 'b')
