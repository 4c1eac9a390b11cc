"""Guided matching without a GPU: the numpy restatement (tests/guided_oracle.py) against literal transcriptions of the demo
and of the sequential RANSAC loop, the 7-point solver's candidates, OpenCV's iteration update, the argument checks of the C
ABI (they run before any HIP call) and of the Python wrappers, and the host logic of filter_guided_matches / guided_match
with the device calls answered by the restatement."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import ZoomEngine, filter_guided_matches, find_fundamental_mat, guided, mutual_matches
from tests import guided_oracle as go


# ---- nearest and mutual -----------------------------------------------------------------------------------------------
def test_distances_are_scipys_bit_for_bit():
    spatial = pytest.importorskip('scipy.spatial')
    rng = np.random.default_rng(0)
    q, k = rng.uniform(-50, 1100, (300, 2)), rng.uniform(0, 1024, (700, 2)).astype(np.float32)
    assert np.array_equal(go.distances(q, k), spatial.distance_matrix(q, k))
    assert np.array_equal(go.nearest(q, k, rows=37), np.argmin(spatial.distance_matrix(q, k), axis=1))


@pytest.mark.parametrize('na,nb,seed', [(1, 1, 0), (30, 20, 1), (60, 90, 2), (120, 120, 3)])
def test_vectorised_mutual_rule_equals_the_demo_loop(na, nb, seed):
    rng = np.random.default_rng(seed)
    kp_a = rng.integers(0, 6, (na, 2)).astype(np.float64)      # duplicate keypoints
    kp_b = rng.integers(0, 6, (nb, 2)).astype(np.float64)
    pred_ab = rng.integers(-1, 13, (na, 2)) / 2.0                # ties at half-integer positions
    pred_ba = rng.integers(-1, 13, (nb, 2)) / 2.0
    for j in range(0, min(na, nb), 3):
        pred_ab[j], pred_ba[j] = kp_b[j], kp_a[j]
    ia, ib = go.nearest(pred_ab, kp_b), go.nearest(pred_ba, kp_a)
    i = np.flatnonzero(go.mutual(ia, ib))
    assert np.array_equal(np.stack([i, ia[i]], 1), go.demo_double_loop(ia, ib))


def test_nearest_takes_the_first_minimum_and_nan_first():
    k = np.array([[1.0, 0], [0, 1], [-1, 0], [np.nan, 0], [0, 0], [np.nan, 1]])
    assert go.nearest(np.zeros((1, 2)), k[:3])[0] == 0
    assert go.nearest(np.zeros((1, 2)), k)[0] == 3
    assert go.nearest(np.array([[np.nan, 0.0]]), k[:3])[0] == 0


# ---- sampler, solver, update, selection ----------------------------------------------------------------------------------
def test_sampler_draws_distinct_indices_in_range_and_is_counter_based():
    s = go.samples(15, 400, 3)
    assert (s >= 0).all() and (s < 15).all()
    assert all(len(set(r)) == 7 for r in s)
    assert np.array_equal(go.samples(15, 100, 3), s[:100])        # iteration it does not depend on max_iters
    assert not np.array_equal(go.samples(15, 100, 4), s[:100])
    # draw d of iteration it, written out with Python integers
    def mix(x):
        m = (1 << 64) - 1
        z = (x + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)
    for it in (0, 1, 399):
        got = []
        for d in range(64):
            c = (mix(mix(3) ^ (it << 6 | d)) >> 32) % 15
            if c not in got:
                got.append(c)
            if len(got) == 7:
                break
        assert list(s[it]) == got


@pytest.mark.parametrize('seed', range(6))
def test_seven_point_candidates_satisfy_their_constraints(seed):
    rng = np.random.default_rng(seed)
    p1, p2 = go.f32(rng.uniform(0, 1000, (7, 2))), go.f32(rng.uniform(0, 800, (7, 2)))
    Fs = go.seven_point(p1, p2)
    assert 1 <= len(Fs) <= 3
    h1, h2 = np.hstack([p1, np.ones((7, 1))]), np.hstack([p2, np.ones((7, 1))])
    for F in Fs:
        M = F.reshape(3, 3)
        nrm = np.linalg.norm(M)
        res = np.abs(np.einsum('ni,ij,nj->n', h2, M, h1)) / (nrm * np.linalg.norm(h1, axis=1) * np.linalg.norm(h2, axis=1))
        assert res.max() < 1e-9
        assert abs(np.linalg.det(M)) / nrm ** 3 < 1e-10
        assert F[8] == 1.0


def test_seven_point_degenerate_sample_gives_nothing():
    p = go.f32(np.random.default_rng(0).uniform(0, 100, (7, 2)))
    assert go.seven_point(np.repeat(p[:1], 7, 0), p) == []
    q = p.copy()
    q[1] = q[0]
    q2 = p.copy()
    q2[1] = q2[0]
    assert go.seven_point(q, q2) == []                           # a repeated pair: rank 6


def test_cubic_roots_ascending_and_degenerate_orders():
    assert go.cubic_roots(1.0, -6.0, 11.0, -6.0) == pytest.approx([1.0, 2.0, 3.0])
    assert go.cubic_roots(1.0, 0.0, 0.0, -8.0) == pytest.approx([2.0])
    assert go.cubic_roots(0.0, 1.0, -3.0, 2.0) == pytest.approx([1.0, 2.0])
    assert go.cubic_roots(0.0, 0.0, 2.0, -1.0) == [0.5]
    assert go.cubic_roots(0.0, 0.0, 0.0, 1.0) == []


def test_update_known_values():
    assert go.update(0.99, 0.0, 7, 1000) == 0                    # every point an inlier: stop
    assert go.update(0.99, 1.0, 7, 1000) == 1000                 # log(1) = 0: keep N
    assert go.update(0.999999, 0.5, 7, 1000) == 1000             # the bound exceeds N: keep N
    # log(0.01) / log(1 - 0.5^7) = -4.60517 / -0.0078431 = 587.2
    assert go.update(0.99, 0.5, 7, 1000) == 587
    assert go.update(0.99, 0.5, 7, 500) == 500
    assert go.update(0.99, 0.2, 7, 1000) == int(np.rint(np.log(0.01) / np.log(1 - 0.8 ** 7)))
    assert go.update(1 - 1e-300, 0.3, 7, 65536) == int(np.rint(np.log(go.DBL_MIN) / np.log(1 - 0.7 ** 7))) == 8243  # 1 - p: DBL_MIN


def _random_counts(rng, iters, n):
    c = rng.integers(0, n + 1, 3 * iters)
    c[rng.random(3 * iters) < 0.3] = -1                         # slots without a candidate
    c[rng.random(3 * iters) < 0.3] = 7
    return c


@pytest.mark.parametrize('seed', range(40))
def test_vectorised_selection_equals_the_sequential_loop(seed):
    rng = np.random.default_rng(seed)
    iters, n = int(rng.integers(1, 400)), int(rng.integers(15, 300))
    conf = [0.5, 0.99, 0.999999][seed % 3]
    cnt = _random_counts(rng, iters, n)
    if seed % 4 == 0:                 # plateaus of equal counts
        cnt = np.minimum(cnt, rng.integers(7, 12))
    if seed % 5 == 0:                 # one near-perfect candidate: early stop
        cnt[3 * (iters // 3)] = n - 1
    assert go.select(cnt, iters, n, conf) == go.select_sequential(cnt, iters, n, conf)


def test_selection_details():
    n = 100
    cnt = np.full(30, 5)
    assert go.select(cnt, 10, n, 0.99) == (0, 0, 10, -1)        # nothing beats 6
    cnt[4] = 7
    cnt[5] = 7                                                    # equal count later: the first one is kept
    assert go.select(cnt, 10, n, 0.99) == (1, 7, 10, 4)
    cnt[6] = 100                                                  # every point: stop after this iteration
    assert go.select(cnt, 10, n, 0.99) == go.select_sequential(cnt, 10, n, 0.99) == (1, 100, 3, 6)
    cnt[3] = 100                                                  # the rest of the iteration is still looked at
    cnt[4] = 100
    assert go.select(cnt, 10, n, 0.99) == (1, 100, 2, 3)


def test_counts_of_empty_and_non_finite_slots():
    p1, p2, _, _ = go.two_view_scene(50, 0.2, 0)
    H = np.full((3, 9), np.nan)
    H[1] = np.inf
    H[2] = go.seven_point(go.f32(p1[:7]), go.f32(p2[:7]))[0]
    c = go.counts(H, p1, p2, 3.0)
    assert c[0] == -1 and c[1] == 0 and c[2] >= 7


@pytest.mark.parametrize('n,outl,thr,conf,iters,seed', go.EDGES)
def test_edge_scenes_find_a_model(n, outl, thr, conf, iters, seed):
    p1, p2, _, _ = go.two_view_scene(n, outl, seed)
    r = go.ransac(p1, p2, thr, conf, iters, seed)
    assert len(p1) == n and r['samples'].shape == (iters, 7)
    if iters >= 63:
        assert r['info'][0] == 1 and r['info'][1] >= 7 and r['mask'].sum() == r['info'][1]


# ---- the C ABI's argument checks ----------------------------------------------------------------------------------------
def test_abi_argument_errors_without_a_gpu():
    lib = _lib.load_library()
    b = ctypes.c_size_t()
    P = ctypes.c_void_p(4096)           # never dereferenced: every call below fails its checks before any HIP call
    assert lib.cotr_nearest_mutual_scratch_bytes(0, 5, ctypes.byref(b)) == -1
    assert b'[1, 2^24]' in lib.cotr_raster_last_error()
    assert lib.cotr_nearest_mutual_scratch_bytes(5, 5, None) == -1
    assert lib.cotr_nearest_mutual_scratch_bytes(2048, 2048, ctypes.byref(b)) == 0 and b.value > 0
    need = b.value
    assert lib.cotr_nearest_mutual(P, P, P, None, 2048, 2048, P, P, P, P, need, None) == -1
    assert b'NULL' in lib.cotr_raster_last_error()
    assert lib.cotr_nearest_mutual(P, P, P, P, 2048, 2048, P, P, P, ctypes.c_void_p(4100), need, None) == -1
    assert b'aligned' in lib.cotr_raster_last_error()
    assert lib.cotr_nearest_mutual(P, P, P, P, 2048, 2048, P, P, P, P, need - 1, None) == -1
    assert b'smaller' in lib.cotr_raster_last_error()

    assert lib.cotr_ransac_fundamental_scratch_bytes(14, 100, ctypes.byref(b)) == -1
    assert b'LMedS' in lib.cotr_raster_last_error()
    for iters in (0, 65537):
        assert lib.cotr_ransac_fundamental_scratch_bytes(100, iters, ctypes.byref(b)) == -1
        assert b'max_iters' in lib.cotr_raster_last_error()
    assert lib.cotr_ransac_fundamental_scratch_bytes(100, 1000, ctypes.byref(b)) == 0 and b.value > 0
    need = b.value

    def call(n=100, thr=3.0, conf=0.99, iters=1000, pts=P, scratch=P, nbytes=need):
        return lib.cotr_ransac_fundamental(pts, P, n, thr, conf, iters, 0, P, P, P, None, None, None, scratch, nbytes, None)
    for kw, word in ((dict(n=14), b'LMedS'), (dict(iters=0), b'max_iters'), (dict(thr=0.0), b'threshold'),
                     (dict(thr=float('nan')), b'threshold'), (dict(thr=float('inf')), b'threshold'),
                     (dict(conf=0.0), b'confidence'), (dict(conf=1.0), b'confidence'), (dict(pts=None), b'NULL'),
                     (dict(scratch=ctypes.c_void_p(4104)), b'aligned'), (dict(nbytes=need - 1), b'smaller')):
        assert call(**kw) == -1, kw
        assert word in lib.cotr_raster_last_error(), (kw, lib.cotr_raster_last_error())


# ---- the Python wrappers ------------------------------------------------------------------------------------------------
def test_wrapper_argument_errors_without_a_gpu():
    z = np.zeros((14, 2))
    with pytest.raises(ValueError, match='LMedS'):
        find_fundamental_mat(z, z)
    with pytest.raises(ValueError, match='same length'):
        find_fundamental_mat(np.zeros((20, 2)), np.zeros((21, 2)))
    with pytest.raises(ValueError, match=r'\[N, 2\]'):
        find_fundamental_mat(np.zeros((20, 3)), np.zeros((20, 3)))
    with pytest.raises(ValueError, match='max_iters'):
        find_fundamental_mat(np.zeros((20, 2)), np.zeros((20, 2)), max_iters=0)
    with pytest.raises(ValueError, match='threshold'):
        find_fundamental_mat(np.zeros((20, 2)), np.zeros((20, 2)), 0.0)
    with pytest.raises(ValueError, match='confidence'):
        find_fundamental_mat(np.zeros((20, 2)), np.zeros((20, 2)), 3.0, 1.0)
    with pytest.raises(ValueError, match=r'\[N, 4\]'):
        mutual_matches(np.zeros((5, 2)), np.zeros((5, 4)), np.zeros((5, 2)), np.zeros((5, 2)))
    with pytest.raises(ValueError, match='one row per'):
        mutual_matches(np.zeros((5, 4)), np.zeros((6, 4)), np.zeros((4, 2)), np.zeros((6, 2)))
    with pytest.raises(ValueError, match='at least one'):
        mutual_matches(np.zeros((0, 4)), np.zeros((3, 4)), np.zeros((0, 2)), np.zeros((3, 2)))


@pytest.fixture
def oracle_device(monkeypatch):
    """the two device calls answered by the restatement, on the host"""
    def nearest_mutual(pred_ab, kp_b, pred_ba, kp_a, device=None):
        ia = go.nearest(np.asarray(pred_ab, np.float64), np.asarray(kp_b, np.float64))
        ib = go.nearest(np.asarray(pred_ba, np.float64), np.asarray(kp_a, np.float64))
        return torch.from_numpy(ia.astype(np.int32)), torch.from_numpy(ib.astype(np.int32)), torch.from_numpy(go.mutual(ia, ib))

    def ransac_fundamental(points1, points2, threshold=3.0, confidence=0.99, max_iters=1000, seed=0, hypotheses=False, device=None):
        if len(points1) < 15:
            raise ValueError('needs at least 15 correspondences (LMedS fallback not provided)')
        r = go.ransac(np.asarray(points1), np.asarray(points2), threshold, confidence, max_iters, seed)
        return dict(F=torch.from_numpy(r['F'].reshape(3, 3)), mask=torch.from_numpy(r['mask']),
                    info=torch.from_numpy(r['info'].astype(np.int32)))
    monkeypatch.setattr(guided, 'nearest_mutual', nearest_mutual)
    monkeypatch.setattr(guided, 'ransac_fundamental', ransac_fundamental)


def _demo(corrs_a_b, corrs_b_a, kp_a, kp_b):
    """demo_guided_matching.py:48-65 with scipy -> the restatement's distances and cv2 -> the restatement's RANSAC"""
    inds_a_b = np.argmin(go.distances(corrs_a_b[:, 2:], kp_b), axis=1)
    inds_b_a = np.argmin(go.distances(corrs_b_a[:, 2:], kp_a), axis=1)
    final_matches = go.demo_double_loop(inds_a_b, inds_b_a)
    final_corrs = np.concatenate([kp_a[final_matches[:, 0]], kp_b[final_matches[:, 1]]], axis=1)
    r = go.ransac(final_corrs[:, :2], final_corrs[:, 2:], 5, 0.999999, 1000, 0)
    mask = r['mask'].astype(np.uint8).reshape(-1, 1)
    return final_corrs[np.where(mask[:, 0])]


def _inputs(n, seed):
    p1, p2, _, _ = go.two_view_scene(n, 0.3, seed)
    rng = np.random.default_rng(seed)
    kp_a, kp_b = p1.astype(np.float32), p2.astype(np.float32)
    corrs_a_b = np.concatenate([kp_a, kp_b + rng.normal(0, 0.7, (n, 2))], axis=1)
    corrs_b_a = np.concatenate([kp_b, kp_a + rng.normal(0, 0.7, (n, 2))], axis=1)
    return corrs_a_b, corrs_b_a, kp_a, kp_b


def test_filter_guided_matches_host_logic(oracle_device):
    corrs_a_b, corrs_b_a, kp_a, kp_b = _inputs(120, 0)
    got = filter_guided_matches(corrs_a_b, corrs_b_a, kp_a, kp_b)
    want = _demo(corrs_a_b, corrs_b_a, kp_a, kp_b)
    assert got.dtype == np.float32 and got.shape[1] == 4 and len(got) > 15
    assert np.array_equal(got, want)
    assert np.array_equal(mutual_matches(corrs_a_b, corrs_b_a, kp_a, kp_b),
                          go.demo_double_loop(go.nearest(corrs_a_b[:, 2:], kp_b), go.nearest(corrs_b_a[:, 2:], kp_a)))
    # float64 keypoints: the rows follow numpy's promotion
    assert filter_guided_matches(corrs_a_b, corrs_b_a, kp_a.astype(np.float64), kp_b).dtype == np.float64


def test_filter_guided_matches_below_15_mutual_matches(oracle_device):
    corrs_a_b, corrs_b_a, kp_a, kp_b = _inputs(12, 1)
    with pytest.raises(ValueError, match='LMedS'):
        filter_guided_matches(corrs_a_b, corrs_b_a, kp_a, kp_b)


def test_guided_match_runs_the_demos_two_calls(oracle_device):
    corrs_a_b, corrs_b_a, kp_a, kp_b = _inputs(60, 2)
    calls = []

    class Spy(ZoomEngine):
        def __init__(self):
            pass

        def cotr_corr_multiscale(self, img_a, img_b, zoom_ins=(1.0,), converge_iters=1, max_corrs=1000, queries_a=None, **kw):
            calls.append((img_a, img_b, tuple(zoom_ins), converge_iters, max_corrs, queries_a.shape, kw))
            return corrs_a_b if img_a == 'a' else corrs_b_a
    got = Spy().guided_match('a', 'b', kp_a, kp_b)
    zooms = tuple(np.linspace(0.5, 0.0625, 4))
    assert calls == [('a', 'b', zooms, 1, 60, (60, 2), {'force': True}), ('b', 'a', zooms, 1, 60, (60, 2), {'force': True})]
    assert np.array_equal(got, _demo(corrs_a_b, corrs_b_a, kp_a, kp_b))
