"""Guided matching on the MI355X (cotr_amd/csrc/guided.hip) against the numpy restatement tests/guided_oracle.py:
nearest indices bit-identical to numpy's argmin over scipy's distances, the mutual rule equal to the demo's double loop, and
every stage of the RANSAC (samples, candidates, counts, selection, mask) against the same rule."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import cotr_amd
from cotr_amd import _lib
from cotr_amd.inference import ZoomEngine, SparseEngine, FasterSparseEngine, filter_guided_matches, find_fundamental_mat, \
    mutual_matches
from cotr_amd.inference.guided import nearest_mutual, ransac_fundamental
from tests import guided_oracle as go

pytestmark = pytest.mark.gpu


def dev_nearest(pred_ab, kp_b, pred_ba, kp_a):
    idx_ab, idx_ba, mutual = nearest_mutual(pred_ab, kp_b, pred_ba, kp_a)
    torch.cuda.synchronize()
    return idx_ab.cpu().numpy(), idx_ba.cpu().numpy(), mutual.cpu().numpy()


def check_nearest(pred_ab, kp_b, pred_ba, kp_a):
    idx_ab, idx_ba, mutual = dev_nearest(pred_ab, kp_b, pred_ba, kp_a)
    ref_ab, ref_ba = go.nearest(pred_ab, kp_b), go.nearest(pred_ba, kp_a)
    assert np.array_equal(idx_ab, ref_ab), f'{int((idx_ab != ref_ab).sum())} of {len(ref_ab)} a->b indices differ'
    assert np.array_equal(idx_ba, ref_ba), f'{int((idx_ba != ref_ba).sum())} of {len(ref_ba)} b->a indices differ'
    assert np.array_equal(mutual, go.mutual(ref_ab, ref_ba))
    return idx_ab, idx_ba, mutual


# ---- nearest keypoint ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('na,nb', [(1, 1), (1, 7), (7, 1), (7, 7), (2048, 2048), (8192, 8192), (300, 4100), (4100, 65),
                                   (257, 1023), (5000, 3)])
def test_nearest_random(na, nb):
    rng = np.random.default_rng(na * 7 + nb)
    kp_a, kp_b = rng.uniform(0, 1000, (na, 2)), rng.uniform(0, 1000, (nb, 2))
    pred_ab, pred_ba = rng.uniform(-20, 1020, (na, 2)), rng.uniform(-20, 1020, (nb, 2))
    check_nearest(pred_ab, kp_b, pred_ba, kp_a)


@pytest.mark.parametrize('na,nb', [(64, 64), (1000, 700), (3000, 5000)])
def test_nearest_integer_grid_ties_and_duplicates(na, nb):
    # keypoints on a small integer grid (many duplicates), queries on the grid and at half-integer positions: exact ties
    # between several keypoints, resolved to the lowest index
    rng = np.random.default_rng(na + nb)
    kp_a = rng.integers(0, 12, (na, 2)).astype(np.float64)
    kp_b = rng.integers(0, 12, (nb, 2)).astype(np.float64)
    pred_ab = rng.integers(-2, 26, (na, 2)) / 2.0
    pred_ba = rng.integers(-2, 26, (nb, 2)) / 2.0
    d = go.distances(pred_ab, kp_b)
    assert ((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).mean() > 0.3      # many queries have ties
    check_nearest(pred_ab, kp_b, pred_ba, kp_a)


def _shared_sqrt_cases(m, seed):
    """m queries, each with two keypoints (2i, 2i+1) whose squared distances differ while their float64 square roots are
    equal, the later keypoint having the smaller square: a comparison on d^2 picks 2i+1, numpy's rule on d picks 2i"""
    rng = np.random.default_rng(seed)
    q, k = [], []
    while len(q) < m:
        qi = np.array([1e5 * len(q) + rng.uniform(0, 1), rng.uniform(0, 1)])
        lo = qi + rng.uniform(300, 900, 2)
        d2lo = (lo[0] - qi[0]) ** 2 + (lo[1] - qi[1]) ** 2
        for steps in range(1, 40):
            hi = lo.copy()
            for _ in range(steps):          # (along y: its ulp does not grow with the case's x offset)
                hi[1] = np.nextafter(hi[1], qi[1])
            d2hi = (hi[0] - qi[0]) ** 2 + (hi[1] - qi[1]) ** 2
            if d2hi < d2lo and np.sqrt(d2hi) == np.sqrt(d2lo):
                q.append(qi)
                k += [lo, hi]
                break
    return np.array(q), np.array(k)


def test_nearest_distinct_squares_with_one_sqrt():
    q, k = _shared_sqrt_cases(256, 5)
    d = go.distances(q, k)
    d2 = d * d
    assert (np.argmin(d, axis=1) == 2 * np.arange(len(q))).all()
    dx = k[None, :, 0] - q[:, None, 0]
    dy = k[None, :, 1] - q[:, None, 1]
    assert (np.argmin(dx * dx + dy * dy, axis=1) == 2 * np.arange(len(q)) + 1).all()   # a rule on d^2 would differ
    del d2
    idx_ab, _, _ = check_nearest(q, k, k, q)
    assert (idx_ab == 2 * np.arange(len(q))).all()


def _hard_sqrt_cases(m, seed):
    """(dx, dy) whose d^2 = dx*dx + dy*dy has an exact square root within 0.1 ulp of the midpoint between two doubles:
    a sqrt that is not correctly rounded gets some of them wrong"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < m:
        dx, dy = rng.uniform(1, 1000, 2)
        d2 = dx * dx + dy * dy
        s = np.sqrt(d2)
        ulp = np.spacing(s)
        frac = (Fraction(float(d2)) - Fraction(float(s)) ** 2) / (2 * Fraction(float(s)) * Fraction(float(ulp)))
        if abs(frac) > 0.4:
            out.append((dx, dy, s))
    return out


def test_nearest_sqrt_is_correctly_rounded():
    # query at the origin; keypoint H at a hard distance and keypoint C = (s, 0) at exactly the correctly rounded s.
    # [C, H]: the tie goes to C unless the device rounds H's distance down; [H, C]: to H unless it rounds it up.
    origin = np.zeros((1, 2))
    wrong = 0
    for dx, dy, s in _hard_sqrt_cases(200, 9):
        for kp, want in ((np.array([[s, 0.0], [dx, dy]]), 0), (np.array([[dx, dy], [s, 0.0]]), 0)):
            assert go.nearest(origin, kp)[0] == want
            idx_ab, _, _ = dev_nearest(origin, kp, kp, origin)
            wrong += int(idx_ab[0] != want)
    assert wrong == 0, f'{wrong} of 400 hard square roots rounded differently from IEEE sqrt'


def test_nearest_nan_and_inf_follow_numpy():
    rng = np.random.default_rng(3)
    kp_a, kp_b = rng.uniform(0, 100, (50, 2)), rng.uniform(0, 100, (70, 2))
    pred_ab, pred_ba = rng.uniform(0, 100, (50, 2)), rng.uniform(0, 100, (70, 2))
    kp_b[[5, 9]] = np.nan
    kp_b[11] = np.inf
    pred_ab[3] = np.nan
    pred_ba[4] = [1e308, -1e308]
    check_nearest(pred_ab, kp_b, pred_ba, kp_a)


def _disk():
    import os
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    return (np.load(os.path.join(g, '21526113_4379776807.jpg.disk.kpts.npy')),
            np.load(os.path.join(g, '21126421_4537535153.jpg.disk.kpts.npy')))


def test_nearest_on_the_reference_disk_keypoints():
    kp_a, kp_b = _disk()
    rng = np.random.default_rng(0)
    # predictions: the other image's keypoints moved a little, some exactly on a keypoint, some far off
    pred_ab = kp_b[rng.permutation(len(kp_b))[:len(kp_a)]].astype(np.float64) + rng.normal(0, 2, (len(kp_a), 2))
    pred_ba = kp_a[rng.permutation(len(kp_a))[:len(kp_b)]].astype(np.float64) + rng.normal(0, 2, (len(kp_b), 2))
    pred_ab[::7] = kp_b[rng.integers(0, len(kp_b), len(pred_ab[::7]))]
    pred_ba[::5] = rng.uniform(-500, 1500, pred_ba[::5].shape)
    check_nearest(pred_ab, kp_b.astype(np.float64), pred_ba, kp_a.astype(np.float64))
    # float32 keypoints are widened exactly by the wrapper
    i32 = dev_nearest(pred_ab, kp_b, pred_ba, kp_a)
    i64 = dev_nearest(pred_ab, kp_b.astype(np.float64), pred_ba, kp_a.astype(np.float64))
    assert all(np.array_equal(x, y) for x, y in zip(i32, i64))


@pytest.mark.parametrize('na,nb,grid', [(40, 60, True), (300, 250, False), (200, 200, True)])
def test_mutual_matches_equal_the_demo_loop(na, nb, grid):
    rng = np.random.default_rng(na + nb)
    if grid:   # duplicates and ties
        kp_a = rng.integers(0, 15, (na, 2)).astype(np.float32)
        kp_b = rng.integers(0, 15, (nb, 2)).astype(np.float32)
    else:
        kp_a, kp_b = rng.uniform(0, 640, (na, 2)).astype(np.float32), rng.uniform(0, 480, (nb, 2)).astype(np.float32)
    corrs_a_b = np.concatenate([kp_a, kp_b[rng.integers(0, nb, na)] + rng.normal(0, 1, (na, 2))], axis=1)
    corrs_b_a = np.concatenate([kp_b, kp_a[rng.integers(0, na, nb)] + rng.normal(0, 1, (nb, 2))], axis=1)
    for j in range(0, min(na, nb), 2):      # make some pairs agree both ways
        corrs_b_a[j, 2:] = kp_a[j]
        corrs_a_b[j, 2:] = kp_b[j]
    got = mutual_matches(corrs_a_b, corrs_b_a, kp_a, kp_b)
    ref = go.demo_double_loop(go.nearest(corrs_a_b[:, 2:], kp_b), go.nearest(corrs_b_a[:, 2:], kp_a))
    assert got.dtype == np.int64 and np.array_equal(got, ref) and len(ref) > 0


# ---- RANSAC -----------------------------------------------------------------------------------------------------------
def dev_ransac(p1, p2, thr, conf, iters, seed):
    r = ransac_fundamental(p1, p2, thr, conf, iters, seed, hypotheses=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _rel(a, b):
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return min(np.abs(a - b).max(), np.abs(a + b).max())


@pytest.mark.parametrize('n,iters,seed', [(15, 300, 0), (100, 1000, 1), (2048, 500, (1 << 63) + 5)])
def test_ransac_samples_are_the_oracles(n, iters, seed):
    rng = np.random.default_rng(n)
    p1, p2 = rng.uniform(0, 640, (n, 2)), rng.uniform(0, 480, (n, 2))
    r = dev_ransac(p1, p2, 3.0, 0.99, iters, seed)
    assert np.array_equal(r['samples'], go.samples(n, iters, seed))


SCENES = [(300, 0.3, 1.0, 0.99, 1000, 0), (500, 0.45, 3.0, 0.999999, 2000, 1), (2048, 0.5, 5.0, 0.99, 1000, 2),
          (200, 0.6, 2.0, 0.999, 3000, 3), (64, 0.3, 4.0, 0.99, 500, 4)]


@pytest.mark.parametrize('n,outl,thr,conf,iters,seed', SCENES)
def test_ransac_every_stage_against_the_oracle(n, outl, thr, conf, iters, seed):
    p1, p2, true_in, _ = go.two_view_scene(n, outl, seed)
    r = dev_ransac(p1, p2, thr, conf, iters, seed)
    smp = go.samples(n, iters, seed)
    assert np.array_equal(r['samples'], smp)
    # candidates: per iteration the same set within 1e-7; iterations whose root count differs (a near-double root of the
    # cubic) or that do not match are counted, and must be rare
    H = go.candidates(p1, p2, smp)
    dev_H = r['hyp_F']
    bad = 0
    for it in range(iters):
        mine = [f for f in dev_H[3 * it:3 * it + 3] if not np.isnan(f).all()]
        ref = [f for f in H[3 * it:3 * it + 3] if not np.isnan(f).all()]
        if len(mine) != len(ref) or any(min(_rel(m, f) for f in ref) > 1e-7 for m in mine):
            bad += 1
    assert bad <= max(2, iters // 100), f'{bad} of {iters} iterations differ from the oracle'
    # counts recomputed in numpy from the device's own candidates: exact
    cnt = go.counts(dev_H, p1, p2, thr)
    assert np.array_equal(r['hyp_count'], cnt)
    assert np.array_equal(np.isnan(dev_H).all(axis=1), cnt < 0)
    # the selection: the sequential loop's answer on the device's counts
    info = tuple(int(v) for v in r['info'])
    assert info == go.select(cnt, iters, n, conf) == go.select_sequential(cnt, iters, n, conf)
    found, best, runs, slot = info
    assert found and best >= 7
    assert np.array_equal(r['F'].reshape(9), dev_H[slot])
    mask = r['mask']
    assert mask.sum() == best and np.array_equal(mask, go.inliers(dev_H[slot], p1, p2, thr)[0])
    # the true inliers: the mask is the thresholded error of F (borderline points aside) and finds the scene's inliers
    err = go.errors(dev_H[slot], p1, p2)[0].astype(np.float64)
    t2 = np.float32(thr * thr)
    clear = np.abs(err - t2) > 1e-6 * t2
    assert np.array_equal(mask[clear], (err <= t2)[clear])
    tp = (mask & true_in).sum()
    assert tp / mask.sum() >= 0.85, (tp, mask.sum())
    assert tp / true_in.sum() >= 0.3, (tp, true_in.sum())


@pytest.mark.parametrize('n,outl,thr,conf,iters,seed', go.EDGES)
def test_ransac_wavefront_chunk_and_workgroup_edges(n, outl, thr, conf, iters, seed):
    """the shared count and mask kernels on the fundamental model past one wavefront, one 2048-point chunk and one solve
    workgroup: every stage exact against the restatement on the device's own candidates"""
    p1, p2, _, _ = go.two_view_scene(n, outl, seed)
    r = dev_ransac(p1, p2, thr, conf, iters, seed)
    assert np.array_equal(r['samples'], go.samples(n, iters, seed))
    dev_H = r['hyp_F']
    cnt = go.counts(dev_H, p1, p2, thr)
    assert np.array_equal(r['hyp_count'], cnt)
    info = tuple(int(v) for v in r['info'])
    assert info == go.select(cnt, iters, n, conf) == go.select_sequential(cnt, iters, n, conf)
    found, best, runs, slot = info
    assert np.array_equal(r['F'].reshape(9), dev_H[slot] if found else np.zeros(9))
    want = go.inliers(dev_H[slot], p1, p2, thr)[0] if found else np.zeros(n, bool)
    assert np.array_equal(r['mask'], want) and r['mask'].sum() == best


def test_ransac_deterministic_across_calls_streams_and_scratch():
    p1, p2, _, _ = go.two_view_scene(1000, 0.4, 7)
    first = dev_ransac(p1, p2, 2.0, 0.999, 1500, 11)
    again = dev_ransac(p1, p2, 2.0, 0.999, 1500, 11)
    for k in first:
        assert np.array_equal(first[k], again[k], equal_nan=True), k
    # the C ABI directly: a side stream, a larger caller scratch full of garbage, no hypothesis tables
    lib = _lib.load_library()
    n, iters = len(p1), 1500
    nbytes = ctypes.c_size_t()
    assert lib.cotr_ransac_fundamental_scratch_bytes(n, iters, ctypes.byref(nbytes)) == 0
    scratch = torch.full((nbytes.value + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
    d1 = torch.from_numpy(p1).cuda()
    d2 = torch.from_numpy(p2).cuda()
    F = torch.empty(9, dtype=torch.float64, device='cuda')
    mask = torch.empty(n, dtype=torch.uint8, device='cuda')
    info = torch.empty(4, dtype=torch.int32, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    rc = lib.cotr_ransac_fundamental(p(d1), p(d2), n, 2.0, 0.999, iters, 11, p(F), p(mask), p(info), None, None, None,
                                     p(scratch), nbytes.value + 4096, ctypes.c_void_p(side.cuda_stream))
    assert rc == 0, lib.cotr_raster_last_error()
    side.synchronize()
    assert np.array_equal(F.cpu().numpy(), first['F'].reshape(9))
    assert np.array_equal(mask.cpu().numpy().astype(bool), first['mask'])
    assert np.array_equal(info.cpu().numpy(), first['info'])


def test_find_fundamental_mat_shapes_and_nothing_found():
    p1, p2, _, _ = go.two_view_scene(200, 0.3, 12)
    F, mask = find_fundamental_mat(p1, p2, 3.0, 0.99)
    assert F.shape == (3, 3) and F.dtype == np.float64 and mask.shape == (200, 1) and mask.dtype == np.uint8
    # 15 points, a threshold whose float32 square is 0: no candidate has 7 inliers, nothing is found
    rng = np.random.default_rng(1)
    q1, q2 = rng.uniform(0, 640, (15, 2)), rng.uniform(0, 480, (15, 2))
    r = dev_ransac(q1, q2, 1e-30, 0.99, 50, 0)
    assert not r['info'][0]
    assert find_fundamental_mat(q1, q2, 1e-30, 0.99, 50) == (None, None)
    assert (r['mask'] == 0).all() and (r['F'] == 0).all() and r['info'][3] == -1 and r['info'][2] == 50
    assert tuple(int(v) for v in r['info']) == go.select(r['hyp_count'], 50, 15, 0.99)


def _guided_inputs(n, seed):
    p1, p2, _, _ = go.two_view_scene(n, 0.3, seed)
    rng = np.random.default_rng(seed)
    kp_a = p1.astype(np.float32)
    perm = rng.permutation(n)
    kp_b = p2[perm].astype(np.float32)                    # kp_b[k] is the match of kp_a[perm[k]]
    inv = np.argsort(perm)
    corrs_a_b = np.concatenate([kp_a, kp_b[inv] + rng.normal(0, 0.7, (n, 2))], axis=1)
    corrs_b_a = np.concatenate([kp_b, kp_a[perm] + rng.normal(0, 0.7, (n, 2))], axis=1)
    wrong = rng.random(n) < 0.15
    corrs_a_b[wrong, 2:] = rng.uniform(0, 640, (int(wrong.sum()), 2))
    return corrs_a_b, corrs_b_a, kp_a, kp_b


@pytest.mark.parametrize('n,seed', [(300, 0), (150, 1)])
def test_filter_guided_matches_equals_the_demo_with_the_oracle(n, seed):
    corrs_a_b, corrs_b_a, kp_a, kp_b = _guided_inputs(n, seed)
    got = filter_guided_matches(corrs_a_b, corrs_b_a, kp_a, kp_b)
    # the demo's lines, scipy + the double loop + cv2 replaced by the restatement
    final_matches = go.demo_double_loop(go.nearest(corrs_a_b[:, 2:], kp_b), go.nearest(corrs_b_a[:, 2:], kp_a))
    final_corrs = np.concatenate([kp_a[final_matches[:, 0]], kp_b[final_matches[:, 1]]], axis=1)
    ref = go.ransac(final_corrs[:, :2], final_corrs[:, 2:], 5.0, 0.999999, 1000, 0)
    mask = ref['mask'].astype(np.uint8).reshape(-1, 1)
    want = final_corrs[np.where(mask[:, 0])]
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(got, want)


def test_guided_match_on_the_hip_model():
    from cotr_amd.models import build_model
    from cotr_amd.utils.synth import synth_state_dict
    from tests.engine_fixtures import synthetic_pair
    sd = synth_state_dict(0)
    hip = build_model(cotr_amd.default_args()).cuda().eval()
    hip.load_state_dict(sd)
    img_a, img_b = synthetic_pair(3)
    rng = np.random.default_rng(4)
    kp_a = np.stack([rng.uniform(5, img_a.shape[1] - 5, 40), rng.uniform(5, img_a.shape[0] - 5, 40)], 1).astype(np.float32)
    kp_b = np.stack([rng.uniform(5, img_b.shape[1] - 5, 36), rng.uniform(5, img_b.shape[0] - 5, 36)], 1).astype(np.float32)
    eng = ZoomEngine(hip)
    assert SparseEngine.guided_match is ZoomEngine.guided_match and FasterSparseEngine.guided_match is ZoomEngine.guided_match
    zooms = np.linspace(0.5, 0.0625, 4)
    with torch.no_grad():
        ab = eng.cotr_corr_multiscale(img_a, img_b, zooms, 1, max_corrs=len(kp_a), queries_a=kp_a, force=True)
        ba = eng.cotr_corr_multiscale(img_b, img_a, zooms, 1, max_corrs=len(kp_b), queries_a=kp_b, force=True)
        assert ab.shape == (40, 4) and ba.shape == (36, 4)
        try:
            want = filter_guided_matches(ab, ba, kp_a, kp_b, ransac_threshold=5.0)
        except ValueError as e:
            with pytest.raises(ValueError) as got:
                eng.guided_match(img_a, img_b, kp_a, kp_b)
            assert str(got.value) == str(e)
            assert len(mutual_matches(ab, ba, kp_a, kp_b)) < 15
            return
        got = eng.guided_match(img_a, img_b, kp_a, kp_b)
    assert np.array_equal(got, want)
