"""The homography estimator on the MI355X (cotr_amd/csrc/homography.hip) against the numpy restatement
tests/homography_oracle.py: every stage of the RANSAC (samples, candidates, counts, selection, mask) against the same rule,
the refit on the device's own mask against the restatement's, repeatability, and the paste built on it.

The refit bound: the device differs from the restatement by the order of its sums and by last-bit differences of the Jacobi
rotations.  The restatement's own dependence on the summation order (sums reversed and shuffled), measured on the CPU over
the scenes used here, is at most 6.24e-10 px at the corners of the points' bounding box (ho.ORDER_NOISE_PX); 1000 times that
is allowed, 6.3e-7 px (ho.REFIT_BOUND_PX), below 1e-6 px and far below the 3e-5 px of the float32 input rounding.  Measured
on an MI355X over these scenes: at most 2.45e-08 px (n = 63, where the device kept 4 Gauss-Newton steps and the restatement
2), 1.5e-11 px for the DLT alone."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from cotr_amd.inference import find_homography, paste_by_corners, paste_by_homography, ransac_homography
from cotr_amd.inference.warp import picture_corners
from tests import homography_oracle as ho

pytestmark = pytest.mark.gpu


def dev_ransac(p1, p2, thr=3.0, conf=0.995, iters=2000, seed=0, refine_iters=10, hypotheses=True):
    r = ransac_homography(p1, p2, thr, conf, iters, seed, refine_iters, hypotheses=hypotheses)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _rel(a, b):
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return min(np.abs(a - b).max(), np.abs(a + b).max())


@pytest.mark.parametrize('n,iters,seed', [(4, 65, 0), (5, 64, 2), (100, 1000, 1), (2049, 63, (1 << 63) + 5)])
def test_samples_are_the_oracles(n, iters, seed):
    rng = np.random.default_rng(n)
    p1, p2 = rng.uniform(0, 640, (n, 2)), rng.uniform(0, 480, (n, 2))
    r = dev_ransac(p1, p2, iters=iters, seed=seed)
    assert np.array_equal(r['samples'], ho.samples(n, iters, seed))


def check_every_stage(scene):
    n, outl, noise, thr, conf, iters, seed = scene
    p1, p2, _, Ht = ho.planar_scene(n, outl, seed, noise)
    r = dev_ransac(p1, p2, thr, conf, iters, seed)
    smp = ho.samples(n, iters, seed)
    assert np.array_equal(r['samples'], smp)
    # candidates: model or no model per iteration, and the same model within 1e-7
    (ref_H, ref_has), dev_H = ho.candidates(p1, p2, smp), r['hyp_H']
    na, nb = r['hyp_count'] < 0, ~ref_has                                        # no model: the device's flag, the oracle's
    assert np.array_equal(np.isnan(dev_H).all(axis=1), na) and np.isfinite(dev_H[~na]).all()
    bad = sum(1 for i in range(iters) if na[i] != nb[i] or (not na[i] and _rel(dev_H[i], ref_H[i]) > 1e-7))
    worst = max([_rel(dev_H[i], ref_H[i]) for i in range(iters) if not na[i] and not nb[i]] or [0.0])
    print(f'n={n} iters={iters}: {bad} iterations differ, worst agreement {worst:.2e}, no model on {na.mean():.2f}')
    assert bad <= max(2, iters // 100), f'{bad} of {iters} iterations differ from the oracle'
    # counts recomputed in numpy from the device's own candidates: exact
    cnt = ho.counts(dev_H, ~na, p1, p2, thr)
    assert np.array_equal(r['hyp_count'], cnt)
    # the selection: the sequential loop's answer on the device's counts
    info = [int(v) for v in r['info']]
    assert tuple(info[:4]) == ho.select(cnt, iters, n, conf) == ho.select_sequential(cnt, iters, n, conf)
    found, best, runs, slot, kept, status = info[:6]
    assert found and best >= 4 and info[6:] == [0, 0]
    assert np.array_equal(r['H_ransac'].reshape(9), dev_H[slot])                  # the chosen slot, bit for bit
    mask = r['mask']
    assert mask.sum() == best and np.array_equal(mask, ho.inliers(dev_H[slot], p1, p2, thr)[0])
    # the refit: the restatement on the device's mask
    H = r['H'].reshape(9)
    ref, ref_kept, ref_status, ref_dlt = ho.refit(p1, p2, mask, 10, dev_H[slot])
    d = ho.corner_error(H, ref, p1)
    print(f'  refit: device - oracle {d:.2e} px (bound {ho.REFIT_BOUND_PX:.1e}), kept {kept} / oracle {ref_kept}, status {status}')
    assert status == ref_status == 0 and 0 <= kept <= 10
    assert d <= ho.REFIT_BOUND_PX
    # refine_iters = 0 gives the DLT result; refining never raises the squared error on the inliers
    r0 = dev_ransac(p1, p2, thr, conf, iters, seed, refine_iters=0, hypotheses=False)
    assert np.array_equal(r0['mask'], mask) and np.array_equal(r0['H_ransac'], r['H_ransac'])
    assert list(r0['info'][:4]) == info[:4] and r0['info'][4] == 0 and r0['info'][5] == 1
    d0 = ho.corner_error(r0['H'], ref_dlt, p1)
    print(f'  DLT: device - oracle {d0:.2e} px')
    assert d0 <= ho.REFIT_BOUND_PX
    e_ref, e_dlt = ho.sq_error(H, p1, p2, mask), ho.sq_error(r0['H'], p1, p2, mask)
    assert e_ref <= e_dlt, (e_ref, e_dlt)
    return r, ref, Ht, p1


@pytest.mark.parametrize('scene', ho.SCENES, ids=lambda s: f'n{s[0]}-it{s[5]}')
def test_every_stage_against_the_oracle(scene):
    r, ref, Ht, p1 = check_every_stage(scene)
    # against the scene's true H: no worse than the restatement, and better than the best 4-point sample
    c_dev, c_ref, c_ransac = (ho.corner_error(h, Ht, p1) for h in (r['H'], ref, r['H_ransac']))
    print(f'  corner error: H_ransac {c_ransac:.3f} px, refit {c_dev:.3f} px, oracle refit {c_ref:.3f} px')
    assert c_dev <= c_ref + ho.REFIT_BOUND_PX
    assert c_dev < c_ransac


@pytest.mark.parametrize('scene', ho.EDGES, ids=lambda s: f'n{s[0]}-it{s[5]}')
def test_wavefront_chunk_and_workgroup_edges(scene):
    check_every_stage(scene)


def test_collinear_points_find_nothing():
    x = 2.0 * np.arange(300)                                    # exact in float32: the cross products are exactly 0
    p = np.stack([x, 0.5 * x + 7], 1)
    r = dev_ransac(p, p + 3, iters=200)
    assert list(r['info']) == [0, 0, 200, -1, 0, 2, 0, 0]
    assert (r['H'] == 0).all() and (r['H_ransac'] == 0).all() and not r['mask'].any()
    assert (r['hyp_count'] == -1).all() and np.isnan(r['hyp_H']).all()
    assert find_homography(p, p + 3, max_iters=200) == (None, None)
    q = np.array([[0, 0], [10, 10], [20, 20], [5, 30]], np.float64)      # n = 4, three on a line
    r = dev_ransac(q, q, iters=65)
    assert list(r['info']) == [0, 0, 65, -1, 0, 2, 0, 0]
    assert (r['H'] == 0).all() and not r['mask'].any() and (r['hyp_count'] == -1).all()


def test_find_homography_shapes():
    n, outl, noise, thr, conf, iters, seed = ho.SCENES[1]
    p1, p2, _, _ = ho.planar_scene(n, outl, seed, noise)
    H, mask = find_homography(p1.astype(np.float32), p2.astype(np.float32), thr, iters, conf, seed)
    assert H.shape == (3, 3) and H.dtype == np.float64 and H[2, 2] == 1.0 and mask.shape == (n, 1) and mask.dtype == np.uint8
    r = dev_ransac(p1, p2, thr, conf, iters, seed)
    assert np.array_equal(H, r['H']) and np.array_equal(mask[:, 0].astype(bool), r['mask'])
    # device tensors stay on the device
    t = ransac_homography(torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda(), thr, conf, iters, seed)
    assert all(v.is_cuda for v in t.values()) and np.array_equal(t['H'].cpu().numpy(), r['H'])


def test_same_bits_across_calls_streams_scratch_and_graph_replay():
    n, outl, noise, thr, conf, iters, seed = 3000, 0.4, 1.0, 3.0, 0.995, 300, 5
    p1, p2, _, _ = ho.planar_scene(n, outl, seed, noise)
    first = dev_ransac(p1, p2, thr, conf, iters, seed)
    again = dev_ransac(p1, p2, thr, conf, iters, seed)
    assert first['info'][0] and first['info'][5] == 0
    for k in first:
        assert np.array_equal(first[k], again[k], equal_nan=True), k
    # the C ABI directly: a side stream, a larger caller scratch full of garbage, no optional outputs
    lib = _lib.load_library()
    nbytes = ctypes.c_size_t()
    assert lib.cotr_ransac_homography_scratch_bytes(n, iters, ctypes.byref(nbytes)) == 0
    d1, d2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def buffers():
        return (torch.full((nbytes.value + 4096,), 0xA5, dtype=torch.uint8, device='cuda'),
                torch.full((9,), -7.0, dtype=torch.float64, device='cuda'), torch.full((n,), 9, dtype=torch.uint8, device='cuda'),
                torch.full((8,), -3, dtype=torch.int32, device='cuda'))

    def same(H, mask, info):
        assert np.array_equal(H.cpu().numpy(), first['H'].reshape(9))
        assert np.array_equal(mask.cpu().numpy().astype(bool), first['mask'])
        assert np.array_equal(info.cpu().numpy(), first['info'])
    scratch, H, mask, info = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rc = lib.cotr_ransac_homography(p(d1), p(d2), n, thr, conf, iters, 10, seed, p(H), p(mask), p(info), None, None, None, None,
                                    p(scratch), nbytes.value + 4096, ctypes.c_void_p(side.cuda_stream))
    assert rc == 0, lib.cotr_raster_last_error()
    side.synchronize()
    same(H, mask, info)
    # captured once (a single linear chain on the capture stream), replayed once
    scratch, H, mask, info = buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.cotr_ransac_homography(p(d1), p(d2), n, thr, conf, iters, 10, seed, p(H), p(mask), p(info), None, None, None, None,
                                        p(scratch), nbytes.value + 4096, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.cotr_raster_last_error()
    graph.replay()
    torch.cuda.synchronize()
    same(H, mask, info)


def _paste_case():
    from tests.engine_fixtures import synthetic_pair
    picture, img_b = synthetic_pair(0, (120, 160), (240, 320))
    corners_b = np.array([[40.5, 30.25], [250.0, 45.0], [55.0, 200.0], [270.75, 190.5]], np.float32)
    return picture, img_b, corners_b


def test_paste_by_homography_from_the_four_corners_is_paste_by_corners():
    # Four correspondences are mapped exactly, by get_perspective_transform on the host: this checks the wrapper's 4-point
    # path and the shared warp launch, not the estimator.  The estimator on the same exact correspondences is checked below.
    picture, img_b, corners_b = _paste_case()
    got = paste_by_homography(picture, picture_corners(picture.shape), corners_b, img_b)
    assert got.dtype == np.uint8 and np.array_equal(got, paste_by_corners(picture, corners_b, img_b))
    assert np.array_equal(paste_by_homography(picture, picture_corners(picture.shape), corners_b, img_b, seed=3, max_iters=10), got)
    with pytest.raises(TypeError, match='unexpected keyword'):
        paste_by_homography(picture, picture_corners(picture.shape), corners_b, img_b, treshold=3.0)
    with pytest.raises(ValueError, match='max_iters'):
        paste_by_homography(picture, picture_corners(picture.shape), corners_b, img_b, max_iters=0)


def test_exact_correspondences_give_the_perspective_transform():
    # the four corners and three points inside, mapped exactly in float64 and rounded to float32 (0.5 ulp of 320 px: 1.5e-5 px
    # each): the estimator's H, through RANSAC and the refit, sends the corners where get_perspective_transform's does within
    # a few times that rounding (1e-4 px allowed; measured 1.4e-6 px, on the device and in the restatement), far below the
    # warp's 1/32 px grid
    from cotr_amd.inference import get_perspective_transform
    picture, img_b, corners_b = _paste_case()
    src4 = picture_corners(picture.shape).astype(np.float64)
    T = get_perspective_transform(src4, corners_b)
    inside = np.array([[80.0, 60.0], [40.0, 90.0], [120.0, 30.0]])
    src = np.concatenate([src4, inside]).astype(np.float32)
    dst = np.concatenate([corners_b, ho.apply(T, inside)]).astype(np.float32)
    r = dev_ransac(src, dst, thr=1.0, iters=100, hypotheses=False)
    assert r['info'][0] and r['info'][1] == 7 and r['mask'].all() and r['info'][5] == 0
    d = ho.corner_error(r['H'], T, src4)
    print(f'estimator against get_perspective_transform on exact correspondences: {d:.2e} px')
    assert d < 1e-4


def test_paste_by_homography_from_noisy_correspondences_with_outliers():
    from cotr_amd.inference import get_perspective_transform
    picture, img_b, corners_b = _paste_case()
    T = get_perspective_transform(picture_corners(picture.shape), corners_b)
    rng = np.random.default_rng(1)
    pp = rng.uniform([0, 0], [160, 120], (200, 2))
    pb = ho.apply(T, pp) + rng.normal(0, 0.3, (200, 2))
    out = rng.random(200) < 0.25
    pb[out] = rng.uniform([0, 0], [320, 240], (int(out.sum()), 2))
    pp, pb = pp.astype(np.float32), pb.astype(np.float32)
    want = paste_by_corners(picture, corners_b, img_b)
    got = paste_by_homography(picture, pp, pb, img_b, seed=4)
    # the share of pixels the restatement's own H changes, plus 0.1 % of the image
    ref = ho.ransac(pp, pb, 3.0, 0.995, 2000, 4)
    assert ref['info'][0]
    from cotr_amd.inference import warp_perspective
    by_oracle = warp_perspective(picture, ref['H'].reshape(3, 3), (320, 240), background=img_b)
    changed = lambda a: float((a != want).any(axis=2).mean())   # noqa: E731
    print(f'pixels changed: device {changed(got):.4f}, oracle {changed(by_oracle):.4f}')
    assert changed(got) <= changed(by_oracle) + 0.001
