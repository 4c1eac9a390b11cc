"""cotr_amd/scene.py on the MI355X against the numpy oracle of tests/scene_oracle.py (which tests/test_scene_cpu.py holds
against the reference's own distance_between_two_caps and get_knn).

The rule: the integer counts (good, union) of every pair are EQUAL and the ratios bit-equal, for every pair without a
candidate within 1e-9 of a decision.  The share of pairs left out may be at most 0: every scene below was chosen on the
CPU so that the oracle finds no such candidate and no world point within round-off of a float32 tie, and each case asserts
it.  Shapes are the smallest at which each mechanism can go wrong; both kernels work in blocks of 256 lanes, so 13 x 20
= 260 pixels is one block and four lanes of the next."""
import numpy as np
import pytest
import torch

from cotr_amd import data, scene
from cotr_amd.data import Capture
from cotr_amd.utils.synth import synth_scene
from tests import scene_oracle as oracle
from tests.test_scene_cpu import GOLDEN, N, golden_scene

pytestmark = pytest.mark.gpu

MAX_LEFT_OUT = 0       # share of a case's pairs with an ambiguous candidate
_scenes = {}


def up(c):
    return Capture(torch.from_numpy(c.image).cuda(), torch.from_numpy(c.depth).cuda(), c.K, c.c2w)


def all_pairs(n):
    return np.argwhere(np.ones((n, n), dtype=bool))


def small_scene(key):
    """4 captures (two on the arc, the one that looks away, the one without depth) of the named shape, built once"""
    if key not in _scenes:
        if key == 'mixed_shapes':                        # one world at two resolutions, different poses
            a, b = synth_scene(30, 4, 64, 96), synth_scene(30, 4, 48, 64)
            _scenes[key] = [a[0], b[1], a[2], b[3]]
        else:
            seed, h, w = key
            _scenes[key] = synth_scene(seed, 3 if h * w == 1 else 4, h, w)
    return _scenes[key]


def check_pairs(caps, pairs, **kw):
    """device overlap_pairs against the oracle by the rule of the module docstring -> (ratio, counts) of the device as numpy"""
    pairs = np.asarray(pairs)
    want_ratio, want_counts, ambiguous = oracle.overlap_pairs(caps, pairs)
    assert sum(oracle.float32_ties(caps[d]) for d in set(pairs[:, 1].tolist())) == 0
    ratio, counts = scene.overlap_pairs([up(c) for c in caps], pairs, **kw)
    assert ratio.dtype == torch.float32 and counts.dtype == torch.int32 and ratio.is_cuda and counts.is_cuda
    assert tuple(ratio.shape) == (len(pairs),) and tuple(counts.shape) == (len(pairs), 2)
    ratio, counts = ratio.cpu().numpy(), counts.cpu().numpy()
    clear = ambiguous == 0
    print(f'{len(pairs)} pairs, {int((~clear).sum())} left out; counts differ in {int((counts != want_counts).any(1).sum())}')
    assert (~clear).mean() <= MAX_LEFT_OUT
    assert np.array_equal(counts[clear], want_counts[clear])
    assert np.array_equal(ratio[clear].view(np.uint32), want_ratio[clear].view(np.uint32))
    return ratio, counts


@pytest.mark.parametrize('key', [(30, 1, 1), (33, 2, 3), (30, 17, 23), (30, 64, 96), (30, 13, 20), 'mixed_shapes'],
                         ids=['1x1', '2x3', '17x23', '64x96', '13x20', '64x96_and_48x64'])
def test_every_pair_of_a_small_scene(key):
    """all ordered pairs: the blind and the empty capture as q and as d, the diagonal, at 1 x 1 a union of 0 -> 0.0"""
    caps = small_scene(key)
    n = len(caps)
    ratio, counts = check_pairs(caps, all_pairs(n))
    ratio = ratio.reshape(n, n)
    assert not ratio[n - 2:].any() and not ratio[:, n - 2:].any()
    if key == (30, 1, 1):
        assert not counts.any() and not ratio.any()
    elif key != (33, 2, 3):
        assert (ratio[:n - 2, :n - 2] > 0.3).all()
    if key == 'mixed_shapes':
        assert caps[0].depth.shape == (64, 96) and caps[1].depth.shape == (48, 64)


def test_many_points_on_one_pixel():
    """96 x 128 into 24 x 32 of the same field of view: the last point in source order owns a pixel"""
    caps = golden_scene('mixed')[0]
    want = oracle.overlap(caps[1], caps[0])
    assert want['crowded'] > want['hit'] / 2
    _, counts = check_pairs(caps, [[1, 0], [0, 1]])
    assert counts[0, 0] == want['good'] != oracle.overlap(caps[1], caps[0], canvas_rule='minz')['good']


def test_tiles_repeats_and_two_runs_return_the_same_bytes():
    """16 pairs in tiles of 3 (a ragged last tile) against the untiled call; a list with repeated d and repeated pairs; two
    runs of one call"""
    caps = small_scene((30, 17, 23))
    pairs = all_pairs(4)
    r0, c0 = check_pairs(caps, pairs)
    r1, c1 = check_pairs(caps, pairs, max_pairs_in_flight=3)
    r2, c2 = check_pairs(caps, pairs, max_pairs_in_flight=1)
    r3, c3 = check_pairs(caps, pairs)
    for r, c in ((r1, c1), (r2, c2), (r3, c3)):
        assert r.tobytes() == r0.tobytes() and c.tobytes() == c0.tobytes()
    rep = np.array([[0, 1], [1, 1], [0, 1], [2, 1], [0, 1], [1, 0], [3, 1], [1, 0]])
    r, c = check_pairs(caps, rep, max_pairs_in_flight=3)
    assert c[0].tolist() == c[2].tolist() == c[4].tolist() == c0[1].tolist() and c[5].tolist() == c[7].tolist() == c0[4].tolist()
    dev = scene.overlap_pairs([up(x) for x in caps], torch.from_numpy(np.concatenate([rep, [[0, 9], [-1, 0]]])).cuda())
    assert dev[1].cpu().numpy()[:8].tobytes() == c.tobytes() and not dev[1][8:].any() and not dev[0][8:].any()
    empty = scene.overlap_pairs([up(x) for x in caps], np.zeros((0, 2), dtype=np.int64))
    assert tuple(empty[0].shape) == (0,) and tuple(empty[1].shape) == (0, 2)


@pytest.mark.parametrize('name', ['plain', 'mixed'])
def test_overlap_matrix_and_covisible(name):
    """the matrix of the golden scenes equals what the reference returned; with a covisible mask the masked cells are 0 and
    the others equal the unmasked run"""
    caps, want, ambiguous = golden_scene(name)
    assert ambiguous.sum() == 0
    dcaps = [up(c) for c in caps]
    dist = scene.overlap_matrix(dcaps)
    assert dist.dtype == torch.float32 and tuple(dist.shape) == (N, N) and dist.is_cuda
    dist = dist.cpu().numpy()
    assert np.array_equal(dist.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(dist, GOLDEN[f'{name}_dist'])
    cov = np.random.default_rng(3).random((N, N)) < 0.6
    cov[0, 0], cov[1, 2], cov[2, 1] = False, False, True
    masked = scene.overlap_matrix(dcaps, covisible=cov, max_pairs_in_flight=4).cpu().numpy()
    assert not masked[~cov].any() and np.array_equal(masked[cov], dist[cov]) and masked[2, 1] > 0
    assert not scene.overlap_matrix(dcaps, covisible=np.zeros((N, N), dtype=bool)).any()


def test_world_points():
    """validity exact, xyz bit-equal as float32 (the scenes hold no float64 value within round-off of a float32 tie)"""
    caps = golden_scene('mixed')[0] + small_scene((30, 13, 20)) + small_scene((30, 1, 1))
    assert sum(oracle.float32_ties(c) for c in caps) == 0
    got = scene.world_points([up(c) for c in caps])
    assert len(got) == len(caps)
    for c, (xyz, valid) in zip(caps, got):
        want_xyz, want_valid, _ = oracle.world_points(c)
        assert xyz.dtype == torch.float32 and valid.dtype == torch.bool and tuple(xyz.shape) == (c.depth.size, 3)
        assert np.array_equal(valid.cpu().numpy(), want_valid) and np.array_equal(want_valid, c.depth.reshape(-1) > 0)
        assert np.array_equal(xyz.cpu().numpy()[want_valid].view(np.uint32), want_xyz[want_valid].view(np.uint32))
        assert torch.isnan(xyz[~valid]).all()


@pytest.mark.parametrize('name', ['plain', 'mixed'])
def test_knn_pool_and_draw_pairs(name):
    """on the DEVICE matrix, against the oracle and the recorded get_knn lists"""
    caps, want_dist, _ = golden_scene(name)
    dist = scene.overlap_matrix([up(c) for c in caps])
    u = np.random.default_rng(5).random(N)
    for k in (1, 2, 3, 5, 7):
        for mask in (None, GOLDEN['db_mask'], [2]):
            pool, counts = scene.knn_pool(dist, k, mask)
            assert pool.dtype == torch.int64 and tuple(pool.shape) == (N, k) and tuple(counts.shape) == (N,)
            want_pool, want_counts = oracle.knn_pool(want_dist, k, mask)
            assert np.array_equal(pool.cpu().numpy(), want_pool) and np.array_equal(counts.cpu().numpy(), want_counts)
            tag = 'all' if mask is None else 'db'
            if f'{name}_knn_k{k}_{tag}' in GOLDEN.files and (mask is None or len(mask) > 1):
                ok = oracle.num_pos(want_dist, mask) >= 1
                assert np.array_equal(pool.cpu().numpy()[ok], GOLDEN[f'{name}_knn_k{k}_{tag}'][ok])
            for uu in (u, torch.from_numpy(u).cuda(), np.zeros(N), np.full(N, 1 - 2.0 ** -53)):
                drawn = scene.draw_pairs(pool, counts, uu)
                assert drawn.dtype == torch.int64 and tuple(drawn.shape) == (N,)
                host = uu.cpu().numpy() if torch.is_tensor(uu) else uu
                assert np.array_equal(drawn.cpu().numpy(), oracle.draw_pairs(want_pool, want_counts, host))


def test_captures_to_training_batch():
    """overlap_matrix -> knn_pool -> draw_pairs -> make_zoom_batch on synth_scene: the queries the oracle says have a
    neighbour (num_pos >= 1) come back valid with a neighbour of overlap > 0.1; nothing in between leaves the device but
    the drawn indices that select the captures"""
    caps, want_dist, _ = golden_scene('plain')
    dcaps = [up(c) for c in caps]
    dist = scene.overlap_matrix(dcaps)
    pool, counts = scene.knn_pool(dist, 2)
    u = np.random.default_rng(9).random(N)
    nn = scene.draw_pairs(pool, counts, u)
    assert np.array_equal(nn.cpu().numpy(), oracle.draw_pairs(*oracle.knn_pool(want_dist, 2), u))
    has = oracle.num_pos(want_dist) >= 1
    assert has.sum() == N - 2
    nn = nn.tolist()
    assert all(want_dist[i, nn[i]] > 0.1 and nn[i] != i for i in np.flatnonzero(has))
    num_kp = 16
    rng = np.random.default_rng(1)
    rand = {'seed': rng.random((N, 100)), 'zoom': rng.random(N), 'jitter': rng.random((N, 2)), 'trim': rng.random((N, num_kp)),
            'flip': rng.random(N)}
    out = data.make_zoom_batch(dcaps, [dcaps[j] for j in nn], num_kp, [1.0, 0.7], 0.1, rand=rand)
    valid = out['valid'].cpu().numpy()
    print('valid', valid, 'neighbours', nn)
    assert valid[has].all() and not valid[~has].any()
    assert tuple(out['image'].shape) == (N, 3, 256, 512) and tuple(out['queries'].shape) == (N, 2 * num_kp, 2)
