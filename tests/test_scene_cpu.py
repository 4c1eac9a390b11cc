"""The pair selection of cotr_amd/scene.py without a GPU: the numpy oracle of tests/scene_oracle.py against what the
reference's own distance_between_two_caps and ReprojRatioKnnSearch.get_knn returned (tests/golden/scene_overlap.npz,
recorded by tests/golden/make_scene_golden.py), the properties of the synthetic scene the GPU tests lean on, and the
argument checks, which all run before any upload."""
import os

import numpy as np
import pytest
import torch

import cotr_amd
from cotr_amd import _lib, scene
from cotr_amd.data import Capture
from cotr_amd.utils.synth import synth_scene
from tests import scene_oracle as oracle

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scene_overlap.npz'))
N = int(GOLDEN['n'])
H, W = (int(v) for v in GOLDEN['shape'])
SCENES = ('plain', 'mixed')
_cache = {}


def golden_scene(name):
    """the scene of a golden entry, regenerated from its seed, with the oracle's matrix (computed once)"""
    if name not in _cache:
        scale = GOLDEN[f'{name}_scale']
        caps = synth_scene(int(GOLDEN[f'{name}_seed']), N, H, W, scale=None if name == 'plain' else scale)
        _cache[name] = (caps, *oracle.overlap_matrix(caps))
    return _cache[name]


@pytest.mark.parametrize('name', SCENES)
def test_oracle_ratios_equal_the_reference(name):
    """ratios of equal integers: exact.  No candidate of the fixture is within 1e-9 of a decision."""
    caps, dist, ambiguous = golden_scene(name)
    assert ambiguous.sum() == 0
    assert dist.dtype == np.float32 and np.array_equal(dist, GOLDEN[f'{name}_dist'])
    assert (np.diag(dist)[:N - 2] > 0.9).all()                       # the diagonal is computed like any other cell


@pytest.mark.parametrize('name', SCENES)
def test_oracle_knn_pool_equals_the_reference(name):
    """the recorded get_knn lists, exactly where the query has a valid neighbour; where it has none the reference's pick
    among equal entries is arbitrary and the single entry is compared by its value"""
    dist = GOLDEN[f'{name}_dist']
    for k in (int(k) for k in GOLDEN['ks']):
        for tag, mask in (('all', None), ('db', GOLDEN['db_mask'])):
            want = GOLDEN[f'{name}_knn_k{k}_{tag}']
            got, counts = oracle.knn_pool(dist, k, mask)
            pos = oracle.num_pos(dist, mask)
            assert (pos >= 1).sum() >= 4 and (pos == 0).sum() >= 2          # both kinds of row are in the fixture
            masked = dist.copy()
            if mask is not None:
                masked[:, np.setdiff1d(np.arange(N), mask)] = -1
            for i in range(N):
                assert counts[i] == (want[i] >= 0).sum() >= 1
                if pos[i] >= 1:
                    assert np.array_equal(got[i], want[i]), (k, tag, i)
                else:
                    assert counts[i] == 1 and masked[i, got[i, 0]] == masked[i, want[i, 0]], (k, tag, i)
    # every branch was taken: more positives than k (with the query among the top and not), and fewer
    assert (oracle.num_pos(dist) > 1).any() and (oracle.num_pos(dist) <= 5).all()


def test_scene_has_a_blind_and_an_empty_capture():
    """capture n - 2 looks away from the planes, capture n - 1 has no depth: their rows and columns of the matrix are 0"""
    for name in SCENES:
        caps, dist, _ = golden_scene(name)
        assert not caps[N - 2].depth.any() and not caps[N - 1].depth.any()
        assert not np.array_equal(caps[N - 2].c2w, caps[N - 1].c2w)
        assert not dist[N - 2:].any() and not dist[:, N - 2:].any()
        assert (dist[:N - 2, :N - 2] > 0).all()
    plain, mixed = golden_scene('plain')[0], golden_scene('mixed')[0]
    assert {c.depth.shape for c in plain} == {(H, W)} and len({c.depth.shape for c in mixed}) >= 3
    for c in mixed:                                                       # K follows the resolution: the same field of view
        assert np.allclose(c.K[0, 2] / c.depth.shape[1], 0.5) and np.allclose(c.K[1, 2] / c.depth.shape[0], 0.5)
    with pytest.raises(ValueError):
        synth_scene(0, 2, 8, 8)
    with pytest.raises(ValueError):
        synth_scene(0, 4, 8, 8, scale=(1.0, 2.0))


def test_last_in_order_rule_decides_the_many_to_one_pair():
    """a 96 x 128 capture into a 24 x 32 query of the same field of view: at least four points land on most canvas pixels
    and a z-buffer or a first-writer canvas would count a different `good`"""
    caps = golden_scene('mixed')[0]
    assert caps[0].depth.shape == (96, 128) and caps[1].depth.shape == (24, 32)
    last = oracle.overlap(caps[1], caps[0])
    assert last['crowded'] > last['hit'] / 2
    assert oracle.overlap(caps[1], caps[0], canvas_rule='minz')['good'] != last['good']
    assert oracle.overlap(caps[1], caps[0], canvas_rule='first')['good'] != last['good']


def test_draw_pairs_oracle():
    pool = np.array([[3, 1, -1], [2, -1, -1], [0, 1, 2]])
    assert oracle.draw_pairs(pool, [2, 1, 3], [0.5, 0.99, 0.99]).tolist() == [1, 2, 2]
    assert oracle.draw_pairs(pool, [2, 1, 3], [0.0, 0.0, 0.34]).tolist() == [3, 2, 1]


def test_names_are_reachable_from_the_package():
    for name in ('world_points', 'overlap_pairs', 'overlap_matrix', 'knn_pool', 'draw_pairs'):
        assert getattr(cotr_amd, name) is getattr(scene, name) and name in cotr_amd.__all__
    lib = _lib.load_library()
    assert lib.cotr_overlap_scratch(3, 100) == 3 * 400 and lib.cotr_overlap_scratch(1, 257) == 1040   # canvases are 16-byte multiples
    assert lib.cotr_overlap_scratch(0, 100) == 0 and lib.cotr_overlap_scratch(1, (1 << 28) + 1) == 0
    assert lib.cotr_world_points(None, None, None, 1, 16, None) == -1          # COTR_ERR_ARG before any HIP call
    assert b'NULL' in lib.cotr_raster_last_error()
    assert lib.cotr_overlap_pairs(None, None, None, 1, None, 1, 16, None, None, None, 0, None) == -1
    assert lib.cotr_overlap_pairs(None, None, None, 1, None, 0, 16, None, None, None, 0, None) == 0    # nothing to do


def test_argument_errors_come_before_any_upload():
    """numpy captures pass the checks up to the point where the first upload would need the GPU: everything asserted here
    is raised before that, on a machine with or without one"""
    caps = [Capture(None, np.ones((4, 5), dtype=np.float32), np.eye(3), np.eye(4)) for _ in range(3)]
    cpu = Capture(None, torch.ones(4, 5), np.eye(3), np.eye(4))
    for fn in (lambda c: scene.world_points(c), lambda c: scene.overlap_pairs(c, [[0, 1]]), lambda c: scene.overlap_matrix(c)):
        with pytest.raises(_lib.CotrHipError, match='CPU tensor'):
            fn([caps[0], cpu])
        with pytest.raises(ValueError, match='float32'):
            fn([Capture(None, np.ones((4, 5)), np.eye(3), np.eye(4))])
        with pytest.raises(ValueError, match='float64'):
            fn([Capture(None, np.ones((4, 5), dtype=np.float32), np.eye(3, dtype=np.float32), np.eye(4))])
        with pytest.raises(ValueError):
            fn([])
    for bad in ([[0, 3]], [[-1, 0]], [[0.0, 1.0]], [0, 1], [[0, 1, 2]]):
        with pytest.raises(ValueError, match='pairs'):
            scene.overlap_pairs(caps, bad)
    with pytest.raises(_lib.CotrHipError, match='CPU tensor'):
        scene.overlap_pairs(caps, torch.tensor([[0, 1]]))
    with pytest.raises(ValueError, match='max_pairs_in_flight'):
        scene.overlap_pairs(caps, [[0, 1]], max_pairs_in_flight=0)
    for bad in (np.ones((2, 3), dtype=bool), np.ones((3, 3)), np.ones(9, dtype=bool), torch.ones(3, 3, dtype=torch.bool)):
        with pytest.raises(ValueError, match='covisible'):
            scene.overlap_matrix(caps, covisible=bad)
    with pytest.raises(_lib.CotrHipError, match='CPU tensor'):
        scene.knn_pool(torch.zeros(3, 3), 1)
    with pytest.raises(ValueError):
        scene.knn_pool(np.zeros((3, 3), dtype=np.float32), 1)
    with pytest.raises(_lib.CotrHipError):
        scene.draw_pairs(torch.zeros(3, 1, dtype=torch.int64), torch.ones(3, dtype=torch.int64), np.zeros(3))
