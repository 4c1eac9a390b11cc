"""cotr_amd/data.py without a GPU: the numpy oracle of tests/dataset_oracle.py reproduces what the reference's own projector
returned (tests/golden/dataset_corrs.npz, written by tests/golden/make_dataset_golden.py), its NEAREST restatement is Pillow's,
its box rule is patch_boxes, the argument checks run before any upload, and the new entry points are declared, bound and
refuse bad arguments before any HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cotr_amd
from cotr_amd import _lib, data
from cotr_amd.build import declared_symbols
from cotr_amd.inference import patch_boxes
from cotr_amd.utils.synth import synth_captures
from tests import dataset_oracle as oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dataset_corrs.npz')
NEW_SYMBOLS = ('cotr_depth_corrs', 'cotr_depth_corrs_scratch', 'cotr_depth_valid', 'cotr_crop_depth_nearest')


def test_oracle_reproduces_the_reference_projector():
    g = np.load(GOLDEN)
    query, nn = synth_captures(int(g['seed']), *g['shape'])
    r = oracle.reproject(query.depth, nn.depth, query.K, query.c2w, nn.K, nn.c2w)
    assert r['rows'].shape == g['q2n'].shape
    assert np.array_equal(r['rows'][:, :2], g['q2n'][:, :2])                     # the same pixels in the same order
    assert np.abs(r['rows'] - g['q2n']).max() <= 1e-12
    print('smallest margin', r['margin'].min())
    # every reject branch is taken in this scene: holes, out of view, inconsistent depth
    n_valid, n_finite = int((query.depth > 0).sum()), int(np.isfinite(r['margin']).sum())
    assert 0 < r['rows'].shape[0] < n_valid == n_finite < query.depth.size
    inside = (r['uv'][:, 0] >= 0) & (r['uv'][:, 0] < nn.depth.shape[1] - 1) & (r['uv'][:, 1] >= 0) & (r['uv'][:, 1] < nn.depth.shape[0] - 1)
    assert r['rows'].shape[0] < int((inside & (query.depth.reshape(-1) > 0)).sum()) < n_valid
    for name, a, b in (('q2n', query, nn), ('n2q', nn, query)):                  # the subset path, repeats included, both directions
        valid = np.flatnonzero(a.depth.reshape(-1) > 0)
        pick = g[name + '_pick']
        assert len(np.unique(pick)) < len(pick)
        s = oracle.reproject(a.depth, b.depth, a.K, a.c2w, b.K, b.c2w, subset=valid[pick])
        assert s['rows'].shape == g[name + '_subset'].shape and np.abs(s['rows'] - g[name + '_subset']).max() <= 1e-12


def test_synth_captures_is_seeded_and_exercises_every_branch():
    a, b = synth_captures(3, 256, 256)
    a2, _ = synth_captures(3, 256, 256)
    assert np.array_equal(a.depth, a2.depth) and np.array_equal(a.image, a2.image)
    assert a.image.dtype == np.uint8 and a.depth.dtype == np.float32 and a.K.dtype == a.c2w.dtype == np.float64
    r = oracle.reproject(a.depth, b.depth, a.K, a.c2w, b.K, b.c2w)
    n_valid, n_keep = int((a.depth > 0).sum()), int(r['keep'].sum())
    assert 1000 < n_keep < n_valid < 256 * 256
    assert len(np.unique(a.depth)) > 1000


@pytest.mark.parametrize('size', [1, 2, 3, 18, 97, 255, 256, 257, 300, 511, 600, 1201])
def test_nearest_restatement_is_pillow(size):
    d = np.random.default_rng(size).random((size, size)).astype(np.float32)
    assert np.array_equal(oracle.nearest_resize(d), oracle.pillow_nearest(d))
    assert np.array_equal(oracle.nearest_resize(d, 37), oracle.pillow_nearest(d, 37))


def test_box_rule_is_patch_boxes():
    rng = np.random.default_rng(0)
    for shape in ((480, 640, 3), (300, 200, 3)):
        for scale in (1.0, 0.5, 0.137, 0.031):
            pos = rng.uniform(-20, max(shape) + 20, (50, 2))
            x, y, size = patch_boxes(shape, pos, scale)
            for i in range(50):
                assert oracle.patch_box(shape, pos[i], scale) == (int(x[i]), int(y[i]), size)
    K = np.array([[500.0, 0, 320.5], [0, 510.0, 239.25], [0, 0, 1]])
    assert np.array_equal(data.cropped_K(K, (10, 20, 96)), oracle.cropped_K(K, (10, 20, 96)))
    s = 256 / 96
    assert np.array_equal(data.cropped_K(K, (10, 20, 96)), [[500.0 * s, 0, (320.5 - 10) * s], [0, 510.0 * s, (239.25 - 20) * s], [0, 0, 1]])


def test_argument_checks_need_no_gpu():
    q, n = synth_captures(1, 32, 40)
    with pytest.raises(_lib.CotrHipError, match='CPU tensor'):
        data.depth_corrs(q._replace(depth=torch.from_numpy(q.depth)), n)
    with pytest.raises(_lib.CotrHipError, match='CPU tensor'):
        data.make_zoom_batch([q._replace(image=torch.from_numpy(q.image))], [n], 10, [0.5], 0.1)
    with pytest.raises(_lib.CotrHipError, match='CPU tensor'):
        data.crop_capture(q._replace(depth=torch.from_numpy(q.depth)), (0, 0, 8))
    for bad in (q._replace(depth=q.depth.astype(np.float64)), q._replace(depth=q.depth[0]), q._replace(image=q.image[:, :, :2]),
                q._replace(image=q.image.astype(np.float32)), q._replace(K=q.K.astype(np.float32)), q._replace(c2w=q.c2w[:3]),
                q._replace(K=np.full((3, 3), np.nan)), (q.image, q.depth, q.K)):
        with pytest.raises(ValueError):
            data.make_zoom_batch([bad], [n], 10, [0.5], 0.1)
        with pytest.raises(ValueError):
            data.make_batch([n], [bad], 10)
    with pytest.raises(ValueError):
        data.make_zoom_batch([q, q], [n], 10, [0.5], 0.1)
    with pytest.raises(ValueError):
        data.make_zoom_batch([q], [n], 0, [0.5], 0.1)
    with pytest.raises(ValueError):
        data.make_zoom_batch([q], [n], 10, [], 0.1)
    with pytest.raises(ValueError):
        data.make_zoom_batch([q], [n], 10, [0.01], 0.1)            # a patch below 2 pixels
    with pytest.raises(ValueError):
        data.crop_capture(q, (30, 0, 16))                          # outside the capture
    assert cotr_amd.make_zoom_batch is data.make_zoom_batch and cotr_amd.depth_corrs is data.depth_corrs
    assert cotr_amd.Capture is data.Capture and cotr_amd.crop_capture is data.crop_capture and cotr_amd.make_batch is data.make_batch


def test_new_symbols_are_declared_bound_and_check_their_arguments():
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and name in declared_symbols()
    lib = _lib.load_library()
    assert lib.cotr_abi_version() == 2
    assert lib.cotr_depth_corrs_scratch(16, 65536) == 16 * 256 * 36 and lib.cotr_depth_corrs_scratch(1, 1) == 48
    assert lib.cotr_depth_corrs_scratch(0, 10) == 0 and lib.cotr_depth_corrs_scratch(1, 0) == 0
    buf = (ctypes.c_double * 64)()                                   # host memory: never reached, the checks come first
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.cotr_depth_corrs(p, p, p, 0, 1, p, 1, p, p, 64, None) == 0            # n == 0 does nothing
    for args in ((p, p, p, -1, 1, p, 1, p, p, 64, None), (p, p, p, 1, 0, p, 1, p, p, 64, None), (None, p, p, 1, 1, p, 1, p, p, 64, None),
                 (p, p, None, 1, 1, p, 1, p, p, 64, None), (p, p, p, 1, 1, p, -1, p, p, 64, None), (p, p, p, 1, 1, p, 1, p, p, 47, None),
                 (p, p, p, 1, 1, p, 1, p, None, 64, None), (p, p, p, 1, 1, None, 1, p, p, 64, None)):
        assert lib.cotr_depth_corrs(*args) == -1, args
        assert lib.cotr_raster_last_error()
    assert lib.cotr_depth_valid(p, p, 1, 1, p, 1, p, p, 47, None) == -1
    assert lib.cotr_depth_valid(None, p, 1, 1, p, 1, p, p, 64, None) == -1
    for args in ((p, p, p, -1, p, 256, None), (p, p, p, 1, p, 0, None), (p, p, p, 1, p, 4097, None), (None, p, p, 1, p, 256, None),
                 (p, p, p, 1, None, 256, None)):
        assert lib.cotr_crop_depth_nearest(*args) == -1, args
