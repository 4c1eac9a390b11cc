"""Pairs entry points without a GPU: declared, exported, NULL-handle errors, and the binding's checks of `pairs`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cotr_amd
from cotr_amd import _lib
from cotr_amd.models import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('cotr_encode_pairs', 'cotr_forward_pairs', 'cotr_scratch_bytes_pairs')


def test_pairs_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'cotr_hip.h')).read()
    for name in NAMES:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    lib = _lib.load_library()
    for name in NAMES:
        assert getattr(lib, name) is not None


def test_pairs_null_handle_is_an_argument_error():
    lib = _lib.load_library()
    idx = (ctypes.c_int * 2)(0, 1)
    assert lib.cotr_encode_pairs(None, None, 2, idx, 1, None) == -1
    assert lib.cotr_forward_pairs(None, None, 2, idx, None, 1, 1, None, None) == -1
    n = ctypes.c_size_t()
    assert lib.cotr_scratch_bytes_pairs(None, 2, 1, 1, ctypes.byref(n)) == -1


BAD_PAIRS = [
    ([(0, 3)], 'image index'),                   # out of range (M = 3)
    ([(0, 1), (-1, 2)], 'image index'),          # negative
    ([(0, 1, 2)], 'not 2'),                      # wrong shape
    ([(0,)], 'not 2'),
    ([], 'no pair'),                             # B = 0
    (torch.zeros(0, 2, dtype=torch.int32), 'no pair'),
    (torch.tensor([[0.0, 1.0]]), 'integers'),
    ([(0.5, 1)], 'image index'),
    ([(True, 1)], 'image index'),
    (7, 'sequence'),
    (np.array([[0, 1], [2, 5]]), 'image index'),
]


@pytest.mark.parametrize('pairs,err', BAD_PAIRS)
def test_binding_rejects_bad_pairs_before_touching_a_device(pairs, err):
    m = build_model(cotr_amd.default_args()).eval()
    images = torch.zeros(3, 3, 256, 256)
    with pytest.raises(ValueError, match=err):
        m.encode_pairs(images, pairs)
    with pytest.raises(ValueError, match=err):
        m.forward_pairs(images, pairs, torch.zeros(1, 4, 2))
    assert m._handle is None


def test_binding_rejects_bad_images_and_queries():
    m = build_model(cotr_amd.default_args()).eval()
    with pytest.raises(ValueError, match='images'):
        m.encode_pairs(torch.zeros(2, 3, 256, 512), [(0, 1)])
    with pytest.raises(ValueError, match='no image'):
        m.encode_pairs(torch.zeros(0, 3, 256, 256), [(0, 0)])
    with pytest.raises(ValueError, match='queries'):
        m.forward_pairs(torch.zeros(2, 3, 256, 256), [(0, 1), (1, 0)], torch.zeros(1, 4, 2))
    assert m._handle is None


def test_binding_accepts_good_pairs_up_to_the_device():
    # good pairs get past the checks: a CPU model then stops at the device check, not at a ValueError
    m = build_model(cotr_amd.default_args()).eval()
    for pairs in ([(0, 1), (1, 0), (2, 2)], torch.tensor([[0, 1], [2, 0]]), np.array([[1, 1]], dtype=np.int64)):
        with pytest.raises(_lib.CotrHipError, match='MI355X'):
            m.encode_pairs(torch.zeros(3, 3, 256, 256), pairs)


def test_pairs_need_eval_mode():
    m = build_model(cotr_amd.default_args()).train()
    with pytest.raises(NotImplementedError):
        m.encode_pairs(torch.zeros(2, 3, 256, 256), [(0, 1)])
