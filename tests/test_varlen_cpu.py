"""Varlen entry points without a GPU: declared, exported, NULL-handle errors, and the binding's checks of `counts`."""
import ctypes
import os
import re

import pytest
import torch

import cotr_amd
from cotr_amd import _lib
from cotr_amd.models import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('cotr_decode_varlen', 'cotr_forward_varlen', 'cotr_scratch_bytes_varlen')


def test_varlen_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'cotr_hip.h')).read()
    for name in NAMES:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    lib = _lib.load_library()
    for name in NAMES:
        assert getattr(lib, name) is not None


def test_varlen_null_handle_is_an_argument_error():
    lib = _lib.load_library()
    offs = (ctypes.c_int * 2)(0, 1)
    assert lib.cotr_decode_varlen(None, None, offs, 1, None, None) == -1
    assert lib.cotr_forward_varlen(None, None, None, offs, 1, None, None) == -1
    n = ctypes.c_size_t()
    assert lib.cotr_scratch_bytes_varlen(None, offs, 1, ctypes.byref(n)) == -1


@pytest.mark.parametrize('counts,err', [([3, 3, 0], 'sum'), ([4, -1, 4], 'non-negative'), ([7], 'counts for'), ([2, 2, 2, 1], 'counts for'),
                                        ([3.5, 3.5, 0], 'non-negative integers')])
def test_binding_rejects_bad_counts_before_touching_a_device(counts, err):
    m = build_model(cotr_amd.default_args()).eval()
    img = torch.zeros(3, 3, 256, 512)
    q = torch.zeros(7, 2)
    with pytest.raises(ValueError, match=err):
        m.forward_varlen(img, q, counts)
    assert m._handle is None
    m._encoded_batch = 3                    # as after an encode of 3 pairs
    with pytest.raises(ValueError, match=err):
        m.decode_varlen(q, counts)
    assert m._handle is None


def test_binding_rejects_unpacked_queries():
    m = build_model(cotr_amd.default_args()).eval()
    with pytest.raises(ValueError, match='packed'):
        m.forward_varlen(torch.zeros(2, 3, 256, 512), torch.zeros(2, 3, 2), [3, 3])
