"""Raw C-ABI plumbing the GPU tests share: the scratch-size queries on a model's handle and a caller-owned workspace
(cotr_set_workspace) for the duration of a with-block."""
import contextlib
import ctypes

import torch

from cotr_amd import _lib


def _size(fn, m, *args):
    need = ctypes.c_size_t()
    assert fn(m._handle, *args, ctypes.byref(need)) == 0, _lib.load_library().cotr_last_error(m._handle)
    return need.value


def scratch_bytes(m, b, q):
    return _size(_lib.load_library().cotr_scratch_bytes, m, b, q)


def scratch_bytes_varlen(m, offsets):
    """offsets: ctypes int[B + 1]"""
    return _size(_lib.load_library().cotr_scratch_bytes_varlen, m, offsets, len(offsets) - 1)


def scratch_bytes_pairs(m, images, b, q):
    return _size(_lib.load_library().cotr_scratch_bytes_pairs, m, images, b, q)


def backbone_upto(m, img, stage, out):
    """cotr_backbone_upto on the handle as it stands -> its return code"""
    return _lib.load_library().cotr_backbone_upto(m._handle, img.data_ptr(), img.shape[0], stage, out.data_ptr(), _lib.current_stream_ptr())


def set_workspace(m, ws, nbytes):
    """cotr_set_workspace(h, the first 256-byte boundary of tensor `ws` (None: back to handle-owned memory), nbytes, keep_encode 0)
    -> its return code"""
    ptr = None if ws is None else ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
    return _lib.load_library().cotr_set_workspace(m._handle, ptr, nbytes, 0, _lib.current_stream_ptr())


@contextlib.contextmanager
def caller_workspace(m, nbytes, fill=None):
    """The handle of model m on a caller workspace of exactly nbytes from a 256-byte boundary, every float of it `fill` where one is
    given; afterwards - also on error - the model forgets it: its next call sizes and hands over a workspace of its own."""
    ws = torch.empty((nbytes + 256 + 3) // 4, dtype=torch.float32, device='cuda')
    if fill is not None:
        ws.fill_(fill)
    try:
        assert set_workspace(m, ws, nbytes) == 0, _lib.load_library().cotr_last_error(m._handle)
        yield
    finally:
        torch.cuda.synchronize()
        m.drop_workspace()
