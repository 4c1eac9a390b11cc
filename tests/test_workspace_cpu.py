"""The model's workspace object without a GPU: per process like the handle - a copy or an unpickled model starts with a fresh one -
and drop_workspace()."""
import copy
import pickle

import pytest
import torch

import cotr_amd
from cotr_amd import _lib
from cotr_amd.models import build_model


def used_model():
    """a model whose workspace object looks as after varlen and pairs calls, a knob change and a captured step"""
    m = build_model(cotr_amd.default_args()).eval()
    ws = m.workspace
    ws.varlen, ws.images, ws.stale = True, 12, True
    m.set_knob('encode_chunk', 7)
    return m


def assert_fresh_workspace(ws):
    assert ws.buffer is None and ws.shape == (0, 0)
    assert ws.varlen is False and ws.images == 0 and ws.stale is False and ws.pins == set()


def assert_fresh(c, m):
    assert c.workspace is not m.workspace
    assert_fresh_workspace(c.workspace)
    assert c._handle is None and c._encoded_batch == 0
    assert c._knobs == m._knobs and c._knobs is not m._knobs


@pytest.mark.parametrize('clone', [copy.deepcopy, lambda m: pickle.loads(pickle.dumps(m))], ids=['deepcopy', 'pickle'])
def test_a_copy_starts_with_a_fresh_workspace(clone):
    m = used_model()
    m.pin_workspace(m)
    assert_fresh(clone(m), m)
    assert m.workspace.varlen and m.workspace.images == 12 and m.workspace.stale and m.workspace.pins     # the original keeps its own


def test_setstate_of_a_state_without_the_workspace_object():
    """as an older pickle has it"""
    m = used_model()
    state = m.__getstate__()
    del state['_workspace']
    c = object.__new__(type(m))
    c.__setstate__(state)
    assert_fresh(c, m)
    del state['_knobs']
    c = object.__new__(type(m))
    c.__setstate__(state)
    assert c._knobs == {}
    assert_fresh_workspace(c.workspace)


def test_drop_workspace_resets_and_refuses_while_pinned():
    m = used_model()
    m.pin_workspace(m)
    with pytest.raises(_lib.CotrHipError, match='captured training step'):
        m.drop_workspace()
    assert m.workspace.varlen and m.workspace.images == 12
    m.unpin_workspace(m)
    before = m.workspace
    m.drop_workspace()
    assert m.workspace is not before and m._encoded_batch == 0
    assert_fresh_workspace(m.workspace)
    assert m._knobs == {'encode_chunk': 7}          # knobs belong to the handle, not to the workspace


def test_backbone_upto_checks_stage_and_out_before_touching_a_device():
    m = build_model(cotr_amd.default_args()).eval()
    img = torch.zeros(1, 3, 256, 512)
    for stage, out, err in [(4, None, 'stage'), (0, None, 'stage'), (1, torch.zeros(1, 64, 128, 255), 'out must be'),
                            (2, torch.zeros(1, 32, 64, 512, dtype=torch.float64), 'out must be'),
                            (3, torch.zeros(1, 16, 1024, 32).transpose(2, 3), 'not contiguous')]:
        with pytest.raises(ValueError, match=err):
            m.backbone_upto(img, stage, out=out)
    assert m._handle is None
