"""The model's workspace object on the GPU: a deep copy starts without the original's sizing flags and computes the same bits,
drop_workspace() sizes the next call afresh, get_profile() returns every entry, batch_chunks() needs no earlier call."""
import copy

import pytest
import torch

import cotr_amd
from cotr_amd.models import build_model
from cotr_amd.utils.synth import synth_state_dict, synth_inputs
from tests import gpu_helpers as G
from tests import raw_abi

pytestmark = pytest.mark.gpu

B, Q = 2, 8


def fresh_model():
    m = build_model(cotr_amd.default_args()).cuda().eval()
    m.load_state_dict(synth_state_dict(0))
    return m


def after_varlen_and_pairs_calls():
    """(a model that has made a varlen and a pairs call, its uniform forward of img, qs -> out)"""
    m = fresh_model()
    img, qs = synth_inputs(B, Q, seed=81)
    img, qs = img.cuda(), qs.cuda()
    m.forward_varlen(img, qs.reshape(-1, 2), [Q] * B)
    m.forward_pairs(torch.cat([img[..., :256], img[..., 256:]]).contiguous(), [(0, B), (1, B + 1)], qs)
    assert m.workspace.varlen and m.workspace.images == 2 * B
    return m, img, qs, m(img, qs)['pred_corrs'].clone()


def test_a_deep_copy_sizes_its_own_workspace_and_gives_the_same_bits():
    m, img, qs, out = after_varlen_and_pairs_calls()
    c = copy.deepcopy(m)
    ws = c.workspace
    assert ws is not m.workspace and ws.buffer is None and not ws.varlen and ws.images == 0 and not ws.stale
    assert torch.equal(c(img, qs)['pred_corrs'], out)
    assert torch.equal(m(img, qs)['pred_corrs'], out)


def test_drop_workspace_between_two_forwards():
    m, img, qs, out = after_varlen_and_pairs_calls()
    old = m.workspace.buffer            # (kept alive: its address cannot be handed out again)
    m.drop_workspace()
    assert m.workspace.buffer is None
    assert torch.equal(m(img, qs)['pred_corrs'], out)
    ws = m.workspace
    assert ws.buffer.data_ptr() != old.data_ptr()
    assert ws.buffer.numel() == raw_abi.scratch_bytes(m, B, Q) + 256
    assert ws.shape == (B, Q) and not ws.varlen and ws.images == 0


PROFILE_PAIRS = 8       # the fewest pairs whose forward at encode_chunk 1 and 1 query per pair has more than 512 per-launch entries
                        # (measured: 28 + 66 per pair - 490 at 7 pairs, 556 at 8)


def test_get_profile_returns_every_entry_beyond_512():
    m = fresh_model()
    img, qs = synth_inputs(PROFILE_PAIRS, 1, seed=82)
    img, qs = img.cuda(), qs.cuda()
    profiles = {}
    with G.model_knobs(m, encode_chunk=1):
        for level in (1, 2):
            m.set_profiling(level)
            try:
                m(img, qs)
                torch.cuda.synchronize()
                profiles[level] = m.get_profile()
                assert m.profile_names() == [n for n, _ in profiles[level]]
            finally:
                m.set_profiling(0)
    assert len(profiles[2]) > 512
    assert all(ms >= 0 for _, ms in profiles[2])
    # api.hip prof_mark, once per encode pass and one pass per pair: the stage marks at level 1, these launches at level 2
    per_pass = {1: ('stem+pool', 'input_proj', 'encoder', 'dec_kv'),
                2: ('stem_pool conv7x7+bn+relu+maxpool',) + tuple(f'bottleneck layer1.{i} 1 pairs' for i in range(3))}
    for level, stages in per_pass.items():
        names = [n for n, _ in profiles[level]]
        for stage in stages:
            assert names.count(stage) == PROFILE_PAIRS, (level, stage, names.count(stage))


def test_batch_chunks_before_and_after_the_first_call():
    m = fresh_model()
    assert m._handle is None
    dec, enc = m.batch_chunks(17, 1000, 1), m.batch_chunks(17, 1000, 0)
    assert sum(dec) == 17 and sum(enc) == 17 and min(dec + enc) >= 1
    img, qs = synth_inputs(1, 1, seed=83)
    m(img.cuda(), qs.cuda())
    assert m.batch_chunks(17, 1000, 1) == dec and m.batch_chunks(17, 1000, 0) == enc
