"""Whole-path parity on the MI355X: libcotr_hip (through the C ABI, via the model object) against
the CPU oracle on the same seeded inputs and against the committed golden vectors generated from
the reference itself.  Bar: 1e-3 px (BASELINE.json north_star), px = |d| * (512, 256)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import cotr_amd
from cotr_amd.models import build_model
from cotr_amd.utils.synth import synth_state_dict, synth_inputs
from oracle import cotr_oracle
from tests import gpu_helpers as G

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    'make_golden', os.path.join(os.path.dirname(__file__), 'golden', 'make_golden.py'))
make_golden = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_golden)

PX_BAR = 1e-3
SHAPE_NOISE_PX = 3e-4  # same math, different fp32 summation order between launch configurations
_models = {}


def hip_model(seed=0, gain=1.0):
    key = (seed, gain)
    if key not in _models:
        m = build_model(cotr_amd.default_args()).cuda().eval()
        m.load_state_dict(synth_state_dict(seed, attn_gain=gain))
        _models[key] = m
    return _models[key]


@pytest.mark.parametrize('name', list(make_golden.CASES))
def test_golden_vectors_from_the_reference(name, golden_dir):
    wseed, gain = make_golden.CASES[name][:2]
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    sd, img, qs = make_golden.case_inputs(name)
    m = hip_model(wseed, gain)
    out = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    assert out.shape == g['pred_f32'].shape
    assert not torch.isnan(out).any()
    e64 = cotr_oracle.px_err(out, torch.from_numpy(g['pred_f64']))
    e32 = cotr_oracle.px_err(out, torch.from_numpy(g['pred_f32']))
    # ill-conditioned cases (near one-hot softmax in all 12 layers): the reference's OWN fp32 run is off its fp64 run by
    # more than the bar (peaky16: 1.7e-2 px, peaky32: 3.2 px - printed by make_golden.py); nothing in fp32 can do better,
    # so there the bar is "no further from the fp64 truth than 3x the reference's fp32 run"
    ref_gap = cotr_oracle.px_err(torch.from_numpy(g['pred_f32']), torch.from_numpy(g['pred_f64']))
    bar = max(PX_BAR, 3 * ref_gap)
    assert e64 < bar, (e64, ref_gap)
    if ref_gap < PX_BAR / 3:
        assert e32 < PX_BAR, (e64, e32)
        mem = m.debug_tap('memory').cpu().view(img.shape[0], 512, 256)[:, ::8]
        assert float((mem - torch.from_numpy(g['memory'])).abs().max()) < 1e-4


@pytest.mark.parametrize('name', ['ragged_b2_q257', 'peaky16_b1_q64', 'flat_b1_q64'])
def test_pos_tables_and_wide_attention_on_the_golden_cases(name, golden_dir):
    """The many-rows forms - pos . W^T taken from the tables of cotr_load_weights as a row-periodic residual of the in-projection
    GEMMs (instead of adding pos to the activations, transformer.py:147-153,192-195) and the 64-query attention kernel - forced onto
    the small golden cases of the reference: same bars as the default path."""
    wseed, gain = make_golden.CASES[name][:2]
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    sd, img, qs = make_golden.case_inputs(name)
    m = hip_model(wseed, gain)
    base = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    with G.model_knobs(m, pos_table_min_rows=0, attention_wide_min_rows=0, attention_fusion_max_rows=0):
        out = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    ref_gap = cotr_oracle.px_err(torch.from_numpy(g['pred_f32']), torch.from_numpy(g['pred_f64']))
    bar = max(PX_BAR, 3 * ref_gap)
    assert cotr_oracle.px_err(out, torch.from_numpy(g['pred_f64'])) < bar
    assert cotr_oracle.px_err(out, base) < max(SHAPE_NOISE_PX, 3 * ref_gap)
    if name != 'flat_b1_q64':      # (q = k = bias only: pos . W^T is zero there and the paths may agree bit for bit)
        assert not torch.equal(out, base), 'the knobs did not change the path'


def test_stage_taps_against_oracle():
    sd, img, qs = make_golden.case_inputs('ragged_b2_q257')
    taps = {}
    ref = cotr_oracle.cotr_forward(sd, img, qs, taps=taps)
    m = hip_model()
    m.set_debug_taps(True)
    out = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    checks = {
        'stem': G.nchw_to_sbs(taps['stem']), 'pool': G.nchw_to_sbs(taps['pool']),
        'layer1': G.nchw_to_sbs(taps['layer1.2']), 'layer2': G.nchw_to_sbs(taps['layer2.3']),
        'layer3': G.nchw_to_sbs(taps['layer3.5']), 'src': G.seq_to_rows(taps['src']),
        'pos': taps['pos'][:, 0], 'memory': G.seq_to_rows(taps['enc.5']),
        'query_pos': G.seq_to_rows(taps['query_pos']),
    }
    errs = {k: G.rel_err(m.debug_tap(k).cpu().view(v.shape), v) for k, v in checks.items()}
    m.set_debug_taps(False)
    assert all(e < 5e-5 for e in errs.values()), errs
    assert cotr_oracle.px_err(out, ref) < PX_BAR


def test_engine_batch_shape_b32_q1():
    """SparseEngine.infer_batch feeds img[<=32,3,256,512], q[<=32,1,2] (sparse_engine.py:47-56)."""
    sd = synth_state_dict(0)
    img, qs = synth_inputs(32, 1, seed=9)
    out = hip_model()(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    assert cotr_oracle.px_err(out, cotr_oracle.cotr_forward(sd, img, qs)) < PX_BAR


def test_encode_chunking_b40():
    """More pairs than one backbone pass (knob encode_chunk: 64 by default, 32 here so that 40 pairs take two passes):
    results must not depend on the chunking."""
    sd = synth_state_dict(0)
    img, qs = synth_inputs(40, 3, seed=10)
    m = build_model(cotr_amd.default_args()).cuda().eval()        # a model of its own: the knob is per handle
    m.load_state_dict(sd)
    m.set_knob('encode_chunk', 32)
    assert m.knobs()['encode_chunk'] == (32, 64) and hip_model().knobs()['encode_chunk'] == (64, 64)
    out = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    tail = m(img[33:35].cuda(), qs[33:35].cuda())['pred_corrs'].cpu()
    # pairs never interact; only the fp32 summation order differs (the GEMM launch configuration, hence the
    # K-split, is chosen per problem shape), so the two runs agree to rounding, not bit for bit
    assert cotr_oracle.px_err(out[33:35], tail) < SHAPE_NOISE_PX
    again = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    assert torch.equal(out, again)                             # same shape -> deterministic, bit-identical
    assert cotr_oracle.px_err(tail, cotr_oracle.cotr_forward(sd, img[33:35], qs[33:35])) < PX_BAR


def test_decode_chunking_q40000_and_query_independence():
    """Q above one decoder pass (DEC_ROWS = 32768), as the dense pass does (inference_helper.py:116-127);
    every query is independent of the others, so any subset must reproduce (to fp32 summation order)."""
    sd = synth_state_dict(0)
    img, qs = synth_inputs(1, 40000, seed=11)
    m = hip_model()
    out = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    sub = torch.cat([qs[:, :100], qs[:, 39000:39100]], 1)
    out_sub = m(img.cuda(), sub.cuda())['pred_corrs'].cpu()
    assert cotr_oracle.px_err(out_sub[:, :100], out[:, :100]) < SHAPE_NOISE_PX
    assert cotr_oracle.px_err(out_sub[:, 100:], out[:, 39000:39100]) < SHAPE_NOISE_PX
    assert cotr_oracle.px_err(out_sub, cotr_oracle.cotr_forward(sd, img, sub)) < PX_BAR
    assert not torch.isnan(out).any()


def test_encode_once_decode_twice_cycle_pass():
    """cotr_corr_base runs model(img, q) then model(img, pred) on the same image
    (inference_helper.py:197-198): the encode is reusable."""
    sd = synth_state_dict(0)
    img, qs = synth_inputs(2, 50, seed=12)
    m = hip_model()
    m.encode(img.cuda())
    fwd = m.decode(qs.cuda())
    cyc = m.decode(fwd)
    ref_fwd = cotr_oracle.cotr_forward(sd, img, qs)
    ref_cyc = cotr_oracle.cotr_forward(sd, img, ref_fwd)
    assert cotr_oracle.px_err(fwd.cpu(), ref_fwd) < PX_BAR
    assert cotr_oracle.px_err(cyc.cpu(), ref_cyc) < 2 * PX_BAR      # second pass inherits the first's error
    assert torch.equal(m(img.cuda(), qs.cuda())['pred_corrs'], fwd)


def test_edge_cases():
    m = hip_model()
    img, qs = synth_inputs(1, 4, seed=13)
    assert m(img.cuda(), qs[:, :0].cuda())['pred_corrs'].shape == (1, 0, 2)          # no queries
    with pytest.raises(AssertionError):                                               # backbone.py:80
        m(img[..., :255, :].cuda(), qs.cuda())
    bad = qs.clone()
    bad[0, 1, 0] = float('nan')
    out = m(img.cuda(), bad.cuda())['pred_corrs'].cpu()
    assert torch.isnan(out[0, 1]).all() and not torch.isnan(out[0, [0, 2, 3]]).any()  # NaN stays in its query
    # non-contiguous views and NestedTensor / list inputs
    from cotr_amd.models import NestedTensor
    wide = torch.randn(1, 3, 256, 1024)
    ref = m(wide[..., 256:768].contiguous().cuda(), qs.cuda())['pred_corrs']
    assert torch.equal(m(wide.cuda()[..., 256:768], qs.cuda())['pred_corrs'], ref)
    assert torch.equal(m(NestedTensor(wide[..., 256:768].cuda(), None), qs.cuda())['pred_corrs'], ref)
    assert torch.equal(m([wide[0, :, :, 256:768].cuda()], qs.cuda())['pred_corrs'], ref)


def test_state_dict_round_trip_and_reload():
    m = hip_model()
    img, qs = synth_inputs(1, 8, seed=14)
    a = m(img.cuda(), qs.cuda())['pred_corrs'].clone()
    sd2 = synth_state_dict(3)
    m2 = build_model(cotr_amd.default_args()).cuda().eval()
    m2.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    assert torch.equal(m2(img.cuda(), qs.cuda())['pred_corrs'], a)
    m2.load_state_dict(sd2)                                                         # new weights re-pack
    b = m2(img.cuda(), qs.cuda())['pred_corrs']
    assert cotr_oracle.px_err(b.cpu(), cotr_oracle.cotr_forward(sd2, img, qs)) < PX_BAR
    assert not torch.equal(a, b)


def test_fused_and_unfused_ffn_paths_agree():
    """The fused FFN block (always up to 1024 rows, up to 4096 where its grid fills whole rounds) and the three-launch path compute the same function."""
    sd = synth_state_dict(0)
    img, qs = synth_inputs(2, 300, seed=15)
    m = hip_model()
    fused = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    with G.model_knobs(m, ffn_fusion_max_rows=0):
        plain = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    assert not torch.equal(fused, plain)                       # really two different launch sequences
    assert cotr_oracle.px_err(fused, plain) < SHAPE_NOISE_PX
    assert cotr_oracle.px_err(plain, cotr_oracle.cotr_forward(sd, img, qs)) < PX_BAR


def test_fused_and_unfused_attention_paths_agree():
    """Default up to 1024 rows: attention with the out projection (and, in the decoder, the q projection) inside the
    kernel + ln_reduce; knob attention_fusion_max_rows = 0 is the six-launch layer.  Same function, different fp32
    summation order; both within the bar of the oracle."""
    sd = synth_state_dict(0)
    img, qs = synth_inputs(2, 300, seed=17)
    m = hip_model()
    fused = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    with G.model_knobs(m, attention_fusion_max_rows=0):
        plain = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    assert not torch.equal(fused, plain)                       # really two different launch sequences
    assert cotr_oracle.px_err(fused, plain) < SHAPE_NOISE_PX
    ref = cotr_oracle.cotr_forward(sd, img, qs)
    assert cotr_oracle.px_err(plain, ref) < PX_BAR and cotr_oracle.px_err(fused, ref) < PX_BAR


@pytest.mark.parametrize('b,q,mixes,what', [(4, 1000, True, 'encoder 2048 rows + decoder 4000 rows: both on the small-row fused kernels (2 / 4 whole rounds)'),
                                      (8, 64, True, 'encoder 4096 rows fused (4 rounds), decoder 512 rows'),
                                      (3, 333, True, 'encoder 1536 rows = 1.5 rounds: the unfused launches; decoder 999 rows fused'),
                                      (6, 500, True, 'encoder 3072 rows: attention fused (3 rounds), FFN unfused (1.5); decoder 3000 rows'),
                                      (12, 257, False, 'the grouped engine call in the middle of the batch axis: unfused layers, conv23'),
                                      (24, 100, True, 'encoder 12288 rows: att_rows / ffn_rows at 3/4 fill, pair-per-XCD placement (24 = 3 x 8)')])
def test_middle_of_the_batch_axis_against_the_oracle(b, q, mixes, what):
    """Round 6: between 1024 and 8192 rows the dispatch picks per sub-layer - the small-row fused kernels where their grid fills whole
    rounds of the 256 CUs (api.hip att_fused_applies / ffn_fused_applies), the unfused launches elsewhere, the one-launch rows kernels
    from 8192 rows on - and FasterSparseEngine's grouped calls / every partial last batch land there (sparse_engine.py:339-369,
    400-411).  Each mix: within the bar of the CPU oracle, bit-repeatable, and the same function as the all-unfused schedule."""
    sd = synth_state_dict(0)
    img, qs = synth_inputs(b, q, seed=100 + b)
    m = hip_model()
    outs = [m(img.cuda(), qs.cuda())['pred_corrs'].cpu() for _ in range(2)]
    assert torch.equal(outs[0], outs[1]), what
    ref = cotr_oracle.cotr_forward(sd, img, qs)
    assert cotr_oracle.px_err(outs[0], ref) < PX_BAR, what
    with G.model_knobs(m, ffn_fusion_max_rows=0, attention_fusion_max_rows=0, att_rows_min_rows=1 << 30, ffn_rows_min_rows=1 << 30):
        plain = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    assert cotr_oracle.px_err(outs[0], plain) < SHAPE_NOISE_PX, what
    assert torch.equal(outs[0], plain) != mixes, 'the default dispatch is not the mix this case names: ' + what


@pytest.mark.parametrize('b,q', [(17, 1000), (33, 40), (20, 257)])
def test_batch_split_walks_a_batch_as_independent_passes(b, q):
    """Knob batch_split (round 6): the forward's time against the pair count is a staircase, so a batch just above a step is walked as
    the step + a remainder - encode passes from the measured table (csrc/enc_split.inc), decode passes where a prefix of the pairs
    fills the one-launch rows kernels (api.hip enc_next_chunk / dec_next_pairs; cotr_batch_chunks reports both).  No arithmetic
    crosses pairs (cotr_model.py:26-40 is per sample), so: (1) the passes cover the batch; (2) where encode and decode cut the batch
    alike and every pass would itself run unsplit, the result is BIT FOR BIT the concatenation of separate calls on the passes;
    (3) the one-pass schedule (batch_split = 0) gives the same numbers to summation-order noise; (4) within the bar of the oracle."""
    sd = synth_state_dict(0)
    img, qs = synth_inputs(b, q, seed=300 + b)
    m = hip_model()
    enc, dec = m.batch_chunks(b, q, 0), m.batch_chunks(b, q, 1)
    assert sum(enc) == b and sum(dec) == b and min(enc + dec) >= 1
    out = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    assert torch.equal(out, m(img.cuda(), qs.cuda())['pred_corrs'].cpu())
    if enc == dec and all(m.batch_chunks(c, q, 0) == [c] and m.batch_chunks(c, q, 1) == [c] for c in enc):
        parts, a = [], 0
        for c in enc:
            parts.append(m(img[a:a + c].cuda(), qs[a:a + c].cuda())['pred_corrs'].cpu())
            a += c
        assert torch.equal(out, torch.cat(parts)), (enc, dec)
    with G.model_knobs(m, batch_split=0):
        assert m.batch_chunks(b, q, 0) == [b] and m.batch_chunks(b, q, 1) == [b]
        one = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    assert cotr_oracle.px_err(out, one) < SHAPE_NOISE_PX
    idx = [0, 1, b - 1]
    assert cotr_oracle.px_err(out[idx], cotr_oracle.cotr_forward(sd, img[idx], qs[idx])) < PX_BAR


def test_random_shapes_against_the_oracle_and_the_one_pass_schedule():
    """Fuzz of the dispatch along both axes (round 6: the measured table, the fill rules, conv23m's gap, the passes of batch_split all
    key on the shape): 24 random (pairs, queries) shapes, 1 ... 70 pairs x 1 ... 1200 queries, in random order on ONE model object (so the
    workspace grows and is re-carved as it goes).  Each: the passes cover the batch; bit-repeatable; the one-pass schedule gives the
    same numbers to summation-order noise; three of its pairs within the bar of the oracle."""
    import random
    rng = random.Random(20260930)
    sd = synth_state_dict(0)
    m = hip_model()
    shapes = [(rng.randint(1, 70), rng.choice([1, rng.randint(2, 300), rng.randint(300, 1200)])) for _ in range(24)]
    for i, (b, q) in enumerate(shapes):
        img, qs = synth_inputs(b, q, seed=500 + i)
        enc, dec = m.batch_chunks(b, q, 0), m.batch_chunks(b, q, 1)
        assert sum(enc) == b and sum(dec) == b, (b, q, enc, dec)
        out = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
        assert torch.isfinite(out).all(), (b, q)
        assert torch.equal(out, m(img.cuda(), qs.cuda())['pred_corrs'].cpu()), (b, q)
        with G.model_knobs(m, batch_split=0):
            one = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
        assert cotr_oracle.px_err(out, one) < SHAPE_NOISE_PX, (b, q, enc, dec)
        idx = sorted(set([0, b // 2, b - 1]))
        assert cotr_oracle.px_err(out[idx], cotr_oracle.cotr_forward(sd, img[idx], qs[idx])) < PX_BAR, (b, q, enc, dec)


@pytest.mark.parametrize('side_stream,b,q', [(0, 1, 200), (3, 1, 200), (0, 17, 1000)])
def test_eval_forward_replays_as_a_captured_hip_graph(side_stream, b, q):
    """The whole forward captured in a HIP graph (torch.cuda.graph around model(img, q): the library only enqueues kernels on the
    caller's stream - no allocation, no synchronisation once the workspace is sized) and replayed on new inputs: the eager call's bits.
    With knob side_stream = 3 the handle's second stream is forked and joined inside the capture (hipEventRecord /
    hipStreamWaitEvent are captured as graph edges): same bits again.  17 pairs x 1000 queries: a call that knob batch_split walks in
    two encode and two decode passes (16 + 1) is a longer chain of launches on the same stream, captured and replayed the same way."""
    m = hip_model()
    img0, qs0 = synth_inputs(b, q, seed=61)
    simg, sqs = img0.cuda().clone(), qs0.cuda().clone()
    with G.model_knobs(m, side_stream=side_stream):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                m(simg, sqs)                                   # sizes the workspace, creates the second stream, sets kernel attributes
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            sout = m(simg, sqs)['pred_corrs']
        for seed in (62, 63):
            img, qs = synth_inputs(b, q, seed=seed)
            simg.copy_(img.cuda())
            sqs.copy_(qs.cuda())
            g.replay()
            torch.cuda.synchronize()
            got = sout.clone()
            assert torch.equal(got, m(img.cuda(), qs.cuda())['pred_corrs'])
        del g
    assert torch.equal(got, m(img.cuda(), qs.cuda())['pred_corrs'])       # knobs back at their defaults: side stream or not, the same bits


def test_dual_conv_launch_is_bit_identical_to_two_launches():
    """The entry blocks' downsample + conv1 in one launch compute exactly what the two launches compute when the
    configuration is the same; end to end the two schedules agree to launch-configuration rounding."""
    sd = synth_state_dict(0)
    img, qs = synth_inputs(1, 64, seed=18)
    m = hip_model()
    dual = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    with G.model_knobs(m, dual_conv=0):
        plain = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    assert cotr_oracle.px_err(dual, plain) < SHAPE_NOISE_PX
    assert cotr_oracle.px_err(dual, cotr_oracle.cotr_forward(sd, img, qs)) < PX_BAR


def test_backbone_fusions_are_bit_identical_to_the_launches_they_replace():
    """conv23.hip / conv23m.hip (conv2 -> conv3 of a layer1 / layer2 bottleneck in one launch) and expand.hip (layer1 block 0's downsample
    + conv1 in one launch) keep the k order of the large-tile GEMM: a forward with them and one with the knobs that turn them off return
    the same bits - on a batch that is neither a power of two nor a multiple of the encode chunk's tile counts (29 pairs: the smallest
    odd count above conv23m's uneven-fill gap of 17 ... 27 pairs, api.hip conv23m_fill_ok), and within the 1e-3 px bar of the CPU oracle
    on its first pairs."""
    sd = synth_state_dict(0)
    img, qs = synth_inputs(29, 40, seed=29)
    m = hip_model()
    on = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    with G.model_knobs(m, conv23_min_pairs=1 << 20, conv23m_min_pairs=1 << 20, expand_min_rows=1 << 30):
        off = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    assert torch.equal(on, off)
    ref = cotr_oracle.cotr_forward(sd, img[:2], qs[:2])
    assert cotr_oracle.px_err(on[:2], ref) < 1e-3


def test_caller_supplied_workspace():
    """cotr_set_workspace: the library's encode cache + scratch live in the caller's (torch caching allocator's) memory.
    Growing shapes re-carve a larger workspace; a cached encode survives the move; a workspace that is too small is an error,
    not an overrun; NULL goes back to handle-owned memory; results do not depend on where the scratch lives."""
    from cotr_amd import _lib
    from tests import raw_abi
    lib = _lib.load_library()
    sd = synth_state_dict(0)
    m = build_model(cotr_amd.default_args()).cuda().eval()
    m.load_state_dict(sd)
    img, qs = synth_inputs(2, 40, seed=23)
    img, qs = img.cuda(), qs.cuda()
    a = m(img[:1], qs[:1, :8])['pred_corrs'].clone()
    assert m.workspace.buffer is not None and m.workspace.shape == (1, 8)
    first_ws = m.workspace.buffer.data_ptr()
    b = m(img, qs)['pred_corrs'].clone()                       # larger B and Q: new workspace
    assert m.workspace.shape == (2, 40) and m.workspace.buffer.data_ptr() != first_ws
    assert torch.equal(m(img[:1], qs[:1, :8])['pred_corrs'], a)          # smaller call inside the larger workspace
    m.encode(img)
    small = m.decode(qs[:, :8]).clone()
    _, big_q = synth_inputs(2, 3000, seed=24)
    big = m.decode(big_q.cuda())                               # Q beyond the workspace: it grows, the cached encode moves along
    assert m.workspace.shape == (2, 3000)
    assert torch.equal(m.decode(qs[:, :8]), small)
    ref = cotr_oracle.cotr_forward(sd, img.cpu(), big_q[:, ::100])
    assert cotr_oracle.px_err(big.cpu()[:, ::100], ref) < PX_BAR
    assert cotr_oracle.px_err(b.cpu(), cotr_oracle.cotr_forward(sd, img.cpu(), qs.cpu())) < PX_BAR
    # raw ABI: a workspace that is too small is refused with a message; NULL returns to handle-owned memory
    tiny = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    out = torch.empty(2, 40, 2, device='cuda')
    try:
        assert raw_abi.set_workspace(m, tiny, (1 << 20) - 256) == 0
        rc = lib.cotr_forward(m._handle, img.data_ptr(), qs.data_ptr(), 2, 40, out.data_ptr(), _lib.current_stream_ptr())
        assert rc == -1 and b'workspace too small' in lib.cotr_last_error(m._handle)
        assert raw_abi.set_workspace(m, None, 0) == 0
        rc = lib.cotr_forward(m._handle, img.data_ptr(), qs.data_ptr(), 2, 40, out.data_ptr(), _lib.current_stream_ptr())
        assert rc == 0 and torch.equal(out, b)
        assert raw_abi.scratch_bytes(m, 2, 40) > (1 << 20)
    finally:
        m.drop_workspace()          # the handle no longer holds the model's buffer


def test_workspace_serves_smaller_shapes_in_any_order():
    """One workspace sized for the largest (B, Q) must serve every smaller shape in any order: few pairs x many queries, then
    more pairs x few queries (the encoder scratch has to grow AFTER the decoder scratch was carved), then back - the order
    tools/time_configs.py walks BASELINE.json's configs in.  Results equal those of a fresh model per shape."""
    sd = synth_state_dict(0)
    m = build_model(cotr_amd.default_args()).cuda().eval()
    m.load_state_dict(sd)
    m.reserve(4, 700)
    ws = m.workspace.buffer.data_ptr()
    shapes = [(1, 700), (2, 300), (4, 16), (1, 700), (3, 1), (4, 700)]
    outs = []
    for b, q in shapes:
        img, qs = synth_inputs(b, q, seed=100 + b * 1000 + q)
        outs.append(m(img.cuda(), qs.cuda())['pred_corrs'].clone())
        assert m.workspace.buffer.data_ptr() == ws, 'the reserved workspace must be enough'
    for (b, q), o in zip(shapes[1:4], outs[1:4]):
        fresh = build_model(cotr_amd.default_args()).cuda().eval()
        fresh.load_state_dict(sd)
        img, qs = synth_inputs(b, q, seed=100 + b * 1000 + q)
        assert torch.equal(fresh(img.cuda(), qs.cuda())['pred_corrs'], o), (b, q)
    assert torch.equal(outs[0], outs[3])


def test_dense_pass_shape_q131072():
    """cotr_patch_flow_exhaustive feeds q[1,131072,2] (inference_helper.py:116-127): 4 decoder chunks; a strided
    sample of it is checked against the oracle."""
    sd = synth_state_dict(0)
    img, _ = synth_inputs(1, 1, seed=16)
    ys, xs = torch.meshgrid(torch.arange(256) / 256.0, torch.arange(512) / 512.0, indexing='ij')
    qs = torch.stack([xs, ys], -1).reshape(1, -1, 2).float()
    m = hip_model()
    out = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    assert out.shape == (1, 131072, 2) and not torch.isnan(out).any()
    idx = torch.arange(0, 131072, 997)
    ref = cotr_oracle.cotr_forward(sd, img, qs[:, idx])
    assert cotr_oracle.px_err(out[:, idx], ref) < PX_BAR


def test_config3_256_pairs_x_1000_queries():
    """BASELINE.json configs[3]: model(img[256,3,256,512], q[256,1000,2]) on one GPU (8 backbone passes of 32 pairs,
    8 decoder passes).  The oracle would need minutes for this, so full size is checked through properties the path
    guarantees: pairs never interact (a pair's answer == the same pair alone, to launch-configuration rounding, and
    == the oracle for a sample), a permutation of the pairs permutes the answers, same call twice is bit-identical."""
    sd = synth_state_dict(0)
    B, Q = 256, 1000
    base_img, base_q = synth_inputs(8, Q, seed=21)
    g = torch.Generator().manual_seed(22)
    gain = 0.5 + torch.rand(B, 1, 1, 1, generator=g)
    shift = 0.3 * torch.randn(B, 3, 1, 1, generator=g)
    img = base_img.repeat(B // 8, 1, 1, 1) * gain + shift               # 256 distinct pairs from 8 textures
    qs = torch.rand(B, Q, 2, generator=g)
    m = hip_model()
    img_d, qs_d = img.cuda(), qs.cuda()
    out = m(img_d, qs_d)['pred_corrs']
    assert out.shape == (B, Q, 2) and not torch.isnan(out).any()
    assert torch.equal(m(img_d, qs_d)['pred_corrs'], out)
    perm = torch.randperm(B, generator=g)
    out_p = m(img_d[perm.cuda()], qs_d[perm.cuda()])['pred_corrs']
    assert cotr_oracle.px_err(out_p.cpu(), out.cpu()[perm]) < SHAPE_NOISE_PX
    for b in (0, 37, 255):
        alone = m(img_d[b:b + 1], qs_d[b:b + 1])['pred_corrs'].cpu()
        assert cotr_oracle.px_err(alone, out[b:b + 1].cpu()) < SHAPE_NOISE_PX
    ref = cotr_oracle.cotr_forward(sd, img[100:101], qs[100:101, :64])
    assert cotr_oracle.px_err(out[100:101, :64].cpu(), ref) < PX_BAR


def test_backbone_entry_points_match_the_stage_taps():
    """cotr_backbone / cotr_backbone_upto (the frozen part of the backbone in the training step) return exactly the layer1 /
    layer2 / layer3 activations the full encode produces (debug taps), in NHWC over the side-by-side pair."""
    from cotr_amd import _lib
    from tests import raw_abi
    lib = _lib.load_library()
    img, qs = synth_inputs(3, 4, seed=41)
    m = hip_model()
    img_d = img.cuda()
    m.set_debug_taps(True)
    m(img_d, qs.cuda())
    taps = {k: m.debug_tap(k).clone() for k in ('layer1', 'layer2', 'layer3')}
    m.set_debug_taps(False)
    shapes = {1: (3, 64, 128, 256), 2: (3, 32, 64, 512), 3: (3, 16, 32, 1024)}
    for stage, shape in shapes.items():
        out = m.backbone_upto(img_d, stage, out=torch.full(shape, float('nan'), device='cuda'))
        ref = taps[f'layer{stage}'].view(shape)
        # the taps run uses the unfused stem (it keeps the 'stem' tap): same math, different MFMA shape in conv1
        assert (out - ref).abs().max().item() <= 2e-5 * ref.abs().max().item(), stage
    full = torch.empty(3 * 512, 1024, device='cuda')
    _lib.check(lib.cotr_backbone(m._handle, img_d.data_ptr(), 3, full.data_ptr(), _lib.current_stream_ptr()), m._handle,
               'cotr_backbone')
    torch.cuda.synchronize()
    assert torch.equal(full.view(3, 16, 32, 1024), out)
    assert raw_abi.backbone_upto(m, img_d, 4, out) != 0
    with pytest.raises(ValueError, match='stage'):
        m.backbone_upto(img_d, 4, out=out)


def test_knobs_are_per_handle():
    """Two models = two library handles: a knob set on one (cotr_set_knob(h, ...)) changes that handle's launch schedule only -
    the other keeps the shipped path bit for bit, also when their calls alternate; a knob the library does not have is refused."""
    from cotr_amd import _lib
    sd = synth_state_dict(0)
    img, qs = synth_inputs(1, 300, seed=33)
    img, qs = img.cuda(), qs.cuda()
    a, b = (build_model(cotr_amd.default_args()).cuda().eval() for _ in range(2))
    a.load_state_dict(sd)
    b.load_state_dict(sd)
    base = a(img, qs)['pred_corrs'].clone()
    assert torch.equal(b(img, qs)['pred_corrs'], base)
    b.set_knob('attention_fusion_max_rows', 0)
    b.set_knob('ffn_fusion_max_rows', 0)
    outs = [(a(img, qs)['pred_corrs'].clone(), b(img, qs)['pred_corrs'].clone()) for _ in range(3)]
    assert all(torch.equal(x, base) for x, _ in outs)
    assert all(not torch.equal(y, base) and torch.equal(y, outs[0][1]) for _, y in outs)
    assert cotr_oracle.px_err(outs[0][1].cpu(), base.cpu()) < SHAPE_NOISE_PX
    assert a.knobs()['ffn_fusion_max_rows'] == (4096, 4096) and b.knobs()['ffn_fusion_max_rows'] == (0, 4096)
    assert _lib.knobs()['ffn_fusion_max_rows'] == (4096, 4096)           # the process-wide set is a third, untouched one
    b.reset_knobs()
    assert torch.equal(b(img, qs)['pred_corrs'], base)
    with pytest.raises(_lib.CotrHipError):
        b.set_knob('no_such_knob', 1)
    if not _lib.experimental_selected():
        with pytest.raises(_lib.CotrHipError):
            b.set_knob('coop_tail', 1)                                   # the measured dead ends are not in the product library
