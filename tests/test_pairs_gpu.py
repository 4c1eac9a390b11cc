"""Pairs calls (cotr_encode_pairs / cotr_forward_pairs, model.encode_pairs / forward_pairs): B pairs drawn from M distinct images
[M, 3, 256, 256], each image's backbone run once.  Pair b must give what cotr_forward gives on the materialised side-by-side input
[images[l] | images[r]]: bit for bit on the identity layout (pairs (2i, 2i + 1), where the image slots and the pair passes are the
dense call's passes), within the oracle bar and the launch-configuration noise on every other layout."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import cotr_amd
from cotr_amd import _lib
from cotr_amd.models import build_model
from cotr_amd.utils.synth import synth_state_dict, synth_inputs
from oracle import cotr_oracle as O
from tests import gpu_helpers as G
from tests import raw_abi
from tests.knob_cases import KNOB_CASES, case_values
from tests.test_stages_fp64_gpu import FLOOR, _rel

pytestmark = pytest.mark.gpu

PX_BAR = 1e-3
SHAPE_NOISE_PX = 3e-4  # same math, different fp32 summation order between launch configurations
POOL = 16

_cache = {}


def hip_model():
    if 'm' not in _cache:
        m = build_model(cotr_amd.default_args()).cuda().eval()
        m.load_state_dict(synth_state_dict(0))
        _cache['m'] = m
    return _cache['m']


def image_pool():
    """POOL distinct images [POOL, 3, 256, 256]: the halves of seeded side-by-side inputs"""
    if 'pool' not in _cache:
        img, _ = synth_inputs(POOL // 2, 0, seed=700)
        _cache['pool'] = torch.cat([img[..., :256], img[..., 256:]]).contiguous()
    return _cache['pool']


def materialise(images, pairs):
    return torch.stack([torch.cat([images[l], images[r]], -1) for l, r in pairs])


def queries(b, q, seed):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).random((b, q, 2)).astype(np.float32))


def oracle_pairs(images_key, images, pairs, qs):
    """the CPU oracle per pair; a pair's encode is cached by its (left, right) images"""
    sd = synth_state_dict(0)
    enc = _cache.setdefault(('enc', images_key), {})
    out = torch.zeros(len(pairs), qs.shape[1], 2)
    with torch.no_grad():
        for b, (l, r) in enumerate(pairs):
            if (l, r) not in enc:
                e = O.cotr_encode(sd, materialise(images, [(l, r)]))
                enc[(l, r)] = (e['memory'], e['pos'])
            mem, pos = enc[(l, r)]
            out[b] = O.cotr_decode(sd, mem, pos, qs[b:b + 1])['pred_corrs'][0]
    return out


# ---- 1. identity layout: bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b', [1, 2, 17, 130])
def test_identity_layout_is_bit_identical_to_cotr_forward(b):
    img, qs = synth_inputs(b, 1000, seed=800 + b)
    img, qs = img.cuda(), qs.cuda()
    images = torch.stack([img[..., :256], img[..., 256:]], 1).reshape(2 * b, 3, 256, 256).contiguous()
    pairs = [(2 * i, 2 * i + 1) for i in range(b)]
    m = hip_model()
    dense = m(img, qs)['pred_corrs'].clone()
    got = m.forward_pairs(images, pairs, qs)['pred_corrs']
    assert torch.equal(got, dense), (b, float((got - dense).abs().max()))


# ---- 2. every layout against the oracle ---------------------------------------------------------------------------------------------
LAYOUTS = {
    'one_to_many_1v32': (POOL, [(0, 1 + (j % (POOL - 1))) for j in range(32)]),
    'both_directions': (8, [p for i in range(4) for p in ((2 * i, 2 * i + 1), (2 * i + 1, 2 * i))]),
    'all_28_of_8': (8, list(itertools.combinations(range(8), 2))),
    'self_pairs': (4, [(0, 0), (3, 3), (1, 2)]),
    'repeated_pairs': (4, [(1, 2), (1, 2), (0, 3), (1, 2)]),
    'unused_images': (POOL, [(5, 9), (12, 5)]),
    'odd_m': (5, [(4, 0), (2, 4), (4, 4), (1, 3)]),
    'one_image_b3': (1, [(0, 0)] * 3),
}


@pytest.mark.parametrize('name', list(LAYOUTS))
def test_every_layout_matches_the_oracle_and_the_dense_call(name):
    m_img, pairs = LAYOUTS[name]
    images = image_pool()[:m_img]
    qs = queries(len(pairs), 100, seed=900 + len(pairs))
    m = hip_model()
    out = m.forward_pairs(images.cuda(), pairs, qs.cuda())['pred_corrs'].cpu()
    assert out.shape == (len(pairs), 100, 2) and torch.isfinite(out).all()
    dense = m(materialise(images, pairs).cuda(), qs.cuda())['pred_corrs'].cpu()
    assert O.px_err(out, dense) < SHAPE_NOISE_PX, name
    ref = oracle_pairs('pool', image_pool(), pairs, qs)
    for b in range(len(pairs)):
        assert O.px_err(out[b], ref[b]) < PX_BAR, (name, b, pairs[b])


def test_pairs_with_many_passes_match_the_dense_call():
    """130 pairs of 16 images, every pass cut of both phases (8 image slots; 64 + 64 + 2 pairs): against the dense call"""
    rng = np.random.Generator(np.random.PCG64(5))
    pairs = [tuple(int(v) for v in rng.integers(0, POOL, 2)) for _ in range(130)]
    images = image_pool().cuda()
    qs = queries(130, 50, seed=6).cuda()
    m = hip_model()
    out = m.forward_pairs(images, pairs, qs)['pred_corrs']
    dense = m(materialise(images, pairs), qs)['pred_corrs']
    assert O.px_err(out.cpu(), dense.cpu()) < SHAPE_NOISE_PX


# ---- 3. taps against float64 --------------------------------------------------------------------------------------------------------
def test_src_and_memory_taps_against_float64():
    """debug taps on: src of the last pair pass (the gather's output) and the memory of every pair against the float64 oracle, with
    the bar rule of tests/test_stages_fp64_gpu.py (err <= max(FLOOR, 4 x the float32 oracle's gap))"""
    pairs = [(3, 0), (0, 3), (2, 2), (1, 4)]
    images = image_pool()[:5]
    qs = queries(len(pairs), 20, seed=31)
    m = hip_model()
    m.set_debug_taps(True)
    try:
        m.forward_pairs(images.cuda(), pairs, qs.cuda())
        src = m.debug_tap('src').view(-1, 512, 256).cpu()
        mem = m.debug_tap('memory').view(len(pairs), 512, 256).cpu()
    finally:
        m.set_debug_taps(False)
    last = len(pairs) - src.shape[0]                      # the last pass holds the last src.shape[0] pairs
    assert last >= 0
    sd = synth_state_dict(0)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        for b, (l, r) in enumerate(pairs):
            x = materialise(images, [(l, r)])
            t64, t32 = {}, {}
            e64 = O.cotr_encode(sd64, x, torch.float64, taps=t64)
            e32 = O.cotr_encode(sd, x, torch.float32, taps=t32)
            gap = _rel(e32['memory'], e64['memory'])
            assert _rel(mem[b], O.seq_to_rows(e64['memory'])) <= max(FLOOR['memory'], 4 * gap), (b, 'memory')
            if b >= last:
                gap = _rel(t32['src'], t64['src'])
                assert _rel(src[b - last], O.seq_to_rows(t64['src'])) <= max(1e-5, 4 * gap), (b, 'src')


# ---- 4. encode once, decode many ----------------------------------------------------------------------------------------------------
def test_encode_pairs_then_decode_many():
    pairs = [(0, 1), (1, 0), (2, 2), (5, 1)]
    images = image_pool()[:6].cuda()
    q1, q2 = queries(4, 300, seed=41).cuda(), queries(4, 17, seed=42).cuda()
    counts = [5, 0, 300, 17]
    qv = queries(1, sum(counts), seed=43)[0].cuda()
    m = hip_model()
    assert m.encode_pairs(images, pairs) is m
    d1, d2 = m.decode(q1), m.decode(q2)
    dv = m.decode_varlen(qv, counts)
    assert torch.equal(d1, m.forward_pairs(images, pairs, q1)['pred_corrs'])
    assert torch.equal(d2, m.forward_pairs(images, pairs, q2)['pred_corrs'])
    dense = m.forward_varlen(materialise(images, pairs), qv, counts)        # (its own encode: launch-configuration noise apart)
    assert O.px_err(dv.cpu(), dense.cpu()) < SHAPE_NOISE_PX


# ---- 5. caller workspace ------------------------------------------------------------------------------------------------------------
def test_caller_workspace_of_exactly_cotr_scratch_bytes_pairs():
    """A workspace of exactly cotr_scratch_bytes_pairs bytes filled with NaN serves the call (the library never allocates with a
    workspace set: a region that does not fit is an error), gives the binding's bits, and a guard region behind `out` stays."""
    lib = _lib.load_library()
    m = build_model(cotr_amd.default_args()).cuda().eval()
    m.load_state_dict(synth_state_dict(0))
    pairs = [(0, 1 + j % (POOL - 1)) for j in range(19)] + [(7, 7)]   # 20 pairs: 16 + 4 under batch_split; 8 image slots
    images = image_pool().cuda()
    qs = queries(len(pairs), 333, seed=51).cuda()
    ref = m.forward_pairs(images, pairs, qs)['pred_corrs'].clone()
    B, Q = len(pairs), 333
    guard = 4096
    buf = torch.full((B * Q * 2 + guard,), 7.25, device='cuda')
    idx = (ctypes.c_int * (2 * B))(*[v for p in pairs for v in p])
    with raw_abi.caller_workspace(m, raw_abi.scratch_bytes_pairs(m, POOL, B, Q), fill=float('nan')):
        rc = lib.cotr_forward_pairs(m._handle, images.data_ptr(), POOL, idx, qs.data_ptr(), B, Q, buf.data_ptr(),
                                    _lib.current_stream_ptr())
        assert rc == 0, lib.cotr_last_error(m._handle)
        torch.cuda.synchronize()
        assert torch.equal(buf[:B * Q * 2].view(B, Q, 2), ref)
        assert bool((buf[B * Q * 2:] == 7.25).all())
        assert raw_abi.set_workspace(m, None, 0) == 0


# ---- 6. graph capture ---------------------------------------------------------------------------------------------------------------
def test_forward_pairs_replays_as_a_captured_hip_graph():
    m = hip_model()
    pairs = [(0, j) for j in range(1, 6)] + [(3, 2), (2, 3)]
    simg = image_pool()[:6].cuda().clone()
    sqs = queries(len(pairs), 200, seed=61).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            m.forward_pairs(simg, pairs, sqs)                  # sizes the workspace, sets kernel attributes
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sout = m.forward_pairs(simg, pairs, sqs)['pred_corrs']
    for seed in (62, 63):
        img, _ = synth_inputs(3, 0, seed=seed)
        simg.copy_(torch.cat([img[..., :256], img[..., 256:]]).cuda())
        sqs.copy_(queries(len(pairs), 200, seed=seed))
        g.replay()
        torch.cuda.synchronize()
        got = sout.clone()
        assert torch.equal(got, m.forward_pairs(simg.clone(), pairs, sqs.clone())['pred_corrs'])
    del g


# ---- 7. knobs -----------------------------------------------------------------------------------------------------------------------
KNOB_VALUES = [(k, v) for k in KNOB_CASES for v in case_values(k)]


@pytest.mark.parametrize('knob,value', KNOB_VALUES, ids=[f'{k}={v}' for k, v in KNOB_VALUES])
def test_every_knob_value_on_a_one_to_many_layout(knob, value):
    pairs = [(2, j) for j in range(POOL) if j != 2][:9]          # one image against 9: 5 slots, 9 pairs (8 + 1 under batch_split)
    images = image_pool()
    qs = queries(len(pairs), 64, seed=71)
    ref = oracle_pairs('pool', images, pairs, qs)
    m = hip_model()
    with G.model_knobs(m, **{knob: value}):
        out = m.forward_pairs(images.cuda(), pairs, qs.cuda())['pred_corrs'].cpu()
    assert O.px_err(out, ref) < PX_BAR, (knob, value)


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------------
def test_malformed_indices_are_argument_errors_and_the_handle_still_works():
    lib = _lib.load_library()
    m = hip_model()
    images = image_pool()[:3].cuda()
    qs = queries(2, 10, seed=81).cuda()
    good = m.forward_pairs(images, [(0, 1), (2, 0)], qs)['pred_corrs'].clone()
    out = torch.full((2, 10, 2), 3.0, device='cuda')
    st = _lib.current_stream_ptr()
    for bad in ([0, 3, 1, 1], [0, 1, -1, 2], [5, 0, 0, 0]):
        idx = (ctypes.c_int * 4)(*bad)
        assert lib.cotr_forward_pairs(m._handle, images.data_ptr(), 3, idx, qs.data_ptr(), 2, 10, out.data_ptr(), st) == -1
        assert b'outside' in lib.cotr_last_error(m._handle)
        assert lib.cotr_encode_pairs(m._handle, images.data_ptr(), 3, idx, 2, st) == -1
    idx = (ctypes.c_int * 4)(0, 1, 2, 0)
    assert lib.cotr_encode_pairs(m._handle, images.data_ptr(), 0, idx, 2, st) == -1
    assert lib.cotr_encode_pairs(m._handle, images.data_ptr(), 3, idx, 0, st) == -1
    assert lib.cotr_encode_pairs(m._handle, None, 3, idx, 2, st) == -1
    assert lib.cotr_encode_pairs(m._handle, images.data_ptr(), 3, None, 2, st) == -1
    assert lib.cotr_forward_pairs(m._handle, images.data_ptr(), 3, idx, None, 2, 10, out.data_ptr(), st) == -1
    n = ctypes.c_size_t()
    assert lib.cotr_scratch_bytes_pairs(m._handle, 0, 2, 10, ctypes.byref(n)) == -1
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())                                # nothing was enqueued
    assert torch.equal(m.forward_pairs(images, [(0, 1), (2, 0)], qs)['pred_corrs'], good)
