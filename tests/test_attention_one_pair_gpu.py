"""The 16-query-tile form of the fused attention (attention.hip attention_q16_kernel, profile variant "q16"): what
attention_fused_splits 0 / 4 launch for q-given attention whose 32-query grid leaves CUs without a workgroup - the encoder
self-attention of one pair.  Through cotr_op_attention_fused (attention + out_proj, then ln_reduce: + bias + residual + LayerNorm)
against fp64 torch, at the softmax extremes of test_ops_gpu.py, bit for bit over two calls; and through the forward against the CPU
oracle, with the per-launch profile showing which form ran."""
import math

import pytest
import torch
import torch.nn.functional as F

from cotr_amd import _lib
from cotr_amd.utils.synth import synth_inputs, synth_state_dict
from oracle import cotr_oracle
from tests import gpu_helpers as G
from tests.test_parity_gpu import PX_BAR, hip_model

pytestmark = pytest.mark.gpu


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _q16(nb, nq):
    """the 32-query grid of the fused kernel leaves CUs idle -> the 16-query form runs (attention_fused_impl)"""
    return (nq + 31) // 32 * 8 * nb < torch.cuda.get_device_properties(0).multi_processor_count


def _reference(q, k, v, nb, nq):
    qh = q.double().view(nb, nq, 8, 32).permute(0, 2, 1, 3)
    kh = k.double().reshape(nb, 512, 8, 32).permute(0, 2, 1, 3)
    vh = v.double().reshape(nb, 512, 8, 32).permute(0, 2, 1, 3)
    return (torch.softmax(qh @ kh.transpose(-1, -2), -1) @ vh).permute(0, 2, 1, 3).reshape(nb * nq, 256)


def _fused(q, kv, wo, nb, nq, o=True):
    """cotr_op_attention_fused with q given and the out projection: (o or None, part [8][rows][256])"""
    lib = _lib.load_library()
    d = G.dev()
    R = nb * nq
    od = torch.full((R, 256), float('nan'), device=d) if o else None
    part = torch.full((8, R, 256), float('nan'), device=d)
    rc = lib.cotr_op_attention_fused(G.P(q), 256, None, None, None, None, 0.0, G.P(kv), G.P(kv[:, 256:]), 512,
                                     G.P(od), 256 if o else 0, G.P(wo), G.P(part), nb, nq, G.sptr())
    assert rc == 0
    return od, part


@pytest.mark.parametrize('nb,nq', [(1, 512), (1, 1000), (1, 333), (1, 1), (2, 512), (2, 333), (3, 77)])
def test_fused_attention_oproj_layernorm(nb, nq):
    """attention + out_proj (8 per-head partials) + ln_reduce against fp64 attention + out_proj + bias + residual + LayerNorm;
    the o-only kernel (no out projection) and the partials-only form (o == nullptr) give the same bits as the combined call."""
    lib = _lib.load_library()
    g = _g(nb * 1000 + nq + 16)
    R = nb * nq
    q = torch.randn(R, 256, generator=g) / math.sqrt(32)
    kv = torch.randn(nb * 512, 512, generator=g)
    wo, bo = torch.randn(256, 256, generator=g) / 16, 0.1 * torch.randn(256, generator=g)
    res = torch.randn(R, 256, generator=g)
    lw, lb = torch.rand(256, generator=g) + 0.5, 0.1 * torch.randn(256, generator=g)
    o_ref = _reference(q, kv[:, :256], kv[:, 256:], nb, nq)
    proj_ref = o_ref @ wo.double().t()
    y_ref = F.layer_norm(res.double() + proj_ref + bo.double(), (256,), lw.double(), lb.double())
    d = G.dev()
    qd, kvd, wod, bod, resd, lwd, lbd = (t.to(d) for t in (q, kv, wo, bo, res, lw, lb))
    o, part = _fused(qd, kvd, wod, nb, nq)
    assert G.rel_err(o, o_ref) < 2e-5
    assert G.rel_err(part.double().sum(0), proj_ref) < 3e-5
    y = torch.full((R, 256), float('nan'), device=d)
    assert lib.cotr_op_ln_reduce(G.P(part), 8, G.P(bod), G.P(resd), G.P(lwd), G.P(lbd), G.P(y), R, G.sptr()) == 0
    assert G.rel_err(y, y_ref) < 3e-5
    # bit-repeatable, and the three entry forms agree bit for bit
    o2, part2 = _fused(qd, kvd, wod, nb, nq)
    assert torch.equal(o2, o) and torch.equal(part2, part)
    _, part3 = _fused(qd, kvd, wod, nb, nq, o=False)
    assert torch.equal(part3, part)
    o4 = torch.full((R, 256), float('nan'), device=d)
    assert lib.cotr_op_attention_fused(G.P(qd), 256, None, None, None, None, 0.0, G.P(kvd), G.P(kvd[:, 256:]), 512,
                                       G.P(o4), 256, None, None, nb, nq, G.sptr()) == 0
    assert torch.equal(o4, o)


@pytest.mark.parametrize('case', ['gain64', 'gain256', 'constant', 'spike_late', 'spike_every_block', 'huge_negative'])
def test_fused_attention_softmax_extremes(case):
    """The inputs of test_ops_gpu.py test_attention_softmax_extremes (forced rescales, one-hot rows, equal scores, exp2 underflow)
    through the 16-query form - 2 pairs x 77 queries: 48 workgroups of 32 queries - against fp64, against the 8-split form, and
    bit for bit over two calls."""
    nb, nq = 2, 77
    assert _q16(nb, nq)
    g = _g(sum(map(ord, case)))
    q = torch.randn(nb * nq, 256, generator=g) / math.sqrt(32)
    k = torch.randn(nb * 512, 256, generator=g)
    v = torch.randn(nb * 512, 256, generator=g)
    if case == 'gain64':
        q *= 64.0
    elif case == 'gain256':
        q *= 256.0
    elif case == 'constant':
        k[:] = k[:1]
    elif case == 'spike_late':
        k[500::512] = 40.0 * q[:nb] / q[:nb].norm(dim=1, keepdim=True)
    elif case == 'spike_every_block':
        for blk in range(16):
            k[blk * 32 + 5::512] *= (1.0 + blk)
        q *= 8.0
    elif case == 'huge_negative':
        q *= 32.0
        k[:, :] = -k.abs()
    wo = torch.randn(256, 256, generator=_g(5)) / 16
    o_ref = _reference(q, k, v, nb, nq)
    d = G.dev()
    qd, kvd, wod = q.to(d), torch.cat([k, v], 1).to(d), wo.to(d)
    tol = 2e-5 if case in ('constant', 'spike_late') else 2e-3 if case == 'gain256' else 3e-4
    o, part = _fused(qd, kvd, wod, nb, nq)
    assert torch.isfinite(o).all() and torch.isfinite(part).all()
    assert G.rel_err(o, o_ref) < tol, case
    assert G.rel_err(part.double().sum(0), o_ref @ wo.double().t()) < 2 * tol, case
    o2, part2 = _fused(qd, kvd, wod, nb, nq)
    assert torch.equal(o2, o) and torch.equal(part2, part)
    _lib.set_knob('attention_fused_splits', 8)          # process-wide (cotr_op_* have no handle); the conftest fixture resets it
    try:
        o8, _ = _fused(qd, kvd, wod, nb, nq)
    finally:
        _lib.set_knob('attention_fused_splits', 0)
    assert G.rel_err(o8, o_ref) < tol, case


@pytest.mark.parametrize('nb,nq', [(1, 512), (1, 1000), (1, 333), (1, 1), (2, 512)])
def test_forward_one_pair_form(nb, nq):
    """The forward against the CPU oracle, bit-repeatable; the per-launch profile names the encoder form (q16 for one pair, 4 key
    splits from two pairs on) and keeps the decoder's."""
    m = hip_model()
    img, qs = synth_inputs(nb, nq, seed=40 + nq)
    out = m(img.cuda(), qs.cuda())['pred_corrs'].cpu()
    assert torch.isfinite(out).all()
    assert torch.equal(out, m(img.cuda(), qs.cuda())['pred_corrs'].cpu()), 'not bit-repeatable'
    assert cotr_oracle.px_err(out, cotr_oracle.cotr_forward(synth_state_dict(0), img, qs)) < PX_BAR
    m.set_profiling(2)
    try:
        m(img.cuda(), qs.cuda())
        torch.cuda.synchronize()
        names = [n for n, _ in m.get_profile()]
    finally:
        m.set_profiling(0)
    enc = [n for n in names if n.startswith('attention+oproj enc')]
    assert len(enc) == 6, names
    want = 'q16' if _q16(nb, 512) else 's4'
    assert all(n == f'attention+oproj enc {want}' for n in enc), enc
    assert all(n.endswith(' s4') for n in names if n.startswith('qproj+attention+oproj dec')), names
