"""Op-level parity: each HIP kernel against the torch CPU op it replaces, same seeded inputs.
fp32 MFMA accumulates in a different order than the CPU, so the bar is a relative error of a
few fp32 ulps times sqrt(K), stated per test."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import gpu_helpers as G

pytestmark = pytest.mark.gpu


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize('M,N,K', [(1000, 256, 256), (512, 768, 256), (130, 1024, 256), (77, 256, 1024),
                                   (65536, 128, 64), (24576, 128, 64), (1, 64, 32)])
def test_linear_bias_relu_residual(M, N, K):
    g = _g(M + N + K)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    b, r = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    ref = F.relu(F.linear(x, w, b) + r)
    d = G.dev()
    y = G.op_linear(x.to(d), w.to(d), bias=b.to(d), residual=r.to(d), relu=True)
    e = G.rel_err(y, ref)
    assert e < 2e-5, e


def test_linear_pos_prologue_and_bn_epilogue():
    g = _g(5)
    M, N, K = 1024, 256, 256
    x, pos = torch.randn(M, K, generator=g), torch.randn(512, K, generator=g)
    w = torch.randn(N, K, generator=g) / 16
    sc, b = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    ref = F.linear(x + pos.repeat(2, 1), w) * sc + b
    d = G.dev()
    y = G.op_linear(x.to(d), w.to(d), x2=pos.to(d), x2_row_mod=512, scale=sc.to(d), bias=b.to(d))
    e = G.rel_err(y, ref)
    assert e < 2e-5, e


@pytest.mark.parametrize('B,H,cin,cout,k,stride', [(1, 16, 64, 64, 3, 1), (2, 16, 128, 128, 3, 2), (1, 32, 256, 512, 1, 2),
                                                   (1, 64, 64, 256, 1, 1), (1, 16, 256, 256, 3, 1), (3, 8, 64, 64, 3, 1)])
def test_conv_frozenbn_residual_relu(B, H, cin, cout, k, stride):
    g = _g(B * 1000 + H + cin + cout + k)
    x = torch.randn(B, cin, H, 2 * H, generator=g)                      # two HxH halves side by side
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    sc, b = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    conv = lambda t: F.conv2d(t, w, stride=stride, padding=k // 2)
    pre = G.per_half(conv, x) * sc.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
    res = torch.randn(pre.shape, generator=g)
    ref = F.relu(pre + res)
    d = G.dev()
    y = G.op_conv(G.nchw_to_sbs(x).to(d), G.pack_conv_weight(w).to(d), sc.to(d), b.to(d), G.nchw_to_sbs(res).to(d), True,
                  cout, k, stride)
    e = G.rel_err(G.sbs_to_nchw(y.cpu()), ref)
    assert e < 3e-5, e


def test_stem_conv7x7_and_maxpool():
    from cotr_amd import _lib
    g = _g(11)
    img = torch.randn(2, 3, 256, 512, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) / math.sqrt(147)
    sc, b = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    stem = lambda t: F.relu(F.conv2d(t, w, stride=2, padding=3) * sc.view(1, -1, 1, 1) + b.view(1, -1, 1, 1))
    ref = G.per_half(stem, img)
    ref_pool = G.per_half(lambda t: F.max_pool2d(t, 3, stride=2, padding=1), ref)
    d = G.dev()
    wp = torch.zeros(64, 160)
    wp[:, :147] = w.reshape(64, 147)
    lib = _lib.load_library()
    y = torch.empty(2, 128, 256, 64, device=d)
    img_d, wp_d, sc_d, b_d = img.to(d), wp.to(d), sc.to(d), b.to(d)   # keep alive until the kernel ran
    assert lib.cotr_op_stem(G.P(img_d), G.P(wp_d), G.P(sc_d), G.P(b_d), G.P(y), 2, G.sptr()) == 0
    e = G.rel_err(G.sbs_to_nchw(y.cpu()), ref)
    assert e < 2e-5, e
    yp = torch.empty(2, 64, 128, 64, device=d)
    assert lib.cotr_op_maxpool(G.P(y), G.P(yp), 2, 128, 128, 64, G.sptr()) == 0
    e = G.rel_err(G.sbs_to_nchw(yp.cpu()), ref_pool)
    assert e < 2e-5, e
    # the one-launch version of the same two ops (stem_pool.hip)
    yf = torch.full((2, 64, 128, 64), float('nan'), device=d)
    assert lib.cotr_op_stem_pool(G.P(img_d), G.P(wp_d), G.P(sc_d), G.P(b_d), G.P(yf), 2, G.sptr()) == 0
    e = G.rel_err(G.sbs_to_nchw(yf.cpu()), ref_pool)
    assert e < 2e-5, e


@pytest.mark.parametrize('nb,nq,gain', [(2, 200, 1.0), (1, 512, 1.0), (3, 1, 1.0), (1, 129, 6.0)])
def test_attention(nb, nq, gain):
    from cotr_amd import _lib
    g = _g(nb * 100 + nq)
    q = torch.randn(nb * nq, 256, generator=g) * gain / math.sqrt(32)   # pre-scaled q
    kv = torch.randn(nb * 512, 1024, generator=g)                        # k at col 256, v at col 640 of a wider matrix
    k, v = kv[:, 256:512], kv[:, 640:896]
    qh = q.view(nb, nq, 8, 32).permute(0, 2, 1, 3)
    kh = k.reshape(nb, 512, 8, 32).permute(0, 2, 1, 3)
    vh = v.reshape(nb, 512, 8, 32).permute(0, 2, 1, 3)
    ref = (torch.softmax(qh @ kh.transpose(-1, -2), -1) @ vh).permute(0, 2, 1, 3).reshape(nb * nq, 256)
    d = G.dev()
    qd, kvd = q.to(d), kv.to(d)
    o = torch.empty(nb * nq, 256, device=d)
    lib = _lib.load_library()
    rc = lib.cotr_op_attention(G.P(qd), 256, G.P(kvd[:, 256:]), G.P(kvd[:, 640:]), 1024, G.P(o), 256, nb, nq, G.sptr())
    assert rc == 0
    e = G.rel_err(o, ref)
    assert e < 2e-5, e


@pytest.mark.parametrize('case', ['gain64', 'gain256', 'constant', 'spike_late', 'spike_every_block', 'huge_negative'])
def test_attention_softmax_extremes(case):
    """The attention kernel keeps scores in the log2 domain with an online (running-max) softmax split over 4 key
    ranges: inputs that FORCE the rescale branch at chosen key blocks, one-hot rows, rows of equal scores and scores
    far below the running maximum (exp2 underflow), each against an fp64 reference of the whole tensor."""
    from cotr_amd import _lib
    nb, nq = 2, 77
    g = _g(hash(case) % 1000)
    q = torch.randn(nb * nq, 256, generator=g) / math.sqrt(32)
    k = torch.randn(nb * 512, 256, generator=g)
    v = torch.randn(nb * 512, 256, generator=g)
    if case == 'gain64':
        q *= 64.0
    elif case == 'gain256':
        q *= 256.0                                     # |logit| ~ 1e3: rows are one-hot, every other exponent underflows
    elif case == 'constant':
        k[:] = k[:1]                                   # every key identical: all scores of a row equal -> plain mean of v
    elif case == 'spike_late':                         # the row maximum jumps at the LAST key block of the last key split
        k[500::512] = 40.0 * q[:nb] / q[:nb].norm(dim=1, keepdim=True)     # key 500 of each pair: a huge score for some rows
    elif case == 'spike_every_block':                  # a larger maximum in every successive 32-key block: rescale each time
        for blk in range(16):
            k[blk * 32 + 5::512] *= (1.0 + blk)
        q *= 8.0
    elif case == 'huge_negative':
        q *= 32.0
        k[:, :] = -k.abs()                             # keeps a wide spread of very negative scores
    qh = q.double().view(nb, nq, 8, 32).permute(0, 2, 1, 3)
    kh = k.double().reshape(nb, 512, 8, 32).permute(0, 2, 1, 3)
    vh = v.double().reshape(nb, 512, 8, 32).permute(0, 2, 1, 3)
    ref = (torch.softmax(qh @ kh.transpose(-1, -2), -1) @ vh).permute(0, 2, 1, 3).reshape(nb * nq, 256)
    d = G.dev()
    kv = torch.cat([k, v], 1).to(d)
    o = torch.full((nb * nq, 256), float('nan'), device=d)
    lib = _lib.load_library()
    for ns in (0, 1, 2, 8):                            # automatic (4 key splits) and explicit split counts
        _lib.set_knob('attention_splits', ns)            # (process-wide set: cotr_op_* have no handle; the conftest fixture resets it)
        rc = lib.cotr_op_attention(G.P(q.to(d)), 256, G.P(kv), G.P(kv[:, 256:]), 512, G.P(o), 256, nb, nq, G.sptr())
        _lib.set_knob('attention_splits', 0)
        assert rc == 0
        assert torch.isfinite(o).all(), (case, ns)
        # one-hot rows amplify the fp32 rounding of the logits (|logit| * 2^-24 absolute) into the weights
        tol = 2e-5 if case in ('constant', 'spike_late') else 2e-3 if case == 'gain256' else 3e-4
        e = G.rel_err(o, ref)
        assert e < tol, (case, ns, e)


@pytest.mark.parametrize('occ', [2, 3])
@pytest.mark.parametrize('nb,nq', [(1, 1), (3, 77), (2, 64), (1, 65), (2, 1000), (5, 2048)])
def test_attention_wide_kernel_is_bit_identical(nb, nq, occ):
    """attention_wide_kernel (64 queries per workgroup, two query tiles per wavefront; taken from 4096 query rows up) does the
    arithmetic of attention_kernel<4> per query - same key split, same merge order - so its output must be bit-identical, ragged
    last tiles included, and both must match the fp64 reference (transformer.py:149-153, 192-195)."""
    from cotr_amd import _lib
    lib = _lib.load_library()
    g = _g(nb * 7919 + nq)
    q = torch.randn(nb * nq, 256, generator=g) * 3.0 / math.sqrt(32)
    kv = torch.randn(nb * 512, 512, generator=g)
    qh = q.double().view(nb, nq, 8, 32).permute(0, 2, 1, 3)
    kh = kv[:, :256].double().reshape(nb, 512, 8, 32).permute(0, 2, 1, 3)
    vh = kv[:, 256:].double().reshape(nb, 512, 8, 32).permute(0, 2, 1, 3)
    ref = (torch.softmax(qh @ kh.transpose(-1, -2), -1) @ vh).permute(0, 2, 1, 3).reshape(nb * nq, 256)
    d = G.dev()
    qd, kvd = q.to(d), kv.to(d)
    outs = []
    for min_rows in (1 << 30, 0):
        _lib.set_knob('attention_wide_min_rows', min_rows)
        _lib.set_knob('attention_wide_occupancy', occ)
        _lib.set_knob('attention_resident', 0)
        o = torch.full((nb * nq + 1, 256), float('nan'), device=d)      # one guard row behind the output
        assert lib.cotr_op_attention(G.P(qd), 256, G.P(kvd), G.P(kvd[:, 256:]), 512, G.P(o), 256, nb, nq, G.sptr()) == 0
        assert torch.isnan(o[-1]).all()
        outs.append(o[:-1])
    assert torch.equal(outs[0], outs[1])
    assert G.rel_err(outs[1], ref) < 2e-5


@pytest.mark.parametrize('nb,nq', [(1, 256), (3, 333), (2, 1000), (5, 2048), (1, 2100), (2, 512)])
def test_attention_resident_kernel_is_bit_identical(nb, nq):
    """attention_res_kernel (K_h / V_h of a head resident in LDS for a chunk of up to 32 query tiles, a wavefront runs the four key
    quarters of its query tile as four chains and merges them in registers; taken from 4096 query rows and 256 queries per pair up)
    does the arithmetic of attention_kernel<4> per query: bit-identical output - ragged last tiles, several chunks per pair (2100
    queries = 66 tiles) included - and it matches the fp64 reference."""
    from cotr_amd import _lib
    lib = _lib.load_library()
    g = _g(nb * 104729 + nq)
    q = torch.randn(nb * nq, 256, generator=g) * 3.0 / math.sqrt(32)
    kv = torch.randn(nb * 512, 512, generator=g)
    qh = q.double().view(nb, nq, 8, 32).permute(0, 2, 1, 3)
    kh = kv[:, :256].double().reshape(nb, 512, 8, 32).permute(0, 2, 1, 3)
    vh = kv[:, 256:].double().reshape(nb, 512, 8, 32).permute(0, 2, 1, 3)
    ref = (torch.softmax(qh @ kh.transpose(-1, -2), -1) @ vh).permute(0, 2, 1, 3).reshape(nb * nq, 256)
    d = G.dev()
    qd, kvd = q.to(d), kv.to(d)
    outs = []
    for min_rows, resident in ((1 << 30, 0), (0, 1)):
        _lib.set_knob('attention_wide_min_rows', min_rows)
        _lib.set_knob('attention_resident', resident)
        o = torch.full((nb * nq + 1, 256), float('nan'), device=d)      # one guard row behind the output
        assert lib.cotr_op_attention(G.P(qd), 256, G.P(kvd), G.P(kvd[:, 256:]), 512, G.P(o), 256, nb, nq, G.sptr()) == 0
        assert torch.isnan(o[-1]).all()
        outs.append(o[:-1])
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())
    assert G.rel_err(outs[1], ref) < 2e-5


@pytest.fixture
def fused_splits(request):
    from cotr_amd import _lib
    _lib.set_knob('attention_fused_splits', request.param)
    yield request.param
    _lib.set_knob('attention_fused_splits', 0)


@pytest.mark.parametrize('fused_splits', [4, 8], indirect=True)
@pytest.mark.parametrize('nb,nq', [(1, 1000), (2, 77), (3, 1)])
def test_attention_with_fused_projections(nb, nq, fused_splits):
    """attention_kernel<4 or 8, QP, OP>: q projection in the prologue (decoder, transformer.py:192 with the packed in_proj of
    nn.MultiheadAttention: q = Wq(tgt + query_pos) * head_dim^-0.5) and out_proj in the epilogue as 8 per-head partial
    outputs that ln_reduce sums (+ bias + residual + LayerNorm, transformer.py:195-198), against fp64 torch."""
    from cotr_amd import _lib
    import torch.nn.functional as F
    lib = _lib.load_library()
    g = _g(nb * 1000 + nq)
    R = nb * nq
    x, x2 = torch.randn(R, 256, generator=g), torch.randn(R, 256, generator=g)
    wq, bq = torch.randn(256, 256, generator=g) / 16, 0.1 * torch.randn(256, generator=g)
    wo, bo = torch.randn(256, 256, generator=g) / 16, 0.1 * torch.randn(256, generator=g)
    kv = torch.randn(nb * 512, 512, generator=g)
    res = torch.randn(R, 256, generator=g)
    lw, lb = torch.rand(256, generator=g) + 0.5, 0.1 * torch.randn(256, generator=g)
    scale = 32 ** -0.5
    qd = ((x + x2).double() @ wq.double().t() + bq.double()) * scale
    qh = qd.view(nb, nq, 8, 32).permute(0, 2, 1, 3)
    kh = kv[:, :256].double().reshape(nb, 512, 8, 32).permute(0, 2, 1, 3)
    vh = kv[:, 256:].double().reshape(nb, 512, 8, 32).permute(0, 2, 1, 3)
    o_ref = (torch.softmax(qh @ kh.transpose(-1, -2), -1) @ vh).permute(0, 2, 1, 3).reshape(R, 256)
    proj_ref = o_ref @ wo.double().t()
    y_ref = F.layer_norm(res.double() + proj_ref + bo.double(), (256,), lw.double(), lb.double())
    d = G.dev()
    xd, x2d, wqd, bqd, wod, bod, kvd, resd, lwd, lbd = (t.to(d) for t in (x, x2, wq, bq, wo, bo, kv, res, lw, lb))
    o = torch.full((R, 256), float('nan'), device=d)
    part = torch.full((8, R, 256), float('nan'), device=d)
    y = torch.full((R, 256), float('nan'), device=d)
    none = None
    # (a) q projection only: o against the reference attention
    rc = lib.cotr_op_attention_fused(none, 0, G.P(xd), G.P(x2d), G.P(wqd), G.P(bqd), scale, G.P(kvd), G.P(kvd[:, 256:]), 512,
                                     G.P(o), 256, none, none, nb, nq, G.sptr())
    assert rc == 0
    assert G.rel_err(o, o_ref) < 2e-5
    # x alone / x2 alone (layer 0 of the decoder: tgt == 0)
    o1 = torch.full((R, 256), float('nan'), device=d)
    xs = (xd + x2d).contiguous()
    for xa, xb in ((xs, None), (None, xs)):
        assert lib.cotr_op_attention_fused(none, 0, G.P(xa), G.P(xb), G.P(wqd), G.P(bqd), scale, G.P(kvd), G.P(kvd[:, 256:]),
                                           512, G.P(o1), 256, none, none, nb, nq, G.sptr()) == 0
        assert torch.equal(o1, o)
    # (b) out projection only, q given: the partials sum to O . Wo^T; o is still written when asked for
    qf = qd.float().to(d)
    o2 = torch.full((R, 256), float('nan'), device=d)
    rc = lib.cotr_op_attention_fused(G.P(qf), 256, none, none, none, none, 0.0, G.P(kvd), G.P(kvd[:, 256:]), 512, G.P(o2), 256,
                                     G.P(wod), G.P(part), nb, nq, G.sptr())
    assert rc == 0
    assert G.rel_err(o2, o_ref) < 2e-5
    assert G.rel_err(part.double().sum(0), proj_ref) < 3e-5
    # (c) both + ln_reduce: the decoder's cross-attention sub-layer in two launches
    part.fill_(float('nan'))
    rc = lib.cotr_op_attention_fused(none, 0, G.P(xd), G.P(x2d), G.P(wqd), G.P(bqd), scale, G.P(kvd), G.P(kvd[:, 256:]), 512,
                                     none, 0, G.P(wod), G.P(part), nb, nq, G.sptr())
    assert rc == 0
    assert lib.cotr_op_ln_reduce(G.P(part), 8, G.P(bod), G.P(resd), G.P(lwd), G.P(lbd), G.P(y), R, G.sptr()) == 0
    assert G.rel_err(y, y_ref) < 3e-5
    assert lib.cotr_op_ln_reduce(G.P(part), 8, G.P(bod), none, G.P(lwd), G.P(lbd), G.P(y), R, G.sptr()) == 0   # no residual
    y0 = F.layer_norm(proj_ref + bo.double(), (256,), lw.double(), lb.double())
    assert G.rel_err(y, y0) < 3e-5
    # a NaN query row stays in its row (the engines test for NaN themselves, sparse_engine.py:54-55)
    if nq > 2:
        x2n = x2d.clone()
        x2n[1] = float('nan')
        assert lib.cotr_op_attention_fused(none, 0, G.P(xd), G.P(x2n), G.P(wqd), G.P(bqd), scale, G.P(kvd), G.P(kvd[:, 256:]), 512,
                                           G.P(o1), 256, G.P(wod), G.P(part), nb, nq, G.sptr()) == 0
        assert torch.isnan(o1[1]).all() and torch.isnan(part[:, 1]).all()
        keep = torch.arange(R, device=d) != 1
        assert torch.equal(o1[keep], o[keep]) and not torch.isnan(part[:, keep]).any()


@pytest.mark.parametrize('rows', [1001, 8192 + 13])
def test_layernorm(rows):
    """(the row after the last one must stay untouched)"""
    from cotr_amd import _lib
    g = _g(3)
    x = torch.randn(rows, 256, generator=g) * 3 + 1
    w, b = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g)
    ref = F.layer_norm(x, (256,), w, b, 1e-5)
    d = G.dev()
    y = torch.full((rows + 1, 256), 7.0, device=d)
    x_d, w_d, b_d = x.to(d), w.to(d), b.to(d)
    assert _lib.load_library().cotr_op_layernorm(G.P(x_d), G.P(w_d), G.P(b_d), G.P(y), rows, G.sptr()) == 0
    e = G.rel_err(y[:rows], ref)
    assert e < 5e-6, e
    assert bool((y[rows] == 7.0).all())


def test_lin_sine_encoding():
    from cotr_amd import _lib
    g = _g(4)
    pts = torch.rand(777, 2, generator=g) * 2 - 0.5        # includes out-of-range coordinates
    ref = torch.cat([torch.sin(i * math.pi * pts) for i in range(1, 65)] +
                    [torch.cos(i * math.pi * pts) for i in range(1, 65)], dim=-1)
    d = G.dev()
    y = torch.empty(777, 256, device=d)
    pts_d = pts.to(d)
    assert _lib.load_library().cotr_op_posenc(G.P(pts_d), G.P(y), 777, G.sptr()) == 0
    e = float((y.cpu() - ref).abs().max())
    assert e < 1e-6, e


@pytest.mark.parametrize('M', [1000, 512, 33, 4000])
def test_fused_ffn_block(M):
    """ffn.hip + ln_reduce: y = LayerNorm(x + linear2(relu(linear1(x)))) (transformer.py:156-158)."""
    from cotr_amd import _lib
    g = _g(M)
    x = torch.randn(M, 256, generator=g)
    w1, b1 = torch.randn(1024, 256, generator=g) / 16, torch.randn(1024, generator=g) * 0.1
    w2, b2 = torch.randn(256, 1024, generator=g) / 32, torch.randn(256, generator=g) * 0.1
    lw, lb = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.1
    ref = F.layer_norm(x + F.linear(F.relu(F.linear(x, w1, b1)), w2, b2), (256,), lw, lb, 1e-5)
    d = G.dev()
    lib = _lib.load_library()
    t = [v.to(d) for v in (x, w1, b1, w2, b2, lw, lb)]
    scratch = torch.empty(lib.cotr_op_ffn_chunks(M) * M * 256, device=d)
    y = torch.empty(M, 256, device=d)
    assert lib.cotr_op_ffn_block(*[G.P(v) for v in t], G.P(scratch), G.P(y), M, G.sptr()) == 0
    e = G.rel_err(y, ref)
    assert e < 2e-5, e


@pytest.mark.parametrize('M,post', [(64, False), (100, True), (8192, False), (20001, True)])
def test_ffn_rows_one_launch(M, post):
    """ffn_rows.hip: the whole block - linear1, ReLU, linear2, bias, residual, LayerNorm [, decoder.norm] - in ONE launch for many rows
    (transformer.py:156-158 / 199-201, :110-111); ragged last tile; the same launch twice gives the same bits."""
    from cotr_amd import _lib
    g = _g(M + 7)
    x = torch.randn(M, 256, generator=g)
    w1, b1 = torch.randn(1024, 256, generator=g) / 16, torch.randn(1024, generator=g) * 0.1
    w2, b2 = torch.randn(256, 1024, generator=g) / 32, torch.randn(256, generator=g) * 0.1
    lw, lb = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.1
    pw, pb = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.1
    ref = F.layer_norm(x.double() + F.linear(F.relu(F.linear(x.double(), w1.double(), b1.double())), w2.double(), b2.double()), (256,),
                       lw.double(), lb.double(), 1e-5)
    if post:
        ref = F.layer_norm(ref, (256,), pw.double(), pb.double(), 1e-5)
    d = G.dev()
    lib = _lib.load_library()
    t = [v.to(d) for v in (x, w1, b1, w2, b2, lw, lb)]
    pp = [pw.to(d), pb.to(d)] if post else [None, None]
    y = torch.full((M + 1, 256), 7.0, device=d)           # one guard row behind the output
    y2 = torch.empty(M, 256, device=d)
    assert lib.cotr_op_ffn_rows(*[G.P(v) for v in t], G.P(pp[0]), G.P(pp[1]), G.P(y), M, G.sptr()) == 0
    assert lib.cotr_op_ffn_rows(*[G.P(v) for v in t], G.P(pp[0]), G.P(pp[1]), G.P(y2), M, G.sptr()) == 0
    e = G.rel_err(y[:M], ref)
    assert e < 2e-5, e
    assert torch.equal(y[:M], y2)
    assert bool((y[M] == 7.0).all()), 'rows past M were written'
    # y must not alias x
    assert lib.cotr_op_ffn_rows(G.P(t[0]), *[G.P(v) for v in t[1:]], G.P(pp[0]), G.P(pp[1]), G.P(t[0]), M, G.sptr()) != 0


def test_ffn_rows_passes_nan_like_the_reference():
    """relu(NaN) = NaN in torch; a NaN row stays NaN, its neighbours are untouched (the engine raises on NaN, sparse_engine.py:54-55)."""
    from cotr_amd import _lib
    g = _g(3)
    M = 130
    x = torch.randn(M, 256, generator=g)
    x[65, 3] = float('nan')
    w1, b1 = torch.randn(1024, 256, generator=g) / 16, torch.randn(1024, generator=g) * 0.1
    w2, b2 = torch.randn(256, 1024, generator=g) / 32, torch.randn(256, generator=g) * 0.1
    lw, lb = torch.ones(256), torch.zeros(256)
    d = G.dev()
    t = [v.to(d) for v in (x, w1, b1, w2, b2, lw, lb)]
    y = torch.empty(M, 256, device=d)
    assert _lib.load_library().cotr_op_ffn_rows(*[G.P(v) for v in t], None, None, G.P(y), M, G.sptr()) == 0
    y = y.cpu()
    assert bool(torch.isnan(y[65]).all())
    assert not bool(torch.isnan(y[:65]).any()) and not bool(torch.isnan(y[66:]).any())


def _att_rows_ref(q, k, v, wo, bo, res, lw, lb, nb, nq):
    """fp64 reference: q [nb*nq, 256] (pre-scaled), k / v [nb*512, 256] -> LN(res + out_proj(MHA))."""
    qh = q.double().view(nb, nq, 8, 32).permute(0, 2, 1, 3)
    kh = k.double().view(nb, 512, 8, 32).permute(0, 2, 1, 3)
    vh = v.double().view(nb, 512, 8, 32).permute(0, 2, 1, 3)
    o = (torch.softmax(qh @ kh.transpose(-1, -2), dim=-1) @ vh).permute(0, 2, 1, 3).reshape(nb * nq, 256)
    y = F.linear(o, wo.double(), bo.double())
    if res is not None:
        y = y + res.double()
    return F.layer_norm(y, (256,), lw.double(), lb.double(), 1e-5)


@pytest.mark.parametrize('nb,nq,qp,with_x,with_res', [(2, 64, False, False, True), (3, 100, True, True, True), (2, 512, False, False, True),
                                                        (1, 1000, True, False, False), (5, 130, True, True, True)])
def test_att_rows_one_launch(nb, nq, qp, with_x, with_res):
    """att_rows.hip: [q projection,] 8-head attention over the pair's 512 keys, out projection, residual and LayerNorm in ONE launch
    (transformer.py:149-155 / 192-198); K / V are column slices of a wider matrix as in the hoisted decoder K/V cache; ragged last
    tile of a pair; the same launch twice gives the same bits."""
    from cotr_amd import _lib
    g = _g(nb * 1000 + nq)
    R = nb * nq
    scale = 32 ** -0.5
    kvw = torch.randn(nb * 512, 768, generator=g)           # [.. | K | V] columns: ldkv = 768, K at 256, V at 512
    k, v = kvw[:, 256:512], kvw[:, 512:768]
    wo, bo = torch.randn(256, 256, generator=g) / 16, torch.randn(256, generator=g) * 0.1
    lw, lb = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.1
    res = torch.randn(R, 256, generator=g) if with_res else None
    d = G.dev()
    lib = _lib.load_library()
    kvd = kvw.to(d)
    if qp:
        x2 = torch.randn(R, 256, generator=g)
        x = torch.randn(R, 256, generator=g) if with_x else None
        wq, bq = torch.randn(256, 256, generator=g) / 16, torch.randn(256, generator=g) * 0.1
        xin = x2.double() + (x.double() if x is not None else 0)
        q = (F.linear(xin, wq.double(), bq.double()) * scale).float()
        args_q = [None, 0, G.P(x.to(d)) if x is not None else None, None, None, None]
        keep = [x2.to(d), wq.to(d), bq.to(d)]
        args_q[3], args_q[4], args_q[5] = G.P(keep[0]), G.P(keep[1]), G.P(keep[2])
        if x is not None:
            keep.append(x.to(d))
            args_q[2] = G.P(keep[-1])
    else:
        qw = torch.randn(R, 768, generator=g) * 0.5           # q columns of a packed projection: ldq = 768
        q = qw[:, :256]
        keep = [qw.to(d)]
        args_q = [G.P(keep[0]), 768, None, None, None, None]
    ref = _att_rows_ref(q, k, v, wo, bo, res, lw, lb, nb, nq)
    t = [wo.to(d), bo.to(d), lw.to(d), lb.to(d)]
    resd = res.to(d) if res is not None else None
    y = torch.full((R + 1, 256), 7.0, device=d)
    y2 = torch.empty(R, 256, device=d)
    import ctypes
    kp = ctypes.c_void_p(kvd.data_ptr() + 256 * 4)
    vp = ctypes.c_void_p(kvd.data_ptr() + 512 * 4)
    for out in (y, y2):
        rc = lib.cotr_op_att_rows(*args_q, scale, kp, vp, 768, G.P(t[0]), G.P(t[1]), G.P(resd), G.P(t[2]), G.P(t[3]), G.P(out), nb, nq,
                                  G.sptr())
        assert rc == 0, rc
    e = G.rel_err(y[:R], ref)
    assert e < 2e-5, e
    assert torch.equal(y[:R], y2)
    assert bool((y[R] == 7.0).all()), 'rows past the last pair were written'


def test_att_rows_passes_nan_like_the_reference():
    """A NaN query row stays NaN through softmax, out projection and LayerNorm; its neighbours - same tile, same wavefronts - are
    untouched (the lazy softmax reference is raised by a wave-wide vote: a NaN lane must not poison the vote of the others)."""
    import ctypes
    from cotr_amd import _lib
    g = _g(11)
    nb, nq = 1, 130
    kvw = torch.randn(nb * 512, 768, generator=g)
    qw = torch.randn(nb * nq, 768, generator=g) * 0.5
    qw[70, 5] = float('nan')
    wo, bo = torch.randn(256, 256, generator=g) / 16, torch.zeros(256)
    lw, lb = torch.ones(256), torch.zeros(256)
    ref = _att_rows_ref(qw[:, :256], kvw[:, 256:512], kvw[:, 512:768], wo, bo, None, lw, lb, nb, nq)
    d = G.dev()
    t = [qw.to(d), kvw.to(d), wo.to(d), bo.to(d), lw.to(d), lb.to(d)]
    y = torch.empty(nb * nq, 256, device=d)
    rc = _lib.load_library().cotr_op_att_rows(G.P(t[0]), 768, None, None, None, None, 0.0, ctypes.c_void_p(t[1].data_ptr() + 1024),
                                              ctypes.c_void_p(t[1].data_ptr() + 2048), 768, G.P(t[2]), G.P(t[3]), None, G.P(t[4]), G.P(t[5]),
                                              G.P(y), nb, nq, G.sptr())
    assert rc == 0
    y = y.cpu()
    assert bool(torch.isnan(y[70]).all())
    ok = torch.ones(nb * nq, dtype=torch.bool)
    ok[70] = False
    assert not bool(torch.isnan(y[ok]).any())
    assert G.rel_err(y[ok], ref[ok]) < 2e-5


# ---- every launch configuration of the GEMM / implicit-GEMM kernels on the same problem -----------------------------
def _cfgs():
    """every GEMM configuration of the loaded library that takes fp32 operands (46 - 51 of the experimental library take packed
    split-f16 operands: tests/test_experimental_gpu.py)"""
    from cotr_amd import _lib
    return [c for c in range(_lib.load_library().cotr_gemm_num_configs()) if c not in (46, 47, 48, 49, 50, 51)]


def _accepts_fixture(test):
    """tests/golden/gemm_cfg_accepts.json (tests/golden/make_gemm_fixtures.py): the configurations that took each shape of the three
    tests below, recorded before the launch configurations became one table - keyed by cotr_is_experimental()"""
    import json
    import os
    from cotr_amd import _lib
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'gemm_cfg_accepts.json')) as f:
        return json.load(f)[str(_lib.load_library().cotr_is_experimental())][test]


def every_gemm_config_linear():
    """-> {shape: [configurations that ran]}; every one that ran is checked against torch"""
    from cotr_amd import _lib
    lib = _lib.load_library()
    d = G.dev()
    accepted = {}
    for M, N, K in [(1000, 256, 256), (300, 128, 64), (4133, 1024, 256)]:
        g = _g(M + N)
        x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
        b, r = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        ref = F.relu(F.linear(x, w, b) + r)
        xd, wd, bd, rd = x.to(d), w.to(d), b.to(d), r.to(d)
        for cfg in _cfgs():
            y = torch.full((M, N), float('nan'), device=d)
            rc = lib.cotr_op_linear_cfg(G.P(xd), G.P(wd), G.P(bd), G.P(rd), 1, G.P(y), M, N, K, cfg, G.sptr())
            if rc != 0:
                continue
            e = G.rel_err(y, ref)
            assert e < 2e-5, (cfg, M, N, K, e)
            accepted.setdefault(f'{M}x{N}x{K}', []).append(cfg)
    return accepted


def test_every_gemm_config_linear():
    """All configurations (spatial, k-split, LDS-DMA, large-tile) compute the same bias+residual+ReLU linear; a
    configuration may decline a shape (rc -1: tile does not divide N), never return a wrong result - and the set that takes
    each shape is the recorded one."""
    accepted = every_gemm_config_linear()
    assert sum(len(v) for v in accepted.values()) >= 60
    assert accepted == _accepts_fixture('linear')


def every_gemm_config_conv():
    from cotr_amd import _lib
    lib = _lib.load_library()
    d = G.dev()
    accepted = {}
    for B, H, cin, cout, k, stride in [(3, 16, 64, 128, 3, 1), (2, 16, 128, 256, 3, 2), (5, 8, 64, 256, 1, 1), (2, 32, 256, 128, 1, 2),
                                       (2, 32, 256, 64, 3, 1)]:   # (the last one also fits the input-patch variant, cfg 31)
        g = _g(B + H + cin + cout)
        x = torch.randn(B, cin, H, 2 * H, generator=g)
        w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
        sc, b = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
        conv = lambda t: F.conv2d(t, w, stride=stride, padding=k // 2)
        pre = G.per_half(conv, x) * sc.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
        res = torch.randn(pre.shape, generator=g)
        ref = F.relu(pre + res)
        xd, wd = G.nchw_to_sbs(x).to(d), G.pack_conv_weight(w).to(d)
        scd, bd, rd = sc.to(d), b.to(d), G.nchw_to_sbs(res).to(d)
        ho = ref.shape[2]
        for cfg in _cfgs():
            y = torch.full((B, ho, 2 * ho, cout), float('nan'), device=d)
            rc = lib.cotr_op_conv_cfg(G.P(xd), G.P(wd), G.P(scd), G.P(bd), G.P(rd), 1, G.P(y), B, H, H, cin, cout, k, stride,
                                      cfg, G.sptr())
            if rc != 0:
                continue
            e = G.rel_err(G.sbs_to_nchw(y.cpu()), ref)
            assert e < 3e-5, (cfg, B, H, cin, cout, k, stride, e)
            accepted.setdefault(f'{B},{H},{cin},{cout},{k},{stride}', []).append(cfg)
    return accepted


def test_every_gemm_config_conv():
    accepted = every_gemm_config_conv()
    assert sum(len(v) for v in accepted.values()) >= 80
    assert accepted == _accepts_fixture('conv')


@pytest.mark.parametrize('B,H,W', [(1, 16, 16), (3, 16, 16), (1, 16, 32), (1, 32, 64), (2, 8, 32)])
def test_conv3x3_input_patch_variant(B, H, W):
    """cfg 31: 3x3 stride-1 convolution over 256 channels with the input pixels of a 32-row output tile (one 32-pixel row segment,
    or on layer3's 16-wide halves the 16-pixel rows of both halves) loaded once (layer3's conv2 at few pairs, torchvision Bottleneck.conv2 + FrozenBatchNorm2d + ReLU): zero padding at the image
    border AND at the seam between the two halves, against torch per half; it declines what it is not written for."""
    from cotr_amd import _lib
    lib = _lib.load_library()
    cin, cout = 256, 256
    g = _g(B * 1000 + H * 10 + W)
    x = torch.randn(B, cin, H, 2 * W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    sc, b = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    pre = G.per_half(lambda t: F.conv2d(t, w, padding=1), x) * sc.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
    res = torch.randn(pre.shape, generator=g)
    ref = F.relu(pre + res)
    d = G.dev()
    xd, wd = G.nchw_to_sbs(x).to(d), G.pack_conv_weight(w).to(d)
    scd, bd, rd = sc.to(d), b.to(d), G.nchw_to_sbs(res).to(d)
    y = torch.full((B, H, 2 * W, cout), float('nan'), device=d)
    assert lib.cotr_op_conv_cfg(G.P(xd), G.P(wd), G.P(scd), G.P(bd), G.P(rd), 1, G.P(y), B, H, W, cin, cout, 3, 1, 31, G.sptr()) == 0
    assert G.rel_err(G.sbs_to_nchw(y.cpu()), ref) < 3e-5
    y30 = torch.full_like(y, float('nan'))
    assert lib.cotr_op_conv_cfg(G.P(xd), G.P(wd), G.P(scd), G.P(bd), G.P(rd), 1, G.P(y30), B, H, W, cin, cout, 3, 1, 30, G.sptr()) == 0
    assert torch.equal(y, y30)          # same contraction order per wavefront, same reduction: bit-identical to the 9-tile form
    # not its shape: stride 2, 1x1, 128 channels, a width that is not a multiple of 32
    for (ci, k, st, ww) in ((256, 3, 2, W), (256, 1, 1, W), (128, 3, 1, W), (256, 3, 1, 8)):
        xx = torch.zeros(1, H, 2 * ww, ci, device=d)
        wx = torch.zeros(cout, k * k * ci, device=d)
        yy = torch.zeros(1, H // st, 2 * (ww // st), cout, device=d)
        assert lib.cotr_op_conv_cfg(G.P(xx), G.P(wx), G.P(scd), G.P(bd), None, 1, G.P(yy), 1, H, ww, ci, cout, k, st, 31, G.sptr()) != 0


DUAL_CASES = [(1, 64, 64, 256, 64, 1), (1, 64, 256, 512, 128, 2), (1, 32, 512, 1024, 256, 2), (2, 16, 64, 256, 64, 2)]


def dual_conv_launch(B, H, cin, c_ds, c_1, stride):
    """-> the configurations that ran; both outputs of each against torch on CPU"""
    from cotr_amd import _lib
    lib = _lib.load_library()
    g = _g(B * 100 + H + cin)
    x = torch.randn(B, cin, H, 2 * H, generator=g)
    wd, w1 = torch.randn(c_ds, cin, 1, 1, generator=g) / math.sqrt(cin), torch.randn(c_1, cin, 1, 1, generator=g) / math.sqrt(cin)
    sd, bd = torch.rand(c_ds, generator=g) + 0.5, torch.randn(c_ds, generator=g)
    s1, b1 = torch.rand(c_1, generator=g) + 0.5, torch.randn(c_1, generator=g)
    ref_d = G.per_half(lambda t: F.conv2d(t, wd, stride=stride), x) * sd.view(1, -1, 1, 1) + bd.view(1, -1, 1, 1)
    ref_1 = F.relu(G.per_half(lambda t: F.conv2d(t, w1), x) * s1.view(1, -1, 1, 1) + b1.view(1, -1, 1, 1))
    d = G.dev()
    xd = G.nchw_to_sbs(x).to(d)
    wdd, w1d = G.pack_conv_weight(wd).to(d), G.pack_conv_weight(w1).to(d)
    sdd, bdd, s1d, b1d = sd.to(d), bd.to(d), s1.to(d), b1.to(d)
    ran = []
    for cfg in _cfgs():
        yd = torch.full((B, H // stride, 2 * H // stride, c_ds), float('nan'), device=d)
        y1 = torch.full((B, H, 2 * H, c_1), float('nan'), device=d)
        rc = lib.cotr_op_conv_dual_cfg(G.P(xd), G.P(wdd), G.P(sdd), G.P(bdd), 0, G.P(yd), c_ds, 1, stride,
                                       G.P(w1d), G.P(s1d), G.P(b1d), 1, G.P(y1), c_1, 1, 1, B, H, H, cin, cfg, G.sptr())
        if rc != 0:
            assert rc == -1, (cfg, rc)
            continue
        assert G.rel_err(G.sbs_to_nchw(yd.cpu()), ref_d) < 3e-5, cfg
        assert G.rel_err(G.sbs_to_nchw(y1.cpu()), ref_1) < 3e-5, cfg
        ran.append(cfg)
    return ran


@pytest.mark.parametrize('B,H,cin,c_ds,c_1,stride', DUAL_CASES)
def test_dual_conv_launch(B, H, cin, c_ds, c_1, stride):
    """Entry block of a ResNet stage: downsample (1x1, stride s, FrozenBN, no ReLU) and conv1 (1x1, stride 1, FrozenBN,
    ReLU) of the same input as ONE launch, under every configuration that has a dual form; a configuration may decline
    (rc -1), never return a wrong result - and the set that takes each shape is the recorded one."""
    ran = dual_conv_launch(B, H, cin, c_ds, c_1, stride)
    assert len(ran) >= 5, ran
    assert ran == _accepts_fixture('dual')[f'{B},{H},{cin},{c_ds},{c_1},{stride}']


@pytest.mark.parametrize('B,cin', [(1, 64), (1, 256), (3, 256), (2, 64)])
def test_fused_layer1_bottleneck(B, cin):
    """bottleneck.hip: conv1 1x1 -> conv2 3x3 -> conv3 1x1 (+ downsample 1x1 when cin == 64) with FrozenBN scale / bias, ReLU and
    the identity in ONE launch, against torchvision's Bottleneck.forward per 64-wide half (COTR/models/backbone.py:46-56,79-92):
    every tile's halo (conv2's zero padding applies to t1, also at the seam between the halves), every phase's MFMA layout, the
    packed weight fragments."""
    from cotr_amd import _lib
    lib = _lib.load_library()
    g = _g(B * 7 + cin)
    x = torch.randn(B, cin, 64, 128, generator=g)
    w1 = torch.randn(64, cin, 1, 1, generator=g) / math.sqrt(cin)
    w2 = torch.randn(64, 64, 3, 3, generator=g) / math.sqrt(576)
    w3 = torch.randn(256, 64, 1, 1, generator=g) / 8
    wd = torch.randn(256, 64, 1, 1, generator=g) / 8 if cin == 64 else None
    sb = lambda n: (torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g))
    (s1, b1), (s2, b2), (s3, b3), (sd, bd) = sb(64), sb(64), sb(256), sb(256)
    bn = lambda t, s_, b_: t * s_.view(1, -1, 1, 1) + b_.view(1, -1, 1, 1)

    def block(h):                                   # one 64 x 64 half, NCHW
        t1 = F.relu(bn(F.conv2d(h, w1), s1, b1))
        t2 = F.relu(bn(F.conv2d(t1, w2, padding=1), s2, b2))
        out = bn(F.conv2d(t2, w3), s3, b3)
        idt = bn(F.conv2d(h, wd), sd, bd) if wd is not None else h
        return F.relu(out + idt)
    ref = G.per_half(block, x)
    d = G.dev()
    xd = G.nchw_to_sbs(x).to(d)
    y = torch.full((B, 64, 128, 256), float('nan'), device=d)
    dv = lambda t: None if t is None else t.to(d)
    args = [dv(G.pack_conv_weight(w1)), dv(G.pack_conv_weight(w2)), dv(G.pack_conv_weight(w3)), dv(None if wd is None else G.pack_conv_weight(wd)),
            dv(s1), dv(b1), dv(s2), dv(b2), dv(s3), dv(b3), dv(sd if wd is not None else None), dv(bd if wd is not None else None)]
    rc = lib.cotr_op_bottleneck(G.P(xd), G.P(y), B, cin, *[G.P(a) for a in args], G.sptr())
    assert rc == 0
    torch.cuda.synchronize()
    e = G.rel_err(G.sbs_to_nchw(y.cpu()), ref)
    assert e < 3e-5, e
    # a shape it is not written for is declined, not mis-computed
    assert lib.cotr_op_bottleneck(G.P(xd), G.P(y), B, 128, *[G.P(a) for a in args], G.sptr()) != 0


@pytest.mark.parametrize('B', [1, 3, 8, 17])
def test_conv23_one_launch(B):
    """conv23.hip: conv2 3x3 (+ FrozenBN + ReLU) -> conv3 1x1 (+ FrozenBN + identity + ReLU) of a layer1 bottleneck in ONE launch,
    against torchvision's Bottleneck.forward per 64-wide half (COTR/models/backbone.py:46-56,79-92): the zero padding of every half's
    border rows / columns (also at the seam), the transposed first product handing its registers to the second, the W3 ring.  Also
    against the two launches it replaces (same contract; equal to fp32 rounding whatever configuration the table picks for them, and
    BIT for bit from 16 pairs on, where they run the large-tile configurations whose k order the kernel follows).  17 pairs: 2176
    workgroups = the staggered first round (blockIdx >> 8, three per CU) plus a ragged last one."""
    from cotr_amd import _lib
    lib = _lib.load_library()
    g = _g(B * 13 + 5)
    t1 = F.relu(torch.randn(B, 64, 64, 128, generator=g))
    w2 = torch.randn(64, 64, 3, 3, generator=g) / math.sqrt(576)
    w3 = torch.randn(256, 64, 1, 1, generator=g) / 8
    idt = torch.randn(B, 256, 64, 128, generator=g)
    sb = lambda n: (torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g))
    (s2, b2), (s3, b3) = sb(64), sb(256)
    bn = lambda t, s_, b_: t * s_.view(1, -1, 1, 1) + b_.view(1, -1, 1, 1)
    t2_ref = G.per_half(lambda h: F.relu(bn(F.conv2d(h, w2, padding=1), s2, b2)), t1)
    ref = F.relu(bn(F.conv2d(t2_ref, w3), s3, b3) + idt)
    d = G.dev()
    t1d, idtd = G.nchw_to_sbs(t1).to(d), G.nchw_to_sbs(idt).to(d)
    w2d, w3d = G.pack_conv_weight(w2).to(d), G.pack_conv_weight(w3).to(d)
    s2d, b2d, s3d, b3d = s2.to(d), b2.to(d), s3.to(d), b3.to(d)
    y = torch.full((B, 64, 128, 256), float('nan'), device=d)
    rc = lib.cotr_op_conv23(G.P(t1d), G.P(w2d), G.P(s2d), G.P(b2d), G.P(w3d), G.P(s3d), G.P(b3d), G.P(idtd), G.P(y), B, G.sptr())
    assert rc == 0
    torch.cuda.synchronize()
    e = G.rel_err(G.sbs_to_nchw(y.cpu()), ref)
    assert e < 3e-5, e
    t2 = G.op_conv(t1d, w2d, s2d, b2d, None, True, 64, 3, 1)
    y2 = G.op_conv(t2, w3d, s3d, b3d, idtd, True, 256, 1, 1)
    assert G.rel_err(y, y2) < 1e-5
    if B >= 16:
        assert torch.equal(y, y2)
    # NaN in, NaN out - where the reference has them (one pixel of t1 reaches its 3 x 3 neighbourhood of one half, every channel)
    t1n = t1d.clone()
    t1n[0, 10, 20, 3] = float('nan')
    assert lib.cotr_op_conv23(G.P(t1n), G.P(w2d), G.P(s2d), G.P(b2d), G.P(w3d), G.P(s3d), G.P(b3d), G.P(idtd), G.P(y), B, G.sptr()) == 0
    torch.cuda.synchronize()
    nan = torch.isnan(y)
    assert bool(nan[0, 9:12, 19:22, :].all()) and int(nan.sum()) == 9 * 256
    assert lib.cotr_op_conv23(G.P(t1d), G.P(w2d), G.P(s2d), G.P(b2d), G.P(w3d), G.P(s3d), G.P(b3d), None, G.P(y), B, G.sptr()) != 0


@pytest.mark.parametrize('M,n0,n1', [(128, 256, 64), (128 * 7, 256, 64), (128 * 3, 64, 0), (128 * 2, 128, 192)])
def test_expand_one_launch(M, n0, n1):
    """expand.hip: one or two 1x1 convolutions (K = 64) over the same x in one launch - FrozenBN scale / bias, ReLU per weight set
    (torchvision Bottleneck.forward with COTR/models/backbone.py:46-56: layer1 block 0's downsample branch and conv1): the rows kept in
    registers as the A operand, the W pieces through two LDS slots, two output tensors with different row pitch."""
    from cotr_amd import _lib
    lib = _lib.load_library()
    g = _g(M + n0 + n1)
    x = torch.randn(M, 64, generator=g)
    d = G.dev()
    sets, outs, refs = [], [], []
    for n, relu in ((n0, False), (n1, True)) if n1 else ((n0, True),):
        w = torch.randn(n, 64, generator=g) / 8
        sc, b = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g)
        ref = (x.double() @ w.double().t()) * sc.double() + b.double()
        refs.append((F.relu(ref) if relu else ref).float())
        y = torch.full((M, n), float('nan'), device=d)
        sets.append((w.to(d), sc.to(d), b.to(d), int(relu), y, n))
        outs.append(y)
    if len(sets) == 1:
        sets.append((None, None, None, 0, None, 0))
    xd = x.to(d)
    flat = []
    for w, sc, b, relu, y, n in sets:
        flat += [G.P(w), G.P(sc), G.P(b), relu, G.P(y), n]
    assert lib.cotr_op_expand(G.P(xd), M, *flat, G.sptr()) == 0
    torch.cuda.synchronize()
    for y, ref in zip(outs, refs):
        assert G.rel_err(y.cpu(), ref) < 2e-5
    # NaN in, NaN out - in that row of both outputs, nowhere else
    xn = xd.clone()
    xn[77, 5] = float('nan')
    assert lib.cotr_op_expand(G.P(xn), M, *flat, G.sptr()) == 0
    torch.cuda.synchronize()
    for y in outs:
        nan = torch.isnan(y)
        assert bool(nan[77].all()) and int(nan.sum()) == y.shape[1]
    # declined, not mis-computed: a row count that is not a multiple of the tile
    assert lib.cotr_op_expand(G.P(xd), M - 1, *flat, G.sptr()) != 0


@pytest.mark.parametrize('B,stride', [(1, 1), (3, 1), (2, 2), (16, 1), (17, 2)])
def test_conv23m_one_launch(B, stride):
    """conv23m.hip: conv2 3x3 (stride 1 / 2, + FrozenBN + ReLU) -> conv3 1x1 (+ FrozenBN + identity + ReLU) of a layer2 bottleneck in ONE
    launch, against torchvision's Bottleneck.forward per half (COTR/models/backbone.py:46-56,79-92) and against the two launches it
    replaces: the zero padding of every half's border (also at the seam), the strided taps of block 0, the W3 pieces through registers."""
    from cotr_amd import _lib
    lib = _lib.load_library()
    g = _g(B * 17 + stride)
    hin = 32 * stride
    t1 = F.relu(torch.randn(B, 128, hin, 2 * hin, generator=g))
    w2 = torch.randn(128, 128, 3, 3, generator=g) / math.sqrt(1152)
    w3 = torch.randn(512, 128, 1, 1, generator=g) / math.sqrt(128)
    idt = torch.randn(B, 512, 32, 64, generator=g)
    sb = lambda n: (torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g))
    (s2, b2), (s3, b3) = sb(128), sb(512)
    bn = lambda t, s_, b_: t * s_.view(1, -1, 1, 1) + b_.view(1, -1, 1, 1)
    t2_ref = G.per_half(lambda h: F.relu(bn(F.conv2d(h, w2, stride=stride, padding=1), s2, b2)), t1)
    ref = F.relu(bn(F.conv2d(t2_ref, w3), s3, b3) + idt)
    d = G.dev()
    t1d, idtd = G.nchw_to_sbs(t1).to(d), G.nchw_to_sbs(idt).to(d)
    w2d, w3d = G.pack_conv_weight(w2).to(d), G.pack_conv_weight(w3).to(d)
    s2d, b2d, s3d, b3d = s2.to(d), b2.to(d), s3.to(d), b3.to(d)
    y = torch.full((B, 32, 64, 512), float('nan'), device=d)
    rc = lib.cotr_op_conv23m(G.P(t1d), G.P(w2d), G.P(s2d), G.P(b2d), G.P(w3d), G.P(s3d), G.P(b3d), G.P(idtd), G.P(y), B, stride, G.sptr())
    assert rc == 0
    torch.cuda.synchronize()
    e = G.rel_err(G.sbs_to_nchw(y.cpu()), ref)
    assert e < 3e-5, e
    t2 = G.op_conv(t1d, w2d, s2d, b2d, None, True, 128, 3, stride)
    y2 = G.op_conv(t2, w3d, s3d, b3d, idtd, True, 512, 1, 1)
    assert G.rel_err(y, y2) < 1e-5
    if B >= 16:        # the staggered first round (two workgroups per CU, blockIdx >> 8) and the large-tile k order: the launches' bits
        assert torch.equal(y, y2)
    assert lib.cotr_op_conv23m(G.P(t1d), G.P(w2d), G.P(s2d), G.P(b2d), G.P(w3d), G.P(s3d), G.P(b3d), G.P(idtd), G.P(y), B, 3, G.sptr()) != 0


def test_large_tile_configs_are_repeatable():
    """The LDS-DMA kernels order other wavefronts' reads by an explicit vmcnt(0) before the barrier (common.h,
    LDS_DMA_WAIT_ALL); without it thousands of workgroups in flight produced rare stale tiles.  Many workgroups, several
    runs, bit-equal results, and equal to the register-staged configuration to rounding."""
    from cotr_amd import _lib
    lib = _lib.load_library()
    d = G.dev()
    g = _g(3)
    for M, N, K in [(65536, 512, 128), (131072, 64, 256)]:
        x, w = torch.randn(M, K, generator=g).to(d), (torch.randn(N, K, generator=g) / math.sqrt(K)).to(d)
        b, r = torch.randn(N, generator=g).to(d), torch.randn(M, N, generator=g).to(d)
        ref = torch.empty(M, N, device=d)
        assert lib.cotr_op_linear_cfg(G.P(x), G.P(w), G.P(b), G.P(r), 1, G.P(ref), M, N, K, 2, G.sptr()) == 0
        first = {}
        for cfg in (26, 27, 19, 20, 40, 41, 32, 35, 36):
            outs = []
            for _ in range(4):
                y = torch.full((M, N), float('nan'), device=d)
                rc = lib.cotr_op_linear_cfg(G.P(x), G.P(w), G.P(b), G.P(r), 1, G.P(y), M, N, K, cfg, G.sptr())
                if rc != 0:
                    break
                outs.append(y)
            if not outs:
                continue
            torch.cuda.synchronize()
            assert all(torch.equal(o, outs[0]) for o in outs[1:]), (cfg, M, N, K)
            assert G.rel_err(outs[0], ref) < 2e-5, (cfg, M, N, K)
            first[cfg] = outs[0]
        # the wave-specialised large tiles (4 loader + 4 MFMA wavefronts, 40 / 41) keep the tile decomposition and the k order of
        # 26 / 27: bit-identical results
        for ws, base in ((40, 26), (41, 27)):
            if ws in first and base in first:
                assert torch.equal(first[ws], first[base]), (ws, base, M, N, K)
