"""Cases shared by tests/test_ffn_fused_loads_gpu.py, tests/test_gemm_epilogue_loads_gpu.py and the generator of their fixtures
(tests/golden/make_load_order_fixtures.py).  A change of WHERE a kernel's loads are issued and waited for (the epilogues of gemm_wp_body
and gemm_ks_body: done; ffn_fused_kernel: tried, not kept) leaves every floating-point operation and its order alone, so every output
must keep the bits the library produced before: the fixtures hold the sha256 of each output as recorded on the commit before the change.

Every output buffer carries one guard row of NaN behind its last row, hashed with it: nothing may be written past row M."""
import functools
import hashlib
import itertools
import math

import torch

from tests import gpu_helpers as G

# ---- fused FFN -------------------------------------------------------------------------------------------------------------------------
FFN_ROWS = [1, 31, 32, 33, 512, 1000]      # one row; the partial row tile around 32; the one-pair encoder / decoder row counts
FFN_CHUNKS = [2, 4, 8, 16]                 # knob ffn_fused_max_chunks: at M = 33 the workgroups walk 8, 4, 2, 1 sub-chunks of 64 hidden units
FFN_NAN_ROW = 17                           # (row 0 where M = 1 would leave nothing finite: M = 1 has no NaN row)


@functools.lru_cache(maxsize=None)
def ffn_inputs(M):
    """(x, w1, b1, w2, b2, ln_w, ln_b) on the CPU, seeded; row magnitudes of x spread over 1e-3 .. 1e3, elements over another decade,
    one NaN row (it must stay in its row).  Built once per row count, never written."""
    g = torch.Generator().manual_seed(9100 + M)
    x = torch.randn(M, 256, generator=g) * 10.0 ** (6 * torch.rand(M, 1, generator=g) - 3) * 10.0 ** (torch.rand(M, 256, generator=g) - 0.5)
    if M > FFN_NAN_ROW:
        x[FFN_NAN_ROW] = float('nan')
    w1, b1 = torch.randn(1024, 256, generator=g) / 16, torch.randn(1024, generator=g) * 0.1
    w2, b2 = torch.randn(256, 1024, generator=g) / 32, torch.randn(256, generator=g) * 0.1
    lw, lb = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.1
    return x, w1, b1, w2, b2, lw, lb


@functools.lru_cache(maxsize=None)
def ffn_inputs_dev(M):
    return tuple(t.to(G.dev()) for t in ffn_inputs(M))


@functools.lru_cache(maxsize=None)
def ffn_reference(M):
    """fp64 evaluation of LayerNorm(x + linear2(relu(linear1(x)))) (transformer.py:156-158)"""
    x, w1, b1, w2, b2, lw, lb = (t.double() for t in ffn_inputs(M))
    F = torch.nn.functional
    return F.layer_norm(x + F.linear(F.relu(F.linear(x, w1, b1)), w2, b2), (256,), lw, lb, 1e-5)


def ffn_run(M, max_chunks):
    """-> (y [M + 1][256] with the guard row, number of hidden-unit chunks the launch used)"""
    from cotr_amd import _lib
    lib = _lib.load_library()
    _lib.set_knob('ffn_fused_max_chunks', max_chunks)
    try:
        t = ffn_inputs_dev(M)
        nch = lib.cotr_op_ffn_chunks(M)
        scratch = torch.empty(nch * M * 256, device=G.dev())
        y = torch.full((M + 1, 256), float('nan'), device=G.dev())
        rc = lib.cotr_op_ffn_block(*[G.P(v) for v in t], G.P(scratch), G.P(y), M, G.sptr())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return y, nch
    finally:
        _lib.reset_knobs()


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


# ---- GEMM epilogues ---------------------------------------------------------------------------------------------------------------------
# the k-split (4, 24, 25, 30, 31) and wave-private (32 - 39) configurations of the one-pair forward
GEMM_CFGS = [4, 24, 25, 30, 31] + list(range(32, 40))
LINEAR_SHAPES = [(M, 256, K) for M in (1, 33, 1000) for K in (128, 1024)]
# cotr_op_linear_cfg takes bias / residual / relu, cotr_op_conv_cfg scale / bias / residual / relu (colscale_n and res_row_mod have no
# op-level entry; the forward's own fixtures cover them): every combination of what the entry takes
LINEAR_COMBOS = list(itertools.product((0, 1), repeat=3))
CONV_SHAPES = [(1, 16, 256, 256, 3, 1), (1, 16, 256, 512, 1, 2)]     # (B, H = W of a half, Cin, Cout, k, stride): a 16 x 32 pair
CONV_COMBOS = list(itertools.product((0, 1), repeat=4))


def _spread(g, *shape):
    """normal values with magnitudes spread over two decades: a changed order of the epilogue's operations changes the bits"""
    return torch.randn(*shape, generator=g) * 10.0 ** (2 * torch.rand(*shape, generator=g) - 1)


@functools.lru_cache(maxsize=None)
def linear_inputs_dev(M, N, K):
    g = torch.Generator().manual_seed(9200 + M + K)
    x, w = _spread(g, M, K), torch.randn(N, K, generator=g) / math.sqrt(K)
    b, r = _spread(g, N), _spread(g, M, N)
    return tuple(t.to(G.dev()) for t in (x, w, b, r))


@functools.lru_cache(maxsize=None)
def conv_inputs_dev(B, H, cin, cout, k, stride):
    g = torch.Generator().manual_seed(9300 + cin + cout + k)
    ho = (H + 2 * (k // 2) - k) // stride + 1
    x = _spread(g, B, H, 2 * H, cin)
    w = torch.randn(cout, k, k, cin, generator=g) / math.sqrt(cin * k * k)
    sc, b = torch.rand(cout, generator=g) + 0.5, _spread(g, cout)
    r = _spread(g, B, ho, 2 * ho, cout)
    return tuple(t.to(G.dev()) for t in (x, w, sc, b, r)) + (ho,)


def gemm_run(cfg):
    """Every case of one configuration -> {case: sha256 of the output with its guard row, or 'refused'}"""
    from cotr_amd import _lib
    lib = _lib.load_library()
    out = {}
    for (M, N, K), (has_b, has_r, relu) in itertools.product(LINEAR_SHAPES, LINEAR_COMBOS):
        x, w, b, r = linear_inputs_dev(M, N, K)
        y = torch.full((M + 1, N), float('nan'), device=G.dev())
        rc = lib.cotr_op_linear_cfg(G.P(x), G.P(w), G.P(b if has_b else None), G.P(r if has_r else None), relu, G.P(y), M, N, K, cfg,
                                    G.sptr())
        torch.cuda.synchronize()
        out[f'linear {M}x{N}x{K} bias{has_b} res{has_r} relu{relu}'] = sha(y) if rc == 0 else 'refused'
    for (B, H, cin, cout, k, stride), (has_s, has_b, has_r, relu) in itertools.product(CONV_SHAPES, CONV_COMBOS):
        x, w, sc, b, r, ho = conv_inputs_dev(B, H, cin, cout, k, stride)
        y = torch.full((B * ho * 2 * ho + 1, cout), float('nan'), device=G.dev())
        rc = lib.cotr_op_conv_cfg(G.P(x), G.P(w), G.P(sc if has_s else None), G.P(b if has_b else None), G.P(r if has_r else None), relu,
                                  G.P(y), B, H, H, cin, cout, k, stride, cfg, G.sptr())
        torch.cuda.synchronize()
        out[f'conv {B},{H},{cin},{cout},{k},{stride} scale{has_s} bias{has_b} res{has_r} relu{relu}'] = sha(y) if rc == 0 else 'refused'
    return out
