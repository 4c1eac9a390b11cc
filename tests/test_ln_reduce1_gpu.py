"""ln_reduce1.hip (what the forward path launches for 8 and 16 partial slabs: cotr_op_ln_reduce1) against ln_reduce_kernel
(pointwise.hip: cotr_op_ln_reduce), bit for bit: same sums in the same order, same wave-sum pairing, so torch.equal - at row counts
that include the ragged last workgroup (4 rows per workgroup), with and without the residual, with and without the second LayerNorm
(decoder.norm inside the last decoder layer's launch: cotr_op_ln_reduce_post, form 0 = ln_reduce_kernel, 1 = the forward path's),
and at slab counts ln_reduce1.hip does not take (the forward path's launcher then runs ln_reduce_kernel itself).
The slabs' magnitudes are spread over 1e-3 .. 1e3 (per slab and per element), so a changed sum order changes the bits."""
import functools

import pytest
import torch

from cotr_amd import _lib
from tests import gpu_helpers as G

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 4, 5, 512, 1000, 1001]
MAX_NP = 16


@functools.lru_cache(maxsize=None)
def _inputs(rows):
    """(parts [16][rows][256], bias, residual, w, b, post_w, post_b) on the device, seeded; built once per row count, never written"""
    g = torch.Generator().manual_seed(8100 + rows)
    slab_mag = 10.0 ** torch.linspace(-3, 3, MAX_NP)[torch.randperm(MAX_NP, generator=g)]
    elem_mag = 10.0 ** (torch.rand(MAX_NP, rows, 256, generator=g) - 0.5)
    parts = torch.randn(MAX_NP, rows, 256, generator=g) * elem_mag * slab_mag[:, None, None]
    bias = 0.1 * torch.randn(256, generator=g)
    res = torch.randn(rows, 256, generator=g) * 10.0 ** (2 * torch.rand(rows, 1, generator=g) - 1)
    w, b = torch.rand(256, generator=g) + 0.5, 0.1 * torch.randn(256, generator=g)
    pw, pb = torch.rand(256, generator=g) + 0.5, 0.1 * torch.randn(256, generator=g)
    return tuple(t.to(G.dev()) for t in (parts, bias, res, w, b, pw, pb))


def _slabs(parts, np_, rows):
    """the first np_ slabs as a contiguous [np_][rows][256] (the slab stride of a launch is rows * 256)"""
    return parts[:np_].contiguous()


@pytest.mark.parametrize('with_res', [True, False], ids=['res', 'nores'])
@pytest.mark.parametrize('np_', [8, 16, 1, 7, 9])
@pytest.mark.parametrize('rows', ROWS)
def test_ln_reduce1_equals_ln_reduce(rows, np_, with_res):
    lib = _lib.load_library()
    parts, bias, res, w, b, _, _ = _inputs(rows)
    p = _slabs(parts, np_, rows)
    r = res if with_res else None
    y0 = torch.full((rows + 1, 256), float('nan'), device=G.dev())   # one guard row: nothing may be written past the last row
    y1 = torch.full((rows + 1, 256), float('nan'), device=G.dev())
    assert lib.cotr_op_ln_reduce(G.P(p), np_, G.P(bias), G.P(r), G.P(w), G.P(b), G.P(y0), rows, G.sptr()) == 0
    assert lib.cotr_op_ln_reduce1(G.P(p), np_, G.P(bias), G.P(r), G.P(w), G.P(b), G.P(y1), rows, G.sptr()) == 0
    assert torch.isfinite(y0[:rows]).all()
    assert torch.equal(y1[:rows], y0[:rows])
    assert torch.isnan(y0[rows]).all() and torch.isnan(y1[rows]).all()
    # and it is the LayerNorm of the sum (fp64).  The bound comes from the sum, not the kernel: 17 fp32 adds of partial sums up to
    # ~1e4 (6e-4 absolute each at worst) against a row spread of ~1e3 that the norm divides by -> 1e-5 of an output of order 1
    x = p.double().sum(0) + bias.double() + (r.double() if with_res else 0)
    ref = torch.nn.functional.layer_norm(x, (256,), w.double(), b.double())
    assert G.rel_err(y1[:rows], ref) < 1e-4


@pytest.mark.parametrize('with_res', [True, False], ids=['res', 'nores'])
@pytest.mark.parametrize('np_', [8, 16, 7])
@pytest.mark.parametrize('rows', [1, 5, 1000, 1001])
def test_ln_reduce1_post_norm_equals_ln_reduce(rows, np_, with_res):
    """the launch that also applies decoder.norm (np = 16 at one pair in the forward; 8 and the fallback for completeness)"""
    lib = _lib.load_library()
    parts, bias, res, w, b, pw, pb = _inputs(rows)
    p = _slabs(parts, np_, rows)
    r = res if with_res else None
    ys = []
    for form in (0, 1):
        y = torch.full((rows + 1, 256), float('nan'), device=G.dev())
        assert lib.cotr_op_ln_reduce_post(G.P(p), np_, G.P(bias), G.P(r), G.P(w), G.P(b), G.P(pw), G.P(pb), G.P(y), rows, form,
                                          G.sptr()) == 0
        ys.append(y)
    assert torch.isfinite(ys[0][:rows]).all()
    assert torch.equal(ys[1][:rows], ys[0][:rows])
    assert torch.isnan(ys[0][rows]).all() and torch.isnan(ys[1][rows]).all()
    # without the post-norm pointers the entry is cotr_op_ln_reduce / cotr_op_ln_reduce1
    y2 = torch.full((rows, 256), float('nan'), device=G.dev())
    y3 = torch.full((rows, 256), float('nan'), device=G.dev())
    assert lib.cotr_op_ln_reduce_post(G.P(p), np_, G.P(bias), G.P(r), G.P(w), G.P(b), None, None, G.P(y2), rows, 1, G.sptr()) == 0
    assert lib.cotr_op_ln_reduce(G.P(p), np_, G.P(bias), G.P(r), G.P(w), G.P(b), G.P(y3), rows, G.sptr()) == 0
    assert torch.equal(y2, y3)
    x = torch.nn.functional.layer_norm(y3.double(), (256,), pw.double(), pb.double())
    assert G.rel_err(ys[1][:rows], x) < 1e-5


def test_ln_reduce1_rejects_bad_arguments():
    lib = _lib.load_library()
    parts, bias, res, w, b, pw, _ = _inputs(4)
    y = torch.zeros(4, 256, device=G.dev())
    assert lib.cotr_op_ln_reduce1(None, 8, G.P(bias), None, G.P(w), G.P(b), G.P(y), 4, G.sptr()) != 0
    assert lib.cotr_op_ln_reduce1(G.P(parts), 0, G.P(bias), None, G.P(w), G.P(b), G.P(y), 4, G.sptr()) != 0
    assert lib.cotr_op_ln_reduce_post(G.P(parts), 8, G.P(bias), None, G.P(w), G.P(b), G.P(pw), None, G.P(y), 4, 1, G.sptr()) != 0
    assert lib.cotr_op_ln_reduce_post(G.P(parts), 8, G.P(bias), None, G.P(w), G.P(b), None, None, G.P(y), 4, 2, G.sptr()) != 0
