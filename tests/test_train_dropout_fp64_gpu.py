"""Op-level parity of the training kernels WITH DROPOUT ON (cotr_amd/csrc/train.hip, attention_train.hip through
cotr_amd/train_ops.py): forward values and every gradient against the same op in fp64 torch on the CPU, the dropout mask
applied there as the constant factor mask / (1 - p).

The mask is exact: tests/dropout_oracle.py restates the kernels' counter-based mask (hash, threshold, salt XOR, index
conventions, seed sequence) on the host, so the reference keeps and drops the very same elements, and the bars are the ones the
same ops are held to at p = 0 in tests/test_train_ops_gpu.py (attention and linear 2e-5 forward / 5e-5 gradients, AddDropLN
1e-5 / 3e-5): dropout removes terms and multiplies by a constant, it does not change a summation.  A wrong mask bit is far
outside them (test_one_flipped_mask_bit_is_seen), so the value comparison is also a bit-exact comparison of the mask indexing:
the hoisted per-row / per-tile hash of the second-form and one-pass attention kernels, the rows past nq of a ragged query tile,
the salt, the seed shared by forward and backward - and, at 2 x 525000 queries, the 32-bit carry of the hoisted index.

How the seed of an op is found: ``T.reseed(base)``, then the op draws ``dropout_oracle.seeds(base, 1)[0]``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cotr_amd import _lib
from cotr_amd import train_ops as T
from tests import dropout_oracle as D
from tests.test_train_bench_shape_gpu import _attention_kernels
from tests.test_train_ops_gpu import _g, _leaf, _leaf64, _rel

pytestmark = pytest.mark.gpu

SALT = 0x5bd1e995
SCALE = 32 ** -0.5


class _Salt:
    """Registers a dropout salt word for the block and clears it afterwards, whatever happens."""

    def __init__(self, on):
        self.on = on
        self.word = torch.full((1,), SALT, dtype=torch.int32, device='cuda') if on else None

    def __enter__(self):
        if self.on:
            assert _lib.load_library().cotr_train_set_dropout_salt(self.word.data_ptr()) == 0
        return SALT if self.on else None

    def __exit__(self, *a):
        torch.cuda.synchronize()
        _lib.load_library().cotr_train_set_dropout_salt(None)
        return False


def _factor(mask, p):
    """bool numpy mask -> fp64 tensor mask / (1 - p), with the kernels' float32 1 / (1 - p)."""
    return torch.from_numpy(mask).double() * D.inv_keep(p)


# ---- cotr_train_dropout_fwd -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_salt', [False, True])
@pytest.mark.parametrize('n', [4, 1028, 1 << 20])
def test_dropout_fwd_on_ones_is_the_host_mask(n, with_salt):
    """dropout_fwd_kernel on ones: (x > 0) is the host mask bit for bit, every kept value is 1 / (1 - p)."""
    lib = _lib.load_library()
    p, seed = 0.1, 777 + n
    x = torch.ones(n, device='cuda')
    with _Salt(with_salt) as salt:
        assert lib.cotr_train_dropout_fwd(x.data_ptr(), n, p, seed, _lib.current_stream_ptr()) == 0
    mask = D.keep(seed, np.arange(n, dtype=np.uint64), p, salt)
    x = x.cpu()
    assert np.array_equal((x > 0).numpy(), mask)
    kept = x[x > 0]
    assert torch.equal(kept, torch.full_like(kept, D.inv_keep(p)))
    assert abs(D.inv_keep(p) - 1 / (1 - p)) < 1.2e-7                       # (one float32 ulp at 1.11)
    assert torch.equal(x[x <= 0], torch.zeros(n - int(mask.sum())))
    if n >= 1024:
        assert 0 < int(mask.sum()) < n


def test_dropout_fwd_rejects_a_length_that_is_no_multiple_of_four():
    lib = _lib.load_library()
    x = torch.ones(1030, device='cuda')
    assert lib.cotr_train_dropout_fwd(x.data_ptr(), 1030, 0.1, 5, _lib.current_stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((x == 1).all())


# ---- AddDropLN --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [37, 1000])
@pytest.mark.parametrize('with_x', [True, False])
def test_residual_dropout_layernorm_forward_backward(rows, with_x):
    """add_drop_ln_fwd_kernel / ln_bwd_kernel at p = 0.1: y, dx, da, dw, db against LayerNorm(x + a * mask / (1 - p)) in fp64."""
    p, base = 0.1, 4000 + rows
    g = _g(rows)
    x, a = torch.randn(rows, 256, generator=g), torch.randn(rows, 256, generator=g) * 2 + 0.3
    w, b = torch.rand(256, generator=g) + 0.5, 0.1 * torch.randn(256, generator=g)
    dy = torch.randn(rows, 256, generator=g)
    xs = [_leaf(x) if with_x else None, _leaf(a), _leaf(w), _leaf(b)]
    T.reseed(base)
    y = T.AddDropLN.apply(xs[0], xs[1], xs[2], xs[3], p)
    grads = torch.autograd.grad(y, [t for t in xs if t is not None], dy.cuda())
    mask = D.flat_mask(D.seeds(base, 1)[0], rows, 256, p)
    assert 0.85 < mask.mean() < 0.95
    rs = [_leaf64(x) if with_x else None, _leaf64(a), _leaf64(w), _leaf64(b)]
    s = rs[1] * _factor(mask, p)
    s = s + rs[0] if with_x else s
    yr = F.layer_norm(s, (256,), rs[2], rs[3])
    refs = torch.autograd.grad(yr, [t for t in rs if t is not None], dy.double())
    errs = [_rel(y, yr)] + [_rel(got, want) for got, want in zip(grads, refs)]
    print(f'[AddDropLN rows {rows} with_x {with_x}] y {errs[0]:.2e}, gradients ' + ' '.join(f'{e:.2e}' for e in errs[1:]))
    assert errs[0] < 1e-5
    assert all(e < 3e-5 for e in errs[1:])
    # da is zero exactly where the mask drops
    da = grads[1 if with_x else 0].cpu()
    assert not bool(da[torch.from_numpy(~mask)].any())


# ---- Proj with ReLU and dropout ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N,K', [(777, 1024, 256), (48, 1024, 256)])
def test_linear_relu_dropout_forward_backward(M, N, K):
    """linear1 of the FFN at p = 0.25 (dropout_fwd_kernel on the GEMM's output, relu_drop_bwd_kernel with 1 / (1 - p)): y and
    dx, dw, db against relu(x w^T + b) * mask / (1 - p) in fp64.  The ReLU sign of the reference is the kernel's own, as in
    test_train_ops_gpu.py::test_linear_forward_backward (an element within rounding of zero may fall on either side) - read only
    where the HOST mask keeps the element, so that the forward mask is the host's and not the kernel's."""
    p, base = 0.25, 6000 + M
    g = _g(M + N + K)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    b, dy = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    xs = [_leaf(x), _leaf(w), _leaf(b)]
    T.reseed(base)
    y = T.linear(xs[0], xs[1], xs[2], relu=True, p=p)
    grads = torch.autograd.grad(y, xs, dy.cuda())
    mask = torch.from_numpy(D.flat_mask(D.seeds(base, 1)[0], M, N, p))
    yc = y.detach().cpu()
    rs = [_leaf64(x), _leaf64(w), _leaf64(b)]
    pre = F.linear(*rs)
    assert not bool((yc != 0)[~mask].any())                                # y != 0 implies the host mask keeps the element
    assert bool((yc > 0)[mask & (pre.detach() > 1e-4)].all())              # every kept, clearly positive element is there
    assert 0.7 < float(mask.double().mean()) < 0.8
    sign = (yc > 0) & mask
    yr = pre * sign.double() * D.inv_keep(p)
    refs = torch.autograd.grad(yr, rs, dy.double())
    errs = [_rel(y, yr)] + [_rel(got, want) for got, want in zip(grads, refs)]
    print(f'[linear relu dropout {M}x{N}x{K}] y {errs[0]:.2e}, gradients ' + ' '.join(f'{e:.2e}' for e in errs[1:]))
    assert errs[0] < 2e-5
    assert all(e < 5e-5 for e in errs[1:])


# ---- Attention --------------------------------------------------------------------------------------------------------
# (pairs, queries, layout): 'packed' = q|k the two halves of one [rows, 512] tensor (encoder), 'plain' = separate q, k, v,
# 'blocks' = k and v column blocks of one wide tensor (T.col_blocks: leading dimension 1024, gradients written in place),
# 'salt' = plain with a dropout salt word registered
ATT_CASES = [(2, 512, 'packed'), (1, 7, 'plain'), (3, 33, 'plain'), (3, 33, 'blocks'), (7, 40, 'plain'), (7, 40, 'salt'),
             (12, 64, 'plain'), (24, 256, 'plain')]
ATT_IDS = [f'{nb}x{nq}-{kind}' for nb, nq, kind in ATT_CASES]
ATT_P = 0.1
_att_refs = {}


def _att_inputs(nb, nq, qmul=2.0):
    g = _g(nb * 1000 + nq)
    q = torch.randn(nb * nq, 256, generator=g) * qmul
    k, v = torch.randn(nb * 512, 256, generator=g), torch.randn(nb * 512, 256, generator=g)
    d_o = torch.randn(nb * nq, 256, generator=g)
    return q, k, v, d_o


def _att_reference(q, k, v, d_o, nb, nq, mask, p, grads=True):
    """softmax(q k^T * scale) * mask / (1 - p) . v per head in fp64 -> (o, dq, dk, dv, probabilities)."""
    rq, rk, rv = _leaf64(q), _leaf64(k), _leaf64(v)
    qh = rq.view(nb, nq, 8, 32).permute(0, 2, 1, 3) * SCALE
    kh = rk.view(nb, 512, 8, 32).permute(0, 2, 1, 3)
    vh = rv.view(nb, 512, 8, 32).permute(0, 2, 1, 3)
    prob = torch.softmax(qh @ kh.transpose(-1, -2), -1)
    o = ((prob * _factor(mask, p)) @ vh).permute(0, 2, 1, 3).reshape(nb * nq, 256)
    if not grads:
        return o.detach(), None, None, None, prob.detach()
    gq, gk, gv = torch.autograd.grad(o, [rq, rk, rv], d_o.double())
    return o.detach(), gq, gk, gv, prob.detach()


def _att_base(nb, nq):
    return 31 * nb + nq


def _att_case(nb, nq, kind):
    """Inputs and fp64 reference of a case, computed once for the four forms."""
    key = (nb, nq, kind == 'salt')
    if key not in _att_refs:
        q, k, v, d_o = _att_inputs(nb, nq)
        mask = D.attention_mask(D.seeds(_att_base(nb, nq), 1)[0], nb, nq, ATT_P, SALT if kind == 'salt' else None)
        _att_refs[key] = (q, k, v, d_o) + _att_reference(q, k, v, d_o, nb, nq, mask, ATT_P)[:4]
    return _att_refs[key]


def _att_run(q, k, v, d_o, nb, nq, kind, base, p=ATT_P):
    """T.Attention forward + backward on the GPU -> (o, dq, dk, dv)."""
    T.reseed(base)
    with _Salt(kind == 'salt'):
        if kind == 'packed':
            qk, vv = _leaf(torch.cat([q, k], dim=1)), _leaf(v)
            o = T.Attention.apply(qk, None, None, vv, nb, nq, SCALE, p)
            dqk, dv = torch.autograd.grad(o, [qk, vv], d_o.cuda())
            return o.detach(), dqk[:, :256], dqk[:, 256:], dv
        if kind == 'blocks':
            junk = torch.full((nb * 512, 256), float('nan'))              # columns the attention must neither read nor write
            wide, qq = _leaf(torch.cat([k, v, junk, junk], dim=1)), _leaf(q)
            blocks = T.col_blocks(wide, 1, 4)[0]
            assert blocks[0].stride(0) == 1024
            o = T.Attention.apply(None, qq, blocks[0], blocks[1], nb, nq, SCALE, p)
            dq, dwide = torch.autograd.grad(o, [qq, wide], d_o.cuda())
            assert not bool(dwide[:, 512:].any())                           # the blocks nobody used: zero
            return o.detach(), dq, dwide[:, :256], dwide[:, 256:512]
        xs = [_leaf(q), _leaf(k), _leaf(v)]
        o = T.Attention.apply(None, xs[0], xs[1], xs[2], nb, nq, SCALE, p)
        return (o.detach(),) + tuple(torch.autograd.grad(o, xs, d_o.cuda()))


def test_attention_cases_reach_every_dropout_kernel():
    """Between them the cases x forms below launch every DROP instantiation: the first- and second-form forward and two-kernel
    backward, and the one-pass backward with the keys of a head over four, two and one workgroup(s)."""
    reached = set()
    for nb, nq, kind in ATT_CASES:
        for form in (0, 1, 2, 3):
            reached.update(_attention_kernels(form, nb, nq, kind == 'packed'))
    assert reached >= {'fwd1', 'fwd2', 'bwd1', 'bwd2', 'one-pass kt1', 'one-pass kt2', 'one-pass kt4'}, reached
    assert _attention_kernels(3, 2, 512, True)[1] == 'one-pass kt4' and _attention_kernels(3, 3, 33, False)[1] == 'one-pass kt1'
    assert _attention_kernels(0, 7, 40, False)[1] == 'one-pass kt1' and _attention_kernels(0, 12, 64, False)[1] == 'one-pass kt2'
    assert _attention_kernels(0, 24, 256, False)[1] == 'one-pass kt4'


@pytest.mark.parametrize('form', [0, 1, 2, 3])
@pytest.mark.parametrize('nb,nq,kind', ATT_CASES, ids=ATT_IDS)
def test_attention_dropout_forward_backward(nb, nq, kind, form):
    """attention at p = 0.1 under every train_attention_form: o, dq, dk, dv against the fp64 reference with the host mask."""
    q, k, v, d_o, o_ref, gq, gk, gv = _att_case(nb, nq, kind)
    _lib.set_knob('train_attention_form', form)
    o, dq, dk, dv = _att_run(q, k, v, d_o, nb, nq, kind, _att_base(nb, nq))
    errs = [_rel(o, o_ref), _rel(dq, gq), _rel(dk, gk), _rel(dv, gv)]
    print(f'[attention {nb}x{nq} {kind} form {form}: {_attention_kernels(form, nb, nq, kind == "packed")}] o {errs[0]:.2e}, '
          f'dq {errs[1]:.2e}, dk {errs[2]:.2e}, dv {errs[3]:.2e}')
    assert errs[0] < 2e-5
    assert all(e < 5e-5 for e in errs[1:])


@pytest.mark.parametrize('form', [1, 2])
def test_one_flipped_mask_bit_is_seen(form):
    """3 x 33 with q scaled by 0.1: the scores are within +-0.5 of each other, every probability within [0.5, 2] / 512, so that
    every single mask decision carries weight.  The kernel's o meets the forward bar against the host mask - and misses it by
    at least 10x against a reference with ONE decision flipped (a kept one, a dropped one, one in the ragged last tile)."""
    nb, nq, base = 3, 33, 4242
    q, k, v, d_o = _att_inputs(nb, nq, qmul=0.1)
    _lib.set_knob('train_attention_form', form)
    o = _att_run(q, k, v, d_o, nb, nq, 'plain', base)[0]
    mask = D.attention_mask(D.seeds(base, 1)[0], nb, nq, ATT_P)
    o_ref, _, _, _, prob = _att_reference(q, k, v, d_o, nb, nq, mask, ATT_P, grads=False)
    assert float(prob.min()) * 512 >= 0.5
    assert _rel(o, o_ref) < 2e-5
    kept, dropped = np.argwhere(mask), np.argwhere(~mask)
    last = np.argwhere(mask[:, :, 32:, :])[5] + np.array([0, 0, 32, 0])
    worst = float('inf')
    for where in (kept[0], kept[len(kept) // 2], dropped[0], dropped[-1], last):
        flipped = mask.copy()
        flipped[tuple(where)] ^= True
        off = _rel(o, _att_reference(q, k, v, d_o, nb, nq, flipped, ATT_P, grads=False)[0])
        worst = min(worst, off)
        assert off >= 10 * 2e-5, (tuple(where), off)
    print(f'[flipped mask bit, form {form}] the weakest of the five flips moves o by {worst:.2e} of its maximum')


# ---- the 32-bit carry of the hoisted mask index -----------------------------------------------------------------------
@pytest.mark.parametrize('form', [1, 2, 3])
def test_attention_mask_index_past_2_to_32(form):
    """2 pairs x 525000 queries: the mask index ((pair * 8 + head) * nq + qi) * 512 + key passes 2^32 inside pair 1, head 7, at
    query 513608 - where MaskTile::row switches to the constant of the next high word and mask_row takes a non-zero high word
    (form 2: the second-form kernels; form 3: the one-pass backward, keys over four workgroups; form 1: the plain 64-bit
    train_keep).  d_o is zero except for three windows of 96 queries (the start of pair 0, 48 either side of the crossing, the
    end of pair 1 - nq is no multiple of 32), so dS vanishes outside them: dk, dv and the windows' dq have a complete fp64
    reference from the 288 window rows, dq is exactly zero elsewhere, o is compared on the window rows."""
    nb, nq, p, base = 2, 525000, ATT_P, 8800
    cross = 513608
    assert ((1 * 8 + 7) * nq + cross) * 512 == 1 << 32 and nq % 32 != 0
    rows = nb * nq
    windows = [(0, 0), (1, cross - 48), (1, nq - 96)]                      # (pair, first query)
    win_rows = torch.cat([torch.arange(pr * nq + q0, pr * nq + q0 + 96) for pr, q0 in windows])
    g = torch.Generator(device='cuda').manual_seed(17)
    q = torch.randn(rows, 256, generator=g, device='cuda') * 2
    k, v = torch.randn(nb * 512, 256, generator=g, device='cuda'), torch.randn(nb * 512, 256, generator=g, device='cuda')
    d_win = torch.randn(288, 256, generator=g, device='cuda')
    d_o = torch.zeros(rows, 256, device='cuda')
    d_o[win_rows.cuda()] = d_win
    _lib.set_knob('train_attention_form', form)
    assert _attention_kernels(form, nb, nq, False) == {1: ('fwd1', 'bwd1'), 2: ('fwd2', 'bwd2'), 3: ('fwd2', 'one-pass kt1')}[form]
    xs = [q.requires_grad_(), k.requires_grad_(), v.requires_grad_()]
    T.reseed(base)
    o = T.Attention.apply(None, xs[0], xs[1], xs[2], nb, nq, SCALE, p)
    dq, dk, dv = torch.autograd.grad(o, xs, d_o)
    torch.cuda.synchronize()
    outside = torch.ones(rows, dtype=torch.bool, device='cuda')
    outside[win_rows.cuda()] = False
    assert int(((dq != 0).any(dim=1) & outside).sum()) == 0              # dq outside the windows: exactly zero, counted on the GPU
    assert int((dq != 0).any(dim=1).sum()) == 288
    assert bool(torch.isfinite(o).all())
    o_win, dq_win = o.detach()[win_rows.cuda()].cpu(), dq[win_rows.cuda()].cpu()
    # fp64 reference from the window rows: per window one "pair" of 96 queries against its pair's keys
    seed = D.seeds(base, 1)[0]
    qw = q.detach()[win_rows.cuda()].cpu()
    kw = torch.cat([k.detach().cpu()[pr * 512:(pr + 1) * 512] for pr, _ in windows])
    vw = torch.cat([v.detach().cpu()[pr * 512:(pr + 1) * 512] for pr, _ in windows])
    mask = np.concatenate([D.attention_mask(seed, 1, nq, p, pair0=pr, queries=np.arange(q0, q0 + 96)) for pr, q0 in windows])
    hi = D.attention_index(1, nq, pair0=1, queries=np.arange(cross - 48, cross + 48))[0, 7] >> np.uint64(32)
    assert hi[:48].max() == 0 and hi[48:].min() == 1                        # the window straddles the carry
    o_ref, gq, gk3, gv3, _ = _att_reference(qw, kw, vw, d_win.cpu(), 3, 96, mask, p)
    gk = torch.cat([gk3[:512], gk3[512:1024] + gk3[1024:]])                 # windows 1 and 2 share pair 1's keys
    gv = torch.cat([gv3[:512], gv3[512:1024] + gv3[1024:]])
    errs = [_rel(o_win, o_ref), _rel(dq_win, gq), _rel(dk, gk), _rel(dv, gv)]
    print(f'[attention 2x525000 form {form}] o {errs[0]:.2e}, dq {errs[1]:.2e}, dk {errs[2]:.2e}, dv {errs[3]:.2e}')
    assert errs[0] < 2e-5
    assert all(e < 5e-5 for e in errs[1:])
