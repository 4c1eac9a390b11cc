"""The whole training step WITH DROPOUT 0.1 (what every real step and bench.py --workload train run) against the fp64 oracle
with the same masks: loss, prediction and every gradient.

The oracle (oracle/cotr_oracle.py, oracle/train_oracle.py) takes a dropout hook; the hook here builds each site's mask on the
host (tests/dropout_oracle.py) from the seed that site drew on the GPU - ``train_ops.next_seed`` is recorded, and the recorded
sequence must be the restated one, four seeds per layer in the order attention probabilities, dropout before the first norm,
FFN hidden, dropout before the last norm - and maps the oracle's tensor layouts onto the kernels' row-major element indices:

    attention probabilities [B*8, Lq, 512], row b*8 + h      ->  ((pair * 8 + h) * Lq + q) * 512 + key
    [L, B, E] sequence-first (E = 256, or 1024 in the FFN)   ->  (pair * L + l) * E + e
    pair = the pair's index in the batch the KERNEL saw: compute_loss encodes both passes as one batch of 2B pairs, so the
    cycle pass's encoder rows are pairs B .. 2B-1 under the same 24 seeds; each decode is a call of its own with its own 24.

Bars: the per-tensor rule of tests/test_train_bench_shape_gpu.py - max(1e-3, 4 x the fp32 oracle's gap to fp64) on the norm,
max(1e-2, 4 x gap) on the maximum, the fp32 oracle under the same masks.  Cases: ``train_case(SEED, 2, 24)``, stage 1 (the
default: backbone frozen).

Measured on the MI355X: every gradient within 1e-6 of its norm (0.001 of the bar) in the compute_loss steps and in forward_train
under form 1; under forms 0, 2 and 3 forward_train has ONE hidden unit of encoder layer 5's FFN within rounding of zero on the other
side of the ReLU than in fp64 - linear1.weight / .bias of that layer 7.9e-5 of the norm (5e-4 of the maximum, one element), the
tensors upstream of it 3.7e-5: 0.08 of the bar, the same effect tests/test_train_ops_gpu.py describes for the ReLU at p = 0."""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cotr_amd
from cotr_amd import _lib, training
from cotr_amd import train_ops as T
from cotr_amd.models import build_model
from oracle import cotr_oracle
from oracle.train_oracle import train_loss_and_grads
from tests import dropout_oracle as D
from tests.golden.make_train_golden import train_case
from tests.test_train_bench_shape_gpu import FAMILIES, _bars, _errors, _family

pytestmark = pytest.mark.gpu

B, Q, P = 2, 24, 0.1
SEED = 0                      # of train_case: see test_step_case_is_well_posed
BASE = 1234                   # of the dropout seed sequence
SALT = 0x5bd1e995
KINDS = ('attn', 'drop1', 'ffn', 'drop2')
TOK = 512


class Masks:
    """The oracle's dropout hook for one step.  ``seeds``: what the step's sites drew, in order; ``whole``: a compute_loss step
    (encoder over 2B pairs, two decodes) or one forward_train (encoder, decoder)."""

    def __init__(self, seeds, whole, salt=None):
        assert len(seeds) == (72 if whole else 48)
        self.seeds, self.whole, self.salt, self.cache, self.sites = list(seeds), whole, salt, {}, []

    def seed_and_pair(self, site):
        parts = site.split('.')
        which, lo = ('pred', 0) if len(parts) == 3 else (parts[0], int(parts[1]))
        part, layer, kind = parts[-3], int(parts[-2]), KINDS.index(parts[-1])
        assert part in ('encoder', 'decoder') and which in ('pred', 'cycle') and (self.whole or which == 'pred')
        if part == 'encoder':
            return self.seeds[4 * layer + kind], lo + (B if which == 'cycle' else 0)
        return self.seeds[24 + (24 if which == 'cycle' else 0) + 4 * layer + kind], lo

    def __call__(self, site, t):
        key = (site, tuple(t.shape))
        if key not in self.cache:
            self.sites.append(site)
            seed, pair0 = self.seed_and_pair(site)
            if site.endswith('.attn'):
                bh, lq, lk = t.shape
                assert lk == TOK and bh % 8 == 0
                m = D.attention_mask(seed, bh // 8, lq, P, self.salt, pair0).reshape(bh, lq, lk)
            else:
                length, nb, e = t.shape
                m = D.flat_mask(seed, nb * length, e, P, self.salt, row0=pair0 * length).reshape(nb, length, e).transpose(1, 0, 2)
            self.cache[key] = torch.from_numpy(np.ascontiguousarray(m))
        return t * (self.cache[key].to(t.dtype) * D.inv_keep(P))


def _names():
    m = build_model(cotr_amd.default_args())
    assert float(m.transformer.encoder.layers[0].self_attn.dropout) == P
    return [n for n, p in m.named_parameters() if p.requires_grad]


def _forward_oracle(sd, img, query, target, names, hook, dtype):
    """mse(f(img, query), target) of the oracle with the hook's masks and its gradients -> (loss, pred, {name: grad})."""
    sd = {k: v.detach().to(dtype) for k, v in sd.items()}
    params = [sd[n].requires_grad_() for n in names]
    pred = cotr_oracle.cotr_forward_grad(sd, img.to(dtype), query.to(dtype), dtype=dtype, dropout=hook)
    loss = F.mse_loss(pred, target.to(dtype))
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    return float(loss.detach()), pred.detach(), {n: g for n, g in zip(names, grads) if g is not None}


class Reference:
    """fp64 and fp32 oracle of one case under the masks of the seed sequence ``D.seeds(BASE, ...)``."""

    def __init__(self, whole, salt):
        t0 = time.time()
        self.case = train_case(SEED, B, Q)
        sd, img, query, target = self.case
        self.names = _names()
        self.hook = Masks(D.seeds(BASE, 72 if whole else 48), whole, salt)
        if whole:
            r64 = train_loss_and_grads(sd, img, query, target, self.names, pairs_per_chunk=B, dropout=self.hook)
            r32 = train_loss_and_grads(sd, img, query, target, self.names, dtype=torch.float32, pairs_per_chunk=B, dropout=self.hook)
            assert torch.equal(r32.mask, r64.mask)
            self.loss, self.pred, self.grads, self.mask, self.margin = r64.loss, r64.pred, r64.grads, r64.mask, r64.margin
            loss32, grads32 = r32.loss, r32.grads
        else:
            self.loss, self.pred, self.grads = _forward_oracle(sd, img, query, target, self.names, self.hook, torch.float64)
            loss32, _, grads32 = _forward_oracle(sd, img, query, target, self.names, self.hook, torch.float32)
            self.mask = self.margin = None
        assert len(self.hook.sites) == (96 if whole else 48) and len(set(self.hook.sites)) == len(self.hook.sites)
        assert grads32.keys() == self.grads.keys()
        self.loss_bar = max(1e-5, 4 * abs(loss32 - self.loss) / self.loss)
        self.bars = _bars(grads32, self.grads)
        print(f'[reference {"compute_loss" if whole else "forward_train"} {B}x{Q} salt {salt}] fp64 + fp32 oracle '
              f'{time.time() - t0:.1f} s; loss {self.loss:.6f}, fp32 gap {abs(loss32 - self.loss) / self.loss:.1e}; margin {self.margin}')

    def check(self, label, loss, pred, cycle, grads):
        assert abs(loss - self.loss) <= self.loss_bar * self.loss, (label, loss, self.loss)
        assert cotr_oracle.px_err(pred.detach().cpu(), self.pred) < 1e-3, label
        if cycle is not None:
            mask = torch.norm(cycle.detach().double().cpu() - self.case[2].double(), dim=-1) < 10 / 256
            assert torch.equal(mask, self.mask), label
        reached = [n for n in self.names if n in self.grads]
        assert reached == [n for n in self.names if not ('decoder' in n and '.norm1.' in n)]    # the forward never applies norm1
        worst, bad = dict.fromkeys(FAMILIES, 0.0), []
        for n in reached:
            assert grads.get(n) is not None, (label, n)
            assert bool(torch.isfinite(grads[n]).all()), (label, n, 'not finite')
            e_norm, e_max = _errors(grads[n], self.grads[n])
            r = max(e_norm / self.bars[n][0], e_max / self.bars[n][1])
            worst[_family(n)] = max(worst[_family(n)], r)
            if not r <= 1:
                bad.append((n, e_norm, self.bars[n][0], e_max, self.bars[n][1]))
        for n in set(self.names) - set(reached):
            assert grads.get(n) is None or not grads[n].any(), (label, n)
        print(f'[{label}] loss error/bar {abs(loss - self.loss) / self.loss / self.loss_bar:.3f}; worst gradient error/bar: '
              + ', '.join(f'{f} {worst[f]:.3f}' for f in FAMILIES if f in {_family(n) for n in reached}))
        assert not bad, (label, bad[:8])


@pytest.fixture(scope='module')
def reference():
    """The CPU oracles, each computed once for the module."""
    cache = {}

    def get(whole, salt=None):
        if (whole, salt) not in cache:
            cache[(whole, salt)] = Reference(whole, salt)
        return cache[(whole, salt)]
    return get


def _record_seeds(monkeypatch):
    """train_ops.next_seed hands out what it did, and notes who asked: (seed, site kind, size) - size = (pairs, queries) for the
    attention probabilities, rows for the others."""
    drawn = []
    real = T.next_seed
    codes = {T.Attention.forward.__code__: 'attn', T.AddDropLN.forward.__code__: 'ln', T.Proj.forward.__code__: 'ffn'}

    def recording():
        import sys
        seed = real()
        frame = sys._getframe(1)
        kind = codes[frame.f_code]
        loc = frame.f_locals
        size = (loc['nb'], loc['nq']) if kind == 'attn' else loc['rows'] if kind == 'ln' else loc['ys'][0].shape[0]
        drawn.append((seed, kind, size))
        return seed
    monkeypatch.setattr(T, 'next_seed', recording)
    return drawn


def _expected_sites(whole):
    def layers(nb, nq):
        return [('attn', (nb, nq)), ('ln', nb * nq), ('ffn', nb * nq), ('ln', nb * nq)] * 6
    if whole:
        return layers(2 * B, TOK) + layers(B, Q) + layers(B, Q)
    return layers(B, TOK) + layers(B, Q)


def _hip_step(ref, whole, salt, monkeypatch):
    """One HIP step at dropout 0.1 under the seed sequence of BASE -> (loss, pred, cycle or None, {name: grad}); asserts the
    seeds it drew: their values (the restated sequence), their number and the sites' order."""
    sd, img, query, target = ref.case
    m = build_model(cotr_amd.default_args()).cuda().train()
    m.load_state_dict(sd)
    img, query, target = img.cuda(), query.cuda(), target.cuda()
    drawn = _record_seeds(monkeypatch)
    cycles = []
    decode = training.decode_train

    def recording(*a, **k):
        cycles.append(decode(*a, **k))
        return cycles[-1]
    monkeypatch.setattr(training, 'decode_train', recording)
    word = torch.full((1,), SALT, dtype=torch.int32, device='cuda')
    lib = _lib.load_library()
    try:
        if salt is not None:
            assert lib.cotr_train_set_dropout_salt(word.data_ptr()) == 0
        T.reseed(BASE)
        if whole:
            loss, pred = training.compute_loss(m, img, query, target, cycle_consis=True, bidirectional=True, branch_free=True)
        else:
            pred = training.forward_train(m, img, query)
            loss = F.mse_loss(pred, target)
        n_forward = len(drawn)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        lib.cotr_train_set_dropout_salt(None)
    assert len(drawn) == n_forward == (72 if whole else 48)                 # the backward draws none: it reuses the forward's
    assert [s for s, _, _ in drawn] == ref.hook.seeds
    assert [(k, n) for _, k, n in drawn] == _expected_sites(whole)
    assert len(cycles) == (2 if whole else 1)
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters() if p.requires_grad}
    return loss.item(), pred.detach(), (cycles[1].detach() if whole else None), grads


@pytest.mark.parametrize('salt', [None, SALT], ids=['plain', 'salt'])
def test_step_case_is_well_posed(salt, reference):
    """compute_loss at train_case(SEED): the cycle term is live under the masks, and no query of the fp64 oracle is within 1e-3
    of the cycle threshold (measured: 2.7e-2), so the cycle mask cannot flip on rounding."""
    ref = reference(True, salt)
    assert 0.2 <= float(ref.mask.float().mean()) <= 0.95
    assert ref.margin > 1e-3, ref.margin


@pytest.mark.parametrize('form', [0, 1, 2, 3])
def test_forward_train_with_dropout(form, reference, monkeypatch):
    """forward_train + the MSE loss at 2 x 24 under every train_attention_form: 48 seeds, loss, pred and every gradient."""
    ref = reference(False)
    _lib.set_knob('train_attention_form', form)
    loss, pred, _, grads = _hip_step(ref, False, None, monkeypatch)
    ref.check(f'forward_train {B}x{Q} dropout {P} form {form}', loss, pred, None, grads)


@pytest.mark.parametrize('salt', [None, SALT], ids=['plain', 'salt'])
def test_compute_loss_step_with_dropout(salt, reference, monkeypatch):
    """One whole compute_loss step (cycle_consis, bidirectional, branch_free) at the default knobs, without and with a dropout
    salt word registered: 72 seeds - one encoder over 2B pairs, then two decodes - loss, pred, cycle mask, every gradient."""
    ref = reference(True, salt)
    loss, pred, cycle, grads = _hip_step(ref, True, salt, monkeypatch)
    ref.check(f'compute_loss {B}x{Q} dropout {P} salt {salt}', loss, pred, cycle, grads)
