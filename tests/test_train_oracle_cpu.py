"""The training oracle (oracle/train_oracle.py) against the reference's own training step (tests/golden/train_step_*_b2_q24.npz,
made by tests/golden/make_train_golden.py from the unmodified reference).  It is the yardstick of the GPU gradient tests at the
benchmark shape (tests/test_train_bench_shape_gpu.py), so it is pinned here in fp32, against its own fp64 run, and chunked
against unchunked.  CPU only."""
import os

import numpy as np
import pytest
import torch

import cotr_amd
from cotr_amd.models import build_model
from oracle.train_oracle import train_loss_and_grads
from tests.golden.make_train_golden import cycle_case, train_case


def _trainable(lr_backbone):
    m = build_model(cotr_amd.default_args(dropout=0.0, lr_backbone=lr_backbone))
    return [n for n, p in m.named_parameters() if p.requires_grad]


def _check_stats(grads, names, stats):
    """Every tensor of the golden's list is there, with its (sum, sum |g|, norm) within 1e-5; and nothing else is."""
    for name, (s, a, n) in zip(names, stats):
        name = str(name)
        if n == 0.0:                   # the reference's allow_unused None: the forward does not touch it
            assert name not in grads, name
            continue
        g = grads[name].double()
        assert abs(float(g.norm()) - n) <= 1e-5 * n, (name, float(g.norm()), n)
        assert abs(float(g.abs().sum()) - a) <= 1e-5 * a, name
    assert set(grads) <= {str(n) for n in names}


def _check_full(grads, g, prefix):
    keys = [k for k in g.files if k.startswith(prefix)]
    assert keys
    for key in keys:
        want = g[key]
        got = grads[key[len(prefix):]].numpy()
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), key


@pytest.mark.parametrize('golden,lr_backbone', [('train_step_b2_q24', 0.0), ('train_step_backbone_b2_q24', 1e-5)])
def test_oracle_reproduces_the_reference_training_step(golden, lr_backbone, golden_dir):
    g = np.load(os.path.join(golden_dir, golden + '.npz'))
    sd, img, query, target = train_case()
    names = _trainable(lr_backbone)
    r32 = train_loss_and_grads(sd, img, query, target, names, dtype=torch.float32)
    assert abs(r32.loss - float(g['loss'])) <= 1e-6 * float(g['loss'])
    assert abs(r32.cycle_loss - float(g['cycle_loss'])) <= 1e-5 * float(g['cycle_loss'])
    assert np.array_equal(r32.mask.numpy(), g['mask'])
    assert np.abs(r32.pred.numpy() - g['pred']).max() < 1e-6
    assert sorted(r32.grads) == sorted(str(n) for n in g['grad_names'])        # exactly the tensors that get a gradient
    assert len(r32.grads) == (186 if lr_backbone else 154)
    _check_stats(r32.grads, g['grad_names'], g['grad_stats'])
    _check_full(r32.grads, g, 'grad.')
    # the cycle term alone (cgrad_names lists the same tensors as the reference's params list)
    _check_stats(r32.cycle_grads, g['cgrad_names'], g['cgrad_stats'])
    _check_full(r32.cycle_grads, g, 'cgrad.')
    # fp64 against fp32: the same step up to fp32 rounding
    r64 = train_loss_and_grads(sd, img, query, target, names)
    assert abs(r64.loss - r32.loss) <= 1e-4 * r64.loss
    assert torch.equal(r64.mask, r32.mask)
    assert r64.grads.keys() == r32.grads.keys()
    for n, want in r64.grads.items():
        got = r32.grads[n].double()
        assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max()), n
        assert float((got - want).norm()) <= 1e-4 * float(want.norm()), n


def test_oracle_reproduces_the_reference_cycle_gradient(golden_dir):
    """The case where the cycle gradient blocked at the query encoding matters (sharpened attention around a fixed point): the
    cycle term alone, against the reference's cycle_loss, cgrad.* and cgrad_stats."""
    g = np.load(os.path.join(golden_dir, 'train_step_cycle_b2_q24.npz'))
    sd, img = cycle_case()
    query, target = torch.from_numpy(g['query']), torch.from_numpy(g['target'])
    r = train_loss_and_grads(sd, img, query, target, _trainable(0.0), dtype=torch.float32)
    assert abs(r.cycle_loss - float(g['cycle_loss'])) <= 1e-6 * float(g['cycle_loss'])
    assert abs(r.loss - float(g['loss'])) <= 1e-6 * float(g['loss'])
    assert np.array_equal(r.mask.numpy(), g['mask'])
    _check_stats(r.cycle_grads, g['cgrad_names'], g['cgrad_stats'])
    _check_full(r.cycle_grads, g, 'cgrad.')


def test_chunked_accumulation_equals_one_chunk():
    """Stage 2, 3 pairs: one pair per chunk against all three in one, fp64 - the same sums in another grouping."""
    sd, img, query, target = train_case(seed=2, B=3, Q=10)
    names = _trainable(1e-5)
    one = train_loss_and_grads(sd, img, query, target, names, pairs_per_chunk=3)
    per_pair = train_loss_and_grads(sd, img, query, target, names, pairs_per_chunk=1)
    assert 0 < int(one.mask.sum()) < one.mask.numel()             # both terms take part
    assert torch.equal(one.mask, per_pair.mask)
    assert abs(one.loss - per_pair.loss) <= 1e-10 * one.loss
    assert one.grads.keys() == per_pair.grads.keys() and len(one.grads) == 186
    for n, want in one.grads.items():
        assert float((per_pair.grads[n] - want).norm()) <= 1e-10 * float(want.norm()), n
