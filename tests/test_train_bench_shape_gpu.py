"""The stage-2 training step at the shape bench.py --workload train times (16 pairs x 200 queries), and at a ragged one (7 x 333),
against float64 gradients of the reference's step (oracle/train_oracle.py).  The gradient tests of test_training_gpu.py all run at
2 pairs x 24 queries; at these shapes other kernels and splits run: the split-M count and tile choice of the dW GEMMs, the implicit
conv wgrad partials, the attention backward form, the GradSink chunk map, cotr_backbone_upto at 16 pairs.

Bars per tensor, fixed from the oracle alone: the fp32 oracle's gap to fp64 is the rounding an fp32 computation of this step
cannot avoid, and the HIP step may be 4x as far (with floors of 1e-3 on the norm and 1e-2 on the max):
    norm_bar = max(1e-3, 4 * |g32 - g64| / |g64|)        max_bar = max(1e-2, 4 * max|g32 - g64| / max|g64|)
Dropout 0 throughout, except the finite-difference check of the dropout masks at the end.

Cases: ``train_case(1, B, Q)``.  Seed 1, because with seed 0 one of the 3200 queries of the 16-pair case sits 8e-5 from the cycle
threshold; with seed 1 the closest is 7e-3 (16 x 200) and 1.3e-2 (7 x 333) away, so the mask cannot flip on rounding."""
import resource
import time

import pytest
import torch
import torch.nn.functional as F

import cotr_amd
from cotr_amd import _lib, training
from cotr_amd.models import build_model
from oracle import cotr_oracle
from oracle.train_oracle import train_loss_and_grads
from tests.golden.make_train_golden import train_case
from tests.test_training_gpu import _dropout_consistency_case

pytestmark = pytest.mark.gpu

CASES = [(16, 200), (7, 333)]
IDS = ['16x200', '7x333']
SEED = 1
FAMILIES = ('layer2', 'layer3', 'input_proj', 'encoder', 'decoder', 'corr_embed')


def _family(name):
    for f in FAMILIES:
        if f in name:
            return f
    raise KeyError(name)


def _model(lr_backbone):
    return build_model(cotr_amd.default_args(dropout=0.0, lr_backbone=lr_backbone)).cuda().train()


def _trainable(m):
    return [n for n, p in m.named_parameters() if p.requires_grad]


def _errors(got, want):
    d = got.double().cpu() - want
    return float(d.norm() / want.norm()), float(d.abs().max() / want.abs().max())


def _bars(g32, g64):
    """{name: (norm_bar, max_bar)} from the fp32 oracle's gap to fp64."""
    out = {}
    for n, g in g64.items():
        gap_norm, gap_max = _errors(g32[n], g)
        out[n] = (max(1e-3, 4 * gap_norm), max(1e-2, 4 * gap_max))
    return out


class _Reference:
    """The stage-2 step of one case: the fp64 oracle, and the bars from the fp32 oracle's gap to it - for the whole loss, and for
    the cycle term alone.  In these cases the cycle term is about 3e-4 of the loss and 0.5-1 % of each tensor's gradient norm
    (the damped head puts every answer near one point, so |cycle - query| is small): a 10 % error in the cycle pass's backward
    would move the whole gradient by about 6e-4, under the 1e-3 floor of its norm bar."""

    def __init__(self, B, Q):
        t0 = time.time()
        self.sd, self.img, self.query, self.target = train_case(SEED, B, Q)
        names = _trainable(build_model(cotr_amd.default_args(dropout=0.0, lr_backbone=1e-5)))
        r64 = train_loss_and_grads(self.sd, self.img, self.query, self.target, names)
        r32 = train_loss_and_grads(self.sd, self.img, self.query, self.target, names, dtype=torch.float32)
        self.pred, self.mask, self.margin = r64.pred, r64.mask, r64.margin
        assert r32.grads.keys() == r64.grads.keys() == r64.cycle_grads.keys() and torch.equal(r32.mask, r64.mask)
        # term -> (loss, loss bar (relative), {name: grad}, {name: (norm_bar, max_bar)})
        cycle_gap = abs(r32.cycle_loss - r64.cycle_loss) / r64.cycle_loss
        self.terms = {'loss': (r64.loss, 1e-5, r64.grads, _bars(r32.grads, r64.grads)),
                      'cycle': (r64.cycle_loss, max(1e-5, 4 * cycle_gap), r64.cycle_grads, _bars(r32.cycle_grads, r64.cycle_grads))}
        self.hip_default = None       # (loss, pred, grads) of the default HIP stage-2 step, for the attention-form comparisons
        print(f'[reference {B}x{Q}] fp64 + fp32 oracle {time.time() - t0:.1f} s; mask {int(self.mask.sum())}/{self.mask.numel()}, '
              f'margin {self.margin:.2e}; cycle loss fp32 gap {cycle_gap:.1e}; '
              f'peak RSS of the process so far {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2**20:.1f} GB')

    def check(self, label, loss, pred, cycle, grads, names, term='loss'):
        """loss, pred and the cycle mask of a HIP step, and the gradient of every name in ``names`` that the forward reaches;
        ``term``: 'loss' (the step) or 'cycle' (the cycle term alone)."""
        want_loss, loss_bar, want, bars = self.terms[term]
        assert abs(loss - want_loss) <= loss_bar * want_loss, (label, loss, want_loss)
        assert cotr_oracle.px_err(pred.detach().cpu(), self.pred) < 1e-3, label
        if cycle is not None:
            mask = torch.norm(cycle.detach().double().cpu() - self.query.double(), dim=-1) < 10 / 256
            assert torch.equal(mask, self.mask), label
        reached = [n for n in names if n in want]
        assert reached == [n for n in names if not ('decoder' in n and '.norm1.' in n)]   # the forward never applies norm1
        worst, bad = dict.fromkeys(FAMILIES, 0.0), []
        for n in reached:
            assert grads.get(n) is not None, (label, n)
            assert bool(torch.isfinite(grads[n]).all()), (label, n, 'not finite')
            e_norm, e_max = _errors(grads[n], want[n])
            r = max(e_norm / bars[n][0], e_max / bars[n][1])
            worst[_family(n)] = max(worst[_family(n)], r)
            if not r <= 1:                              # (a NaN fails too)
                bad.append((n, e_norm, bars[n][0], e_max, bars[n][1]))
        for n in set(names) - set(reached):             # untouched: no gradient, or the sink's zeros
            assert grads.get(n) is None or not grads[n].any(), (label, n)
        print(f'[{label}] worst error/bar: ' + ', '.join(f'{f} {worst[f]:.3f}' for f in FAMILIES if f in {_family(n) for n in reached}))
        assert not bad, (label, bad[:8])


@pytest.fixture(scope='module')
def reference():
    """The CPU oracle of each case, computed once for the module."""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = _Reference(*case)
        return cache[case]
    return get


def _step(m, ref, monkeypatch, sink=None, cycle_only=False):
    """compute_loss + backward on the case's inputs -> (loss, pred, cycle, {name: grad}).  The cycle is the second decode_train
    of compute_loss, recorded on the way.  ``cycle_only``: backward from the cycle term alone, mse(cycle[mask], query[mask]) of
    that recorded cycle - the same graph, the same kernels at the same shapes, without the prediction term."""
    outs = []
    decode = training.decode_train

    def recording(*a, **k):
        outs.append(decode(*a, **k))
        return outs[-1]
    monkeypatch.setattr(training, 'decode_train', recording)
    m.load_state_dict(ref.sd)
    loss, pred = training.compute_loss(m, ref.img.cuda(), ref.query.cuda(), ref.target.cuda())
    monkeypatch.setattr(training, 'decode_train', decode)
    assert len(outs) == 2
    if cycle_only:
        query = ref.query.cuda()
        mask = torch.norm(outs[1] - query, dim=-1) < 10 / 256
        loss = F.mse_loss(outs[1][mask], query[mask])
    if sink is not None:
        sink.zero()
        with sink.collect():
            loss.backward()
    else:
        loss.backward()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters() if p.requires_grad}
    return loss.item(), pred.detach(), outs[1].detach(), grads


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_case_is_well_posed(case, reference):
    """The cycle term is live (a real share of the queries in the mask) and no query is near enough the threshold to flip."""
    ref = reference(case)
    frac = float(ref.mask.float().mean())
    assert 0.2 <= frac <= 0.95, frac
    assert ref.margin > 1e-3, ref.margin


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_stage2_step_and_grad_sink(case, reference, monkeypatch):
    """(a) Stage 2, compute_loss + backward; (b) the same step collected by grad_sink_for(optim): bit for bit (a)."""
    ref = reference(case)
    m = _model(1e-5)
    names = _trainable(m)
    loss, pred, cycle, grads = _step(m, ref, monkeypatch)
    ref.check(f'{case[0]}x{case[1]} stage 2', loss, pred, cycle, grads, names)
    ref.hip_default = (loss, pred, grads)
    m = _model(1e-5)
    sink = training.grad_sink_for(training.optimizer_for(m, 1e-4, 1e-5))
    loss_s, pred_s, _, grads_s = _step(m, ref, monkeypatch, sink)
    assert loss_s == loss and torch.equal(pred_s, pred)
    assert grads_s.keys() == grads.keys()
    for n, g in grads.items():
        if g is None:
            assert not grads_s[n].any(), n
        else:
            assert torch.equal(grads_s[n], g), (n, float((grads_s[n] - g).abs().max()))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_stage2_cycle_term(case, reference, monkeypatch):
    """(a') Stage 2, backward from the cycle term alone: the second decode, the second half of the shared 2B-pair encoder pass,
    the second pass's block of the hoisted decoder K / V, and the backbone under it, held to bars of their own."""
    ref = reference(case)
    m = _model(1e-5)
    loss, pred, cycle, grads = _step(m, ref, monkeypatch, cycle_only=True)
    ref.check(f'{case[0]}x{case[1]} stage 2, cycle term alone', loss, pred, cycle, grads, _trainable(m), term='cycle')


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_stage1_step(case, reference, monkeypatch):
    """(c) Stage 1 (lr_backbone 0, bench.py --stage 1): the backbone on the inference kernels, no backbone gradient."""
    ref = reference(case)
    m = _model(0.0)
    names = _trainable(m)
    assert not any('backbone' in n for n in names)
    loss, pred, cycle, grads = _step(m, ref, monkeypatch)
    ref.check(f'{case[0]}x{case[1]} stage 1', loss, pred, cycle, grads, names)


def _attention_kernels(form, nb, nq, packed):
    """Which attention kernels train_attention_fwd / train_attention_bwd (csrc/attention_train.hip) launch for a form at a shape:
    (forward, backward).  Backward: kt 4 / 2 / 1 = the one-pass kernel with the keys of a head over 4 / kt workgroups
    (attn_fused_kt), else the two-kernel first or second form.  train_ops.Attention hands the kernel a dQ scratch (the condition
    of a key split) only for unpacked q (the decoder) below 24 pairs.  Restates attn_fused_kt and the form switch of
    train_attention_fwd / train_attention_bwd (attention_train.hip) and the ``scratch`` condition of train_ops.Attention.backward,
    which also fixes the decoder's lddq at 256: when either changes, change this with it (the identity assertion below fails
    until then)."""
    can_split = not packed and nb * 8 < 192
    if form in (1, 2):
        kt = 0
    elif nb * 8 >= 192 or not can_split:
        kt = 4 if (form == 3 or (nb * 8 >= 192 and nq >= 256)) else 0
    elif nb * 16 >= 192:
        kt = 2
    elif nb * 32 >= 192 or form == 3:
        kt = 1
    else:
        kt = 0
    return ('fwd1' if form == 1 else 'fwd2'), (f'one-pass kt{kt}' if kt else ('bwd1' if form == 1 else 'bwd2'))


@pytest.mark.parametrize('form', [1, 2, 3])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_attention_forms(case, form, reference, monkeypatch):
    """(d) train_attention_form forced process-wide (conftest puts it back).  Every form is within the bars.  Where the form picks
    the same kernels as the default for both attention calls of the step - the encoder's self-attention over 2B pairs x 512, packed
    q|k, and the decoder's B pairs x Q - the step is bit-identical to the default one; where it does not, it differs (the evidence
    that the forced branch ran).  At 16 x 200 form 3 coincides with the default everywhere: the one-pass backward for the encoder,
    its two-way key split for the decoder."""
    ref = reference(case)
    B, Q = case
    calls = ((2 * B, 512, True), (B, Q, False))
    same = all(_attention_kernels(form, *c) == _attention_kernels(0, *c) for c in calls)
    if case == (16, 200):
        assert same == (form == 3)
    if ref.hip_default is None:                         # (this test run on its own)
        loss0, pred0, _, grads0 = _step(_model(1e-5), ref, monkeypatch)
    else:
        loss0, pred0, grads0 = ref.hip_default
    _lib.set_knob('train_attention_form', form)
    m = _model(1e-5)
    names = _trainable(m)
    loss, pred, cycle, grads = _step(m, ref, monkeypatch)
    ref.check(f'{B}x{Q} stage 2 attention form {form}', loss, pred, cycle, grads, names)
    identical = loss == loss0 and torch.equal(pred, pred0) and all(
        (g is None) == (grads0[n] is None) and (g is None or torch.equal(g, grads0[n])) for n, g in grads.items())
    assert identical == same, (form, [_attention_kernels(form, *c) for c in calls], [_attention_kernels(0, *c) for c in calls])


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_graphed_step_leaves_the_gradients_in_its_sink(case, reference):
    """(e) GraphedTrainStep with FusedAdam (capturable) at learning rate 0: after one replay the gradients in its GradSink - which
    nothing clears behind the optimiser step - are within the bars, and the weights have not moved."""
    ref = reference(case)
    m = _model(1e-5)
    m.load_state_dict(ref.sd)
    names = _trainable(m)
    opt = training.optimizer_for(m, learning_rate=0.0, lr_backbone=1e-5, capturable=True, fused=True)
    for g in opt.param_groups:
        g['lr'] = 0.0                                   # (optimizer_for leaves the backbone group out at lr_backbone 0)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    img, query, target = ref.img.cuda(), ref.query.cuda(), ref.target.cuda()
    step = None
    try:
        step = training.GraphedTrainStep(m, opt, img, query, target, warmup=1)
        loss, pred = step(img, query, target, check=True)
        torch.cuda.synchronize()
        flat = opt.sink.flat
        lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
        grads = {}
        for n, p in m.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and lo <= p.grad.data_ptr() < hi, n
                grads[n] = p.grad.detach().clone()
        ref.check(f'{case[0]}x{case[1]} graphed step', float(loss), pred, None, grads, names)
        for n, p in m.named_parameters():
            assert torch.equal(p.detach(), before[n]), n
    finally:
        if step is not None:
            step.close()
        _lib.load_library().cotr_train_set_dropout_salt(None)


@pytest.mark.parametrize('whole_step', [False, True], ids=['forward_train', 'compute_loss'])
@pytest.mark.parametrize('with_salt', [False, True])
def test_dropout_masks_are_consistent_at_the_bench_shape(with_salt, whole_step):
    """Dropout 0.1 at 16 x 200: the analytic gradient (backward kernels regenerating the masks) against central finite differences
    of the loss, as test_training_gpu.py checks at 2 x 24.  ``forward_train``: the prediction pass alone, so the encoder sees 16
    pairs and its attention runs the two-kernel backward.  ``compute_loss``: the loss of the benchmarked step, both passes, so the
    encoder sees 32 pairs and runs the one-pass backward with dropout, and the decoder its two-way key split.  (A cycle-mask flip
    under the +-eps perturbation would move the loss by at most (10/256)^2 / (2 N) ~ 3e-7: far below the 3 % bar.)"""
    _dropout_consistency_case(with_salt, B=16, Q=200, whole_step=whole_step)
