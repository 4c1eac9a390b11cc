"""Loss and gradients of one training step of the reference, on CPU, in fp32 or fp64.

TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``): the checker of the HIP training step (``cotr_amd/training.py``).

The loss is ``COTRTrainer.train_batch`` (COTR/trainers/cotr_trainer.py:124-142) with ``cycle_consis`` and
``bidirectional`` on, dropout 0 (or the caller's masks: ``dropout``), on the oracle's forward (``cotr_oracle.cotr_forward_grad``):

    pred  = f(img, query)                    loss = mse(pred, target) + mse(cycle[mask], query[mask])
    cycle = f(img, pred.detach())            mask = |cycle - query| < 10/256

The cycle pass gets the prediction detached because the reference's query encoding is ``@torch.no_grad()``
(COTR/models/position_encoding.py:40-45): nothing flows back through ``pred``.

Bounded memory.  Pairs never interact, so the gradient is a sum over chunks of pairs, and only one chunk's pass holds a
graph at a time.  The two terms have disjoint graphs (the cycle pass sees ``pred`` only detached), so each chunk adds
``grad sum (pred - target)^2`` and ``grad sum_mask (cycle - query)^2`` to two accumulators.  They are scaled by
``1 / (2 B Q)`` and ``1 / (2 N)`` at the end, when the mask count N over the whole batch is known: no separate no-grad
pass is needed for N.  16 pairs x 200 queries in fp64 with 2 pairs per chunk peak at about 3 GB.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import cotr_oracle

CYCLE_RADIUS = 10 / 256       # cotr_trainer.py:131 (10 / MAX_SIZE)


def train_loss_and_grads(sd, img, query, target, trainable_names, dtype=torch.float64, pairs_per_chunk=2, dropout=None):
    """-> namespace with ``loss`` (the reference's value, float), ``pred_loss``, ``cycle_loss``, ``pred`` [B,Q,2],
    ``cycle`` [B,Q,2], ``mask`` [B,Q] (bool), ``margin`` (the smallest | |cycle - query| - 10/256 | over all queries: how
    far the mask is from flipping), ``grads`` {name: d loss / d weight} and ``cycle_grads`` {name: d cycle_loss / d weight}.

    ``trainable_names``: the parameters that train (a HIP model's ``named_parameters()`` with ``requires_grad``).  Those
    the forward never touches (the decoder's ``norm1``) get no entry, as they get no ``.grad`` in a backward pass.
    ``pairs_per_chunk``: pairs per forward / backward (memory); the result does not depend on it beyond rounding.
    ``dropout``: None, or the training-mode dropouts with the caller's masks: ``dropout(site, tensor) -> tensor * mask factor``
    as in ``cotr_oracle.cotr_encode``, the site prefixed with the pass and the chunk's first pair, ``'pred.<lo>.'`` or
    ``'cycle.<lo>.'`` (e.g. ``'cycle.2.decoder.0.attn'``: the tensor holds pairs lo .. of that pass)."""
    sd = {k: v.detach().to(dtype) for k, v in sd.items()}
    names = list(trainable_names)
    params = [sd[n].requires_grad_() for n in names]
    img, query, target = img.to(dtype), query.to(dtype), target.to(dtype)
    bsz, nq, _ = query.shape
    acc_pred, acc_cycle = {}, {}

    def accumulate(acc, term):
        for n, g in zip(names, torch.autograd.grad(term, params, allow_unused=True)):
            if g is not None:
                acc[n] = g if n not in acc else acc[n] + g

    preds, cycles = [], []
    for lo in range(0, bsz, pairs_per_chunk):
        hi = min(bsz, lo + pairs_per_chunk)
        kw = [{}, {}]
        if dropout is not None:
            kw = [{'dropout': (lambda site, t, pre=f'{which}.{lo}.': dropout(pre + site, t))} for which in ('pred', 'cycle')]
        pred = cotr_oracle.cotr_forward_grad(sd, img[lo:hi], query[lo:hi], dtype=dtype, **kw[0])
        accumulate(acc_pred, ((pred - target[lo:hi]) ** 2).sum())
        pred = pred.detach()
        cycle = cotr_oracle.cotr_forward_grad(sd, img[lo:hi], pred, dtype=dtype, **kw[1])
        mask = torch.norm(cycle.detach() - query[lo:hi], dim=-1) < CYCLE_RADIUS
        accumulate(acc_cycle, ((cycle - query[lo:hi])[mask] ** 2).sum())
        preds.append(pred)
        cycles.append(cycle.detach())
    pred, cycle = torch.cat(preds), torch.cat(cycles)
    dist = torch.norm(cycle - query, dim=-1)
    mask = dist < CYCLE_RADIUS
    count = int(mask.sum())
    pred_loss = F.mse_loss(pred, target)
    cycle_loss = F.mse_loss(cycle[mask], query[mask]) if count else torch.zeros((), dtype=dtype)
    # mse_loss means over the elements: 2 coordinates per query
    grads = {n: g / (2 * bsz * nq) for n, g in acc_pred.items()}
    cycle_grads = {n: g / (2 * count) for n, g in acc_cycle.items()} if count else {}
    for n, g in cycle_grads.items():
        grads[n] = grads[n] + g if n in grads else g
    return SimpleNamespace(loss=float(pred_loss + cycle_loss), pred_loss=float(pred_loss), cycle_loss=float(cycle_loss),
                           pred=pred, cycle=cycle, mask=mask, margin=float((dist - CYCLE_RADIUS).abs().min()),
                           grads=grads, cycle_grads=cycle_grads)
