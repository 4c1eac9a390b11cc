"""Varlen decode against the zero-padded uniform call on the same inputs (model.forward_varlen vs model(img, padded)).

  (a) 32 pairs, counts [257] + 31 x [8]      (FasterSparseEngine's grouped call with one large squad)
  (b) 8 pairs, counts spread 200 ... 4000    (per-pair keypoints)
  (c) uniform 32 x 1000 and 1 x 1000         (the varlen path's overhead against cotr_forward)
  (d) FasterSparseEngine at the configs[2] shape (512x512 pair, 10 000 forced queries, converge_iters 3), varlen off / on:
      wall time, decoded_rows, histogram of the grouped calls' squad sizes

Timing: device-synchronised host clock around `--iters` calls after `--warmup` calls of the same shape; the two forms alternate
in `--rounds` rounds and the median per call is reported (with min / max over rounds).  Outputs of the two forms are compared on
the real rows.  GPU box:  python tools/bench_varlen.py [--out profiles/varlen_bench.json]
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import cotr_amd
from cotr_amd.models import build_model
from cotr_amd.utils.synth import synth_state_dict, synth_inputs


def timed(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e3


def compare(m, counts, seed, args):
    b = len(counts)
    img, _ = synth_inputs(b, 1, seed=seed)
    rng = np.random.default_rng(seed)
    n = int(sum(counts))
    q = torch.from_numpy(rng.random((n, 2)).astype(np.float32)).cuda()
    img = img.cuda()
    qmax = max(counts)
    pad = torch.zeros(b, qmax, 2, device='cuda')
    ends = np.cumsum(counts)
    for i, c in enumerate(counts):
        pad[i, :c] = q[ends[i] - c:ends[i]]
    run_vl = lambda: m.forward_varlen(img, q, counts)            # noqa: E731
    run_pad = lambda: m(img, pad)['pred_corrs']                  # noqa: E731
    for _ in range(args.warmup):
        run_vl()
        run_pad()
    t_vl, t_pad = [], []
    for _ in range(args.rounds):
        t_pad.append(timed(run_pad, args.iters))
        t_vl.append(timed(run_vl, args.iters))
    vl, pd = run_vl().cpu(), run_pad().cpu()
    real = torch.cat([pd[i, :c] for i, c in enumerate(counts)])
    err = float(((vl.double() - real.double()).abs() * torch.tensor([512.0, 256.0], dtype=torch.float64)).max()) if n else 0.0
    return dict(pairs=b, rows=n, padded_rows=b * qmax, varlen_ms=statistics.median(t_vl), padded_ms=statistics.median(t_pad),
                varlen_ms_minmax=[min(t_vl), max(t_vl)], padded_ms_minmax=[min(t_pad), max(t_pad)],
                speedup=statistics.median(t_pad) / statistics.median(t_vl), max_px_diff=err)


def engine_case(m, varlen):
    from cotr_amd.inference import FasterSparseEngine
    from tests.engine_fixtures import synthetic_pair
    ia, ib = synthetic_pair(4, (512, 512), (512, 512))
    rng = np.random.default_rng(1)
    q10k = np.stack([rng.uniform(5, 507, 10000), rng.uniform(5, 507, 10000)], 1)
    zooms = np.linspace(0.5, 0.0625, 4)
    eng = FasterSparseEngine(m, 32, 'tile', max_load=256, varlen=varlen)
    hist = collections.Counter()
    form = eng._form_grouped_batch

    def logged(zoom, tasks):
        squads, boxes, queries = form(zoom, tasks)
        hist.update(len(s) for s in squads)
        return squads, boxes, queries
    eng._form_grouped_batch = logged
    np.random.seed(0)
    torch.cuda.synchronize()
    t = time.perf_counter()
    corrs = eng.cotr_corr_multiscale(ia, ib, zooms, 3, max_corrs=10000, queries_a=q10k, force=True)
    torch.cuda.synchronize()
    return dict(varlen=varlen, wall_s=time.perf_counter() - t, correspondences=len(corrs), decoded_rows=eng.decoded_rows,
                squad_size_histogram=dict(sorted(hist.items()))), np.asarray(corrs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-engine', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_varlen.py measures on the GPU; no device found')
    m = build_model(cotr_amd.default_args()).cuda().eval()
    m.load_state_dict(synth_state_dict(0))
    res = {}
    cases = {
        'a_32_pairs_257_31x8': [257] + [8] * 31,
        'b_8_pairs_200_to_4000': [int(c) for c in np.linspace(200, 4000, 8).round()],
        'c_uniform_32x1000': [1000] * 32,
        'c_uniform_1x1000': [1000],
    }
    for i, (name, counts) in enumerate(cases.items()):
        res[name] = compare(m, counts, 700 + i, args)
        print(name, json.dumps(res[name]), flush=True)
    if not args.skip_engine:
        engine_case(m, False)                                    # warm-up of every shape the engine walks
        for varlen in (False, True, False, True):
            r, _ = engine_case(m, varlen)
            res.setdefault('d_faster_sparse_engine_config2', []).append(r)
            print('d', json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
