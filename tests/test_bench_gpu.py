"""bench.py on the MI355X.  --dump-outputs: what the timed path computed in its last step is the product path's answer on the
benchmark's seeded inputs, checked against the CPU oracle.  A plain run (no --full) does what its headline figure needs and no
more.  Both tests read ONE plain run of the benchmark."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from cotr_amd.utils.synth import synth_inputs, synth_state_dict
from oracle import cotr_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 3, 1


@pytest.fixture(scope='module')
def plain_run(tmp_path_factory):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR` in a process of its own -> (its JSON line, DIR, seconds from start to exit)"""
    out = tmp_path_factory.mktemp('bench_dump')
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS), '--warmup', str(WARMUP),
                        '--dump-outputs', str(out)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), out, wall


def test_headline_dump_is_the_forward_on_the_seeded_inputs(plain_run):
    line, tmp_path, _ = plain_run
    assert line['steps'] == 3 and line['ms_per_step'] > 0
    assert line['dumped_outputs'] == {'pred_corrs': [1, 1000, 2]}
    out = np.load(tmp_path / 'pred_corrs.npy')
    assert out.dtype == np.float32
    img, qs = synth_inputs(1, 1000, seed=1)                     # the headline workload's inputs (rank 0)
    ref = cotr_oracle.cotr_forward(synth_state_dict(0), img, qs)
    err = cotr_oracle.px_err(torch.from_numpy(out), ref)
    assert err < 1e-3, f'dumped prediction vs the CPU oracle: {err} px'


def test_plain_run_is_lean(plain_run):
    """Without --full the line carries the headline and nothing that takes runs of its own, and the run spends at most 30 s outside
    its steps: start to exit of the process, less (steps + warmup) x ms_per_step."""
    line, _, wall = plain_run
    assert line['metric'] == 'query-correspondences/sec at 256x512 SBS, 1k queries' and line['unit'] == 'query-correspondences/s'
    assert line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['steps'] == STEPS and line['warmup'] == WARMUP
    assert abs(line['value'] - 1000 / (line['ms_per_step'] * 1e-3)) <= 1e-6 * line['value']
    assert 'cpu_baseline' not in line and 'also_measured' not in line
    moved = {'stages', 'kernels', 'dominant_kernel', 'launches_per_forward', 'by_batch', 'batched_frac', 'traffic_detail'}
    assert not moved & set(line['roofline']), sorted(moved & set(line['roofline']))
    assert 'measured' not in str(line['roofline'].get('traffic_source', ''))
    outside = wall - (STEPS + WARMUP) * line['ms_per_step'] * 1e-3
    print(f'plain run: {wall:.1f} s from start to exit, {outside:.1f} s outside its steps')
    assert outside <= 30.0, f'{outside:.1f} s outside the steps'
