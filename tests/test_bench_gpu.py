"""bench.py --dump-outputs on the MI355X: what the timed path computed in its last step is the product path's answer on the
benchmark's seeded inputs, checked against the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cotr_amd.utils.synth import synth_inputs, synth_state_dict
from oracle import cotr_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_headline_dump_is_the_forward_on_the_seeded_inputs(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '1', '--no-extras', '--no-cpu-baseline',
                        '--traffic', 'none', '--dump-outputs', str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['steps'] == 3 and line['ms_per_step'] > 0
    assert line['dumped_outputs'] == {'pred_corrs': [1, 1000, 2]}
    out = np.load(tmp_path / 'pred_corrs.npy')
    assert out.dtype == np.float32
    img, qs = synth_inputs(1, 1000, seed=1)                     # the headline workload's inputs (rank 0)
    ref = cotr_oracle.cotr_forward(synth_state_dict(0), img, qs)
    err = cotr_oracle.px_err(torch.from_numpy(out), ref)
    assert err < 1e-3, f'dumped prediction vs the CPU oracle: {err} px'
