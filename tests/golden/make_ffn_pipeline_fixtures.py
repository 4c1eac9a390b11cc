"""Records ffn_pipeline_sha.json: the sha256 of cotr_op_ffn_block's output (tests/load_order_cases.ffn_run, guard row hashed) at the row
counts and chunk limits of tests/ffn_pipeline_cases.py, as THIS build of the library computes it.  It was recorded on the commit before
the few-rows fused FFN got its pipelined form (ffn_pipe.hip), whose workgroups run on ffn_fused_kernel's arithmetic in ffn_fused_kernel's
order: the yardstick of tests/test_ffn_pipeline_gpu.py is that commit, not the code under test.

    python tests/golden/make_ffn_pipeline_fixtures.py      # MI355X
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main(where=HERE):
    import torch
    from tests import gpu_helpers as G
    from tests import load_order_cases as C
    from tests import ffn_pipeline_cases as FP
    out = {}
    for M in FP.EDGE_ROWS:
        ref = C.ffn_reference(M)
        finite = torch.isfinite(ref).all(1)
        for mc in FP.EDGE_CHUNKS:
            y, nch = C.ffn_run(M, mc)
            e = G.rel_err(y[:M][finite.to(y.device)], ref[finite])
            print(f'ffn M {M} max_chunks {mc}: {nch} chunks, rel err against fp64 {e:.3g}', flush=True)
            out[f'M{M} max_chunks{mc}'] = {'nch': nch, 'sha256': C.sha(y)}
    with open(os.path.join(where, 'ffn_pipeline_sha.json'), 'w') as f:
        json.dump(out, f, sort_keys=True, indent=0, separators=(',', ':'))
        f.write('\n')


if __name__ == '__main__':
    main(*sys.argv[1:])
