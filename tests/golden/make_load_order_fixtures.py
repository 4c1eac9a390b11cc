"""Records ffn_fused_sha.json and gemm_epilogue_sha.json: the sha256 of every output of tests/load_order_cases.py as THIS build of the
library computes it.  They were recorded on the commit before the scale / bias / residual requests of the k-split / wave-private GEMM
epilogues were moved in front of the K loop, so the yardstick of tests/test_ffn_fused_loads_gpu.py and tests/test_gemm_epilogue_loads_gpu.py is that commit, not
the code under test; a later change that is meant to alter these bits re-records them and says so.

    python tests/golden/make_load_order_fixtures.py      # MI355X
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def dump(name, obj, where):
    with open(os.path.join(where, name), 'w') as f:
        json.dump(obj, f, sort_keys=True, indent=0, separators=(',', ':'))
        f.write('\n')


def main(where=HERE):
    import torch
    from tests import gpu_helpers as G
    from tests import load_order_cases as C
    ffn = {}
    for M in C.FFN_ROWS:
        ref = C.ffn_reference(M)
        finite = torch.isfinite(ref).all(1)
        for mc in C.FFN_CHUNKS:
            y, nch = C.ffn_run(M, mc)
            e = G.rel_err(y[:M][finite.to(y.device)], ref[finite])
            print(f'ffn M {M} max_chunks {mc}: {nch} chunks, rel err against fp64 {e:.3g}', flush=True)
            ffn[f'M{M} max_chunks{mc}'] = {'nch': nch, 'sha256': C.sha(y)}
    dump('ffn_fused_sha.json', ffn, where)
    gemm = {}
    for cfg in C.GEMM_CFGS:
        gemm[str(cfg)] = C.gemm_run(cfg)
        print(f'gemm cfg {cfg}: {sum(v != "refused" for v in gemm[str(cfg)].values())} of {len(gemm[str(cfg)])} cases ran', flush=True)
    dump('gemm_epilogue_sha.json', gemm, where)


if __name__ == '__main__':
    main(*sys.argv[1:])
