"""Records the fixtures of the launch-configuration table (csrc/gemm.hip).  They pin what the library did BEFORE the configurations
became one table; a later change of the table that is meant to alter a pick or an accepted set re-records them and says so.

    python tests/golden/make_gemm_fixtures.py picks      # no GPU needed: gemm_picks.json
    python tests/golden/make_gemm_fixtures.py gpu        # MI355X: gemm_cfg_accepts.json (this library's key), forward_launch_names.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def dump(name, obj):
    with open(os.path.join(HERE, name), 'w') as f:
        json.dump(obj, f, sort_keys=True, separators=(',', ':'))
        f.write('\n')


def main(what):
    from tests import gemm_table_cases as C
    if what == 'picks':
        dump('gemm_picks.json', [{'knobs': s['knobs'], 'picks': s['picks']} for s in C.compute_picks()])
        return
    from cotr_amd import _lib
    from tests import test_ops_gpu as T
    path = os.path.join(HERE, 'gemm_cfg_accepts.json')
    acc = json.load(open(path)) if os.path.exists(path) else {}
    acc[str(_lib.load_library().cotr_is_experimental())] = {
        'linear': T.every_gemm_config_linear(), 'conv': T.every_gemm_config_conv(),
        'dual': {','.join(str(v) for v in c): T.dual_conv_launch(*c) for c in T.DUAL_CASES}}
    dump('gemm_cfg_accepts.json', acc)
    dump('forward_launch_names.json', C.forward_launch_names())


if __name__ == '__main__':
    main(sys.argv[1])
