"""Every stage of every pair against the float64 oracle, at shapes that together launch every kernel the forward's dispatch can
launch for 1 ... 70 pairs.

The forward picks its kernels by shape - pairs B and queries Q select the kernel family, the fill rules, the tuned GEMM configuration
(csrc/gemm_tuned.inc, nearest M) and the passes of batch_split - and a px bar on pred_corrs alone lets a 1e-4 relative error in the
memory or in layer3 through.  So each shape of SHAPES runs the default knobs (profiling off) on a batch drawn from a pool of POOL
distinct seeded pairs and checks, for every pair: layer1 / layer2 / layer3 (cotr_backbone_upto: the default path, fused stem, all
passes), memory, kv (the hoisted decoder K/V) and pos (taps that always cover the whole batch), pred_corrs for every query; then, where
the decode is one pass, query_pos and hs from a second run with debug taps on.

Bars, per pair p and stage s: err = max|gpu - ref64| / max|ref64|, gap32 the same quantity for the float32 oracle;
err <= max(FLOOR[s], 4 * gap32) (the rule of tests/test_training_gpu.py's float64 gradient check).  pred_corrs: px error against
float64 <= max(1e-3 px, 3 x the float32 oracle's px gap), as in tests/test_parity_gpu.py test_golden_vectors_from_the_reference.

test_checked_shapes_launch_every_kernel_the_dispatch_can_launch ties SHAPES to the dispatch: it lists the launches of a profiled
forward (cotr_set_profiling 2) at every B in 1 ... 70 and Q in COVERAGE_Q, normalises each name to a key (launch_key) and asserts that
SHAPES reach every key.
"""
import re

import pytest
import torch

from cotr_amd.utils.synth import synth_state_dict, synth_inputs
from oracle import cotr_oracle as O
from tests.test_parity_gpu import PX_BAR, hip_model

pytestmark = pytest.mark.gpu

POOL = 70
# (pairs, queries): the regimes of tests/knob_cases.py and tests/test_parity_gpu.py, then the shapes the coverage test asks for
SHAPES = [(1, 1000),   # q16 encoder attention, dual convolutions, conv_patch
          (1, 1), (2, 257), (3, 333), (4, 1000),
          (5, 17),     # bottleneck.hip at bottleneck_max_pairs
          (8, 512), (9, 100), (16, 16), (17, 1000), (24, 100), (28, 17), (32, 1), (33, 40), (64, 100), (65, 1), (70, 257),
          # then what the coverage test asked for: GEMM configurations of the tuned table (gemm_tuned.inc, nearest M) that no shape above
          # picks - 7: conv1x1 cfg27; 10: conv1x1 / linear cfg11, linear cfg12, the +pos in-projection on cfg1; 13: conv cfg40 / cfg41;
          # 15: conv3x3 cfg26, +pos on cfg25; 21: conv3x3 cfg27; 30: linear cfg33; 46: layer3 conv3x3 cfg27, linear cfg26, +pos on cfg1
          (7, 1), (10, 333), (13, 1), (15, 100), (21, 1), (30, 17), (46, 333)]
COVERAGE_Q = (1, 16, 17, 100, 257, 1000)
STAGES = ('layer1', 'layer2', 'layer3', 'memory', 'kv', 'pos', 'query_pos', 'hs')
FLOOR = dict(layer1=1e-5, layer2=1e-5, layer3=1e-5, memory=1e-5, kv=1e-5, hs=1e-5, pos=1e-6, query_pos=1e-6)
LAYER_SHAPE = {1: (64, 128, 256), 2: (32, 64, 512), 3: (16, 32, 1024)}   # [H, 2W, C] of layer1 ... layer3, NHWC over the pair

_pool = {}
_worst = {}   # stage -> (err / bar, (B, Q), pool pair)


def _rel(a, b):
    """max|a - b| / max|b| in float64 (b: the float64 truth)"""
    a, b = a.double(), b.double().to(a.device)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def pool():
    """POOL seeded pairs through the oracle's encoder, once per module, in float64 and in float32: the float64 stages in the
    library's layouts rounded to float32 (~6e-8 relative; ~17 MB a pair), the float32 oracle's gap to them, both memories for the
    decoder and the K/V."""
    if not _pool:
        sd = synth_state_dict(0)
        sd64 = {k: v.double() for k, v in sd.items()}
        pairs = []
        with torch.no_grad():
            for i in range(POOL):
                img = synth_inputs(1, 0, seed=9000 + i)[0]
                e64, e32 = O.cotr_encode(sd64, img, torch.float64), O.cotr_encode(sd, img, torch.float32)
                kv64, kv32 = O.decoder_kv(sd64, e64['memory'], e64['pos']), O.decoder_kv(sd, e32['memory'], e32['pos'])
                ref, gap = {}, {}
                for s in ('layer1', 'layer2', 'layer3'):
                    ref[s] = O.nchw_to_sbs(e64[s])[0].float()
                    gap[s] = _rel(e32[s], e64[s])
                ref['memory'], gap['memory'] = O.seq_to_rows(e64['memory']).float(), _rel(e32['memory'], e64['memory'])
                gap['kv'] = _rel(kv32, kv64)                                # (kv64 itself is recomputed per shape: cheap, 6 MB a pair)
                pairs.append(dict(img=img[0], ref=ref, gap=gap, mem64=e64['memory'], mem32=e32['memory']))
        _pool.update(sd=sd, sd64=sd64, pairs=pairs, pos64=e64['pos'], pos32=e32['pos'],
                     pos_gap=_rel(e32['pos'], e64['pos']))
    return _pool


def shape_pairs(b, q):
    """pool pairs (offset + j) % POOL: distinct within a batch, and a pair sits at another position in every shape"""
    offset = (13 * SHAPES.index((b, q))) % POOL
    return [(offset + j) % POOL for j in range(b)]


def shape_queries(b, q):
    """seeded per shape; about 5 % in [-0.5, 1.5], as the cycle pass feeds predictions back (inference_helper.py:197-198)"""
    g = torch.Generator().manual_seed(100000 + 1000 * b + q)
    qs = torch.rand(b, q, 2, generator=g)
    wide = torch.rand(b, q, 1, generator=g) < 0.05
    return torch.where(wide, torch.rand(b, q, 2, generator=g) * 2 - 0.5, qs)


@pytest.mark.parametrize('b,q', SHAPES, ids=[f'{b}x{q}' for b, q in SHAPES])
def test_every_stage_of_every_pair_against_float64(b, q):
    P = pool()
    idx = shape_pairs(b, q)
    pairs = [P['pairs'][i] for i in idx]
    img = torch.stack([p['img'] for p in pairs]).cuda()
    qs = shape_queries(b, q)
    m = hip_model()
    out = m(img, qs.cuda())['pred_corrs'].cpu()
    got = {'memory': m.debug_tap('memory').view(b, 512, 256), 'kv': m.debug_tap('kv').view(b, 512, -1)}
    pos = m.debug_tap('pos').view(512, 256)
    for stage in (1, 2, 3):
        got[f'layer{stage}'] = m.backbone_upto(img, stage, out=torch.full((b,) + LAYER_SHAPE[stage], float('nan'), device='cuda'))
    one_decode_pass = m.batch_chunks(b, q, 1) == [b]
    if one_decode_pass:
        m.set_debug_taps(True)
        try:
            m(img, qs.cuda())
            got['query_pos'] = m.debug_tap('query_pos').view(b, q, 256)
            got['hs'] = m.debug_tap('hs').view(b, q, 256)
        finally:
            m.set_debug_taps(False)

    with torch.no_grad():
        mem64 = torch.cat([p['mem64'] for p in pairs], 1)
        mem32 = torch.cat([p['mem32'] for p in pairs], 1)
        taps64, taps32 = {}, {}
        d64 = O.cotr_decode(P['sd64'], mem64, P['pos64'], qs, torch.float64, taps=taps64)
        d32 = O.cotr_decode(P['sd'], mem32, P['pos32'], qs, torch.float32, taps=taps32)
    ref = {s: [p['ref'][s] for p in pairs] for s in ('layer1', 'layer2', 'layer3', 'memory')}
    ref['kv'] = O.decoder_kv(P['sd64'], mem64, P['pos64']).view(b, 512, -1)
    gap = {s: [p['gap'][s] for p in pairs] for s in ('layer1', 'layer2', 'layer3', 'memory', 'kv')}
    for s, t64, t32 in (('query_pos', taps64['query_pos'], taps32['query_pos']), ('hs', d64['hs'], d32['hs'])):
        ref[s] = [t64[:, j] for j in range(b)]                              # [Q,B,E] -> pair j's [Q,E]
        gap[s] = [_rel(t32[:, j], t64[:, j]) for j in range(b)]

    rows = []                                                                # (stage, pair, err, bar)
    for s in STAGES:
        if s == 'pos':
            rows.append((s, None, _rel(pos, P['pos64'][:, 0]), max(FLOOR[s], 4 * P['pos_gap'])))
            continue
        if s not in got:
            continue
        for j in range(b):
            rows.append((s, idx[j], _rel(got[s][j], ref[s][j]), max(FLOOR[s], 4 * gap[s][j])))
    for j in range(b):
        e64 = O.px_err(out[j], d64['pred_corrs'][j])
        rows.append(('pred_corrs', idx[j], e64, max(PX_BAR, 3 * O.px_err(d32['pred_corrs'][j], d64['pred_corrs'][j]))))

    assert torch.isfinite(out).all()
    worst_here = {}
    for s, p, e, bar in rows:
        if e / bar > worst_here.get(s, (-1.0,))[0]:
            worst_here[s] = (e / bar, e, bar, p)
        if e / bar > _worst.get(s, (-1.0,))[0]:
            _worst[s] = (e / bar, (b, q), p)
    print(f'\n{b} x {q}: ' + '  '.join(f'{s} {r:.3f} ({e:.2e}/{bar:.1e})' for s, (r, e, bar, _) in worst_here.items()))
    print('worst err/bar so far: ' + '  '.join(f'{s} {r:.3f} @{bq[0]}x{bq[1]}' for s, (r, bq, _) in _worst.items()))
    bad = [(s, p, f'{e:.3e} > {bar:.3e}') for s, p, e, bar in rows if not e <= bar]
    assert not bad, f'{len(bad)} (stage, pool pair) over the bar at {b} x {q}: {bad[:20]}'
    if one_decode_pass:
        assert {'query_pos', 'hs'} <= set(worst_here)


# ---- coverage of the dispatch --------------------------------------------------------------------------------------------------------
def launch_key(name):
    """A per-launch profile name (api.hip prof_mark: kernel, variant, GEMM shape and configuration, flags) without what only scales
    the launch: the kernel, its variant ('enc s4', 'dec q16', 'layer1.2'), the GEMM configuration (cfgN), N and K, and the '+pos' /
    '+table' / 'dense' flags are kept; row, pair and chunk counts ('1000 rows', '5 pairs', the fused FFN's 'x4') and the M of every
    MxNxK are dropped.  'linear 512x3072x256 cfg7 +table' -> 'linear 3072x256 cfg7 +table'."""
    name = re.sub(r'(?<![\w/])\d+x(\d+x\d+)\b', r'\1', name)     # MxNxK -> NxK (also each half of a dual launch's A+B)
    name = re.sub(r' \d+ (rows|pairs)\b', '', name)              # row / pair counts
    return re.sub(r' x\d+$', '', name)                            # chunk count of the fused FFN


def launch_keys(m, img, qs):
    """the keys of one profiled forward (profiling turns the side stream off; side_stream is off by default)"""
    m.set_profiling(2)
    try:
        m(img, qs)
        torch.cuda.synchronize()
        names = m.profile_names()
        assert 0 < len(names)
        return {launch_key(name) for name in names}
    finally:
        m.set_profiling(0)


def coverage(m, shapes):
    """{key: the smallest (B, Q) of the grid that reaches it} for the keys of B = 1 ... POOL x COVERAGE_Q that no shape of `shapes`
    reaches"""
    g = torch.Generator(device='cuda').manual_seed(3)
    img = torch.randn(POOL, 3, 256, 512, device='cuda', generator=g)     # the dispatch does not look at the data
    qs = torch.rand(POOL, max(max(COVERAGE_Q), max(q for _, q in shapes)), 2, device='cuda', generator=g)
    m.reserve(POOL, qs.shape[1])
    checked = set()
    for b, q in shapes:
        checked |= launch_keys(m, img[:b], qs[:b, :q].contiguous())
    first = {}
    for b in range(1, POOL + 1):
        for q in COVERAGE_Q:
            for k in launch_keys(m, img[:b], qs[:b, :q].contiguous()) - checked:
                first.setdefault(k, (b, q))
    return first


def test_checked_shapes_launch_every_kernel_the_dispatch_can_launch():
    m = hip_model()
    missing = coverage(m, SHAPES)
    assert not missing, 'launch keys no shape of SHAPES reaches (key <- smallest (pairs, queries) that does):\n' + \
        '\n'.join(f'  {k}  <- {bq}' for k, bq in sorted(missing.items(), key=lambda kv: (kv[1], kv[0])))
