"""cotr_amd/data.py on the MI355X against the numpy oracle of tests/dataset_oracle.py (which tests/test_dataset_cpu.py holds
against the reference's own projector) and against Pillow itself.

depth_corrs: candidates whose oracle margin to the nearest decision is below MARGIN are left out (at most 0.01 % of a
case's candidates, asserted), the rest must agree in membership AND order, coordinates within TOL.  Both are float64
round-off bounds - two orderings of a 4-term float64 dot product differ by about 1e-13 relative at values up to about
2e3 - not tuned numbers."""
import numpy as np
import PIL.Image
import pytest
import torch

import cotr_amd
from cotr_amd import data, training
from cotr_amd.data import Capture
from cotr_amd.inference import patch_boxes
from cotr_amd.models import build_model
from cotr_amd.utils.synth import synth_captures, synth_state_dict
from tests import dataset_oracle as oracle
from tests import image_kernel_cases as cases

pytestmark = pytest.mark.gpu

MARGIN = 1e-9          # px or depth units
TOL = 1e-9             # px
MAX_AMBIGUOUS = 1e-4   # share of the candidates of a case


def _oracle(f, t, subset=None):
    return oracle.reproject(f.depth, t.depth, f.K, f.c2w, t.K, t.c2w, subset=subset)


def _compare(dev_rows, dev_count, f, t, subset=None, cap=None):
    """device rows [cap, 4] + count of one item against the oracle, by the rule of the module docstring"""
    r = _oracle(f, t, subset)
    W = f.depth.shape[1]
    ambiguous = r['margin'] < MARGIN
    share = ambiguous.mean() if ambiguous.size else 0.0
    print(f'{f.depth.shape} -> {t.depth.shape}: {ambiguous.size} candidates, {int(r["keep"].sum())} kept, device count {dev_count}, '
          f'{int(ambiguous.sum())} ambiguous, smallest margin {r["margin"].min() if r["margin"].size else None}')
    assert share <= MAX_AMBIGUOUS
    amb_px = np.unique(r['index'][ambiguous])
    clear = r['keep'] & ~ambiguous
    want_px, want_uv = r['index'][clear], r['uv'][clear]
    written = dev_count if cap is None else min(dev_count, cap)
    got = dev_rows[:written]
    got_px = (got[:, 1] * W + got[:, 0]).astype(np.int64)
    assert np.array_equal(got[:, 0], np.floor(got[:, 0])) and np.array_equal(got[:, 1], np.floor(got[:, 1]))
    sel = ~np.isin(got_px, amb_px)
    got_px, got_uv = got_px[sel], got[sel, 2:]
    if cap is not None and dev_count > cap:
        want_px, want_uv = want_px[:len(got_px)], want_uv[:len(got_px)]   # the first rows, in order
        assert not amb_px.size or subset is None
    elif not amb_px.size:
        assert dev_count == len(want_px)
    assert np.array_equal(got_px, want_px)                         # membership and order
    if len(want_px):
        err = np.abs(got_uv - want_uv).max()
        print('   largest coordinate difference', err)
        assert err <= TOL
    if dev_rows.shape[0] > written:
        assert not dev_rows[written:].any()                         # nothing written past the count


def _run(froms, tos, subsets=None, cap=None):
    rows, counts = data.depth_corrs(froms, tos, subsets, cap=cap)
    rows2, counts2 = data.depth_corrs(froms, tos, subsets, cap=cap)
    assert torch.equal(counts, counts2) and torch.equal(rows.view(torch.int64), rows2.view(torch.int64))   # the same bytes
    return rows.cpu().numpy(), counts.cpu().numpy()


def _filled(c, value=7.0):
    return c._replace(depth=np.where(c.depth > 0, c.depth, np.float32(value)).astype(np.float32))


def _looking_away(c):
    return c._replace(c2w=c.c2w @ np.diag([-1.0, 1.0, -1.0, 1.0]))


@pytest.mark.parametrize('shape', [(1, 1), (2, 3), (255, 257), (256, 256), (257, 256), (480, 640), (1200, 1600)])
def test_depth_corrs_shapes(shape):
    q, n = synth_captures(shape[0] + shape[1], *shape)
    rows, counts = _run([q, n], [n, q])
    _compare(rows[0], int(counts[0]), q, n)
    _compare(rows[1], int(counts[1]), n, q)
    if shape[0] >= 255:
        assert counts.min() > 1000
        single = data.depth_corrs(q, n)
        assert single.shape == (int(counts[0]), 4) and np.array_equal(single.cpu().numpy(), rows[0, :int(counts[0])])


def test_depth_corrs_depth_patterns_and_cameras():
    q, n = synth_captures(77, 200, 300)
    zero = q._replace(depth=np.zeros_like(q.depth))
    froms = [zero, q, _filled(q), q, q]
    tos = [n, n._replace(depth=np.zeros_like(n.depth)), _filled(n), _looking_away(n), n]   # (never q -> q: u, v would be exact integers)
    rows, counts = _run(froms, tos)
    for i, (f, t) in enumerate(zip(froms, tos)):
        _compare(rows[i], int(counts[i]), f, t)
    assert counts[0] == 0 and counts[1] == 0 and counts[3] == 0 and counts[2] > 0 and counts[4] > 0
    r = _oracle(q, _looking_away(n))
    assert not r['keep'].any() and np.isfinite(r['margin']).any()            # rejected at p.z <= 0, not at the holes


def test_depth_corrs_mixed_shapes_in_one_call():
    a = synth_captures(5, 96, 128)
    b = synth_captures(5, 240, 320)
    c = synth_captures(6, 1, 7)
    froms, tos = [a[0], b[1], a[1], c[0], b[0]], [b[1], a[0], b[0], a[1], b[1]]          # from and to of different shapes
    rows, counts = _run(froms, tos)
    for i, (f, t) in enumerate(zip(froms, tos)):
        _compare(rows[i], int(counts[i]), f, t)
    assert rows.shape[1] == 240 * 320 and counts[0] > 100 and counts[1] > 100


def test_depth_corrs_subset_with_repeats():
    q, n = synth_captures(9, 240, 320)
    rng = np.random.default_rng(9)
    valid = np.flatnonzero(q.depth.reshape(-1) > 0)
    s1 = valid[rng.integers(0, valid.size, 700)]
    s1[100:140] = s1[99]                                                       # one pixel 41 times in a row
    s2 = rng.integers(0, 240 * 320, 300)                                       # holes included
    s2[::3] = s2[0]
    rows, counts = _run([q, n, q], [n, q, n], [s1, s2, None])
    _compare(rows[0], int(counts[0]), q, n, s1)
    _compare(rows[1], int(counts[1]), n, q, s2)
    _compare(rows[2], int(counts[2]), q, n)
    assert counts[0] > 100
    dev = data.depth_corrs(q, n, subset=torch.from_numpy(s1).cuda())
    assert np.array_equal(dev.cpu().numpy(), rows[0, :int(counts[0])])


def test_depth_corrs_capacity_below_the_count():
    q, n = synth_captures(13, 256, 256)
    full, counts = _run([q, n], [n, q])
    for cap in (0, 1, 1000):
        rows, c = _run([q, n], [n, q], cap=cap)
        assert np.array_equal(c, counts) and rows.shape == (2, cap, 4)
        assert np.array_equal(rows, full[:, :cap])
        if cap:
            _compare(rows[0], int(c[0]), q, n, cap=cap)
    assert counts.min() > 1000


def test_valid_pixels_is_np_where():
    depths = [synth_captures(s, h, w)[0].depth for s, (h, w) in enumerate(((1, 1), (37, 53), (256, 256), (480, 640)))]
    depths.append(np.zeros((5, 9), dtype=np.float32))
    depths.append(np.full((3, 300), np.nan, dtype=np.float32))
    idx, counts = data.valid_pixels([torch.from_numpy(d).cuda() for d in depths])
    idx2, counts2 = data.valid_pixels([torch.from_numpy(d).cuda() for d in depths])
    assert torch.equal(idx, idx2) and torch.equal(counts, counts2)
    for i, d in enumerate(depths):
        want = np.flatnonzero(d.reshape(-1) > 0)
        assert int(counts[i]) == want.size and np.array_equal(idx[i, :want.size].cpu().numpy(), want)


def _crop_case_boxes(shape, sizes, rng):
    """patch_boxes at random centres (the borders included) for every size -> int [n, 3]"""
    short = min(shape)
    out = []
    for s in sizes:
        pos = np.concatenate([rng.uniform(-50, max(shape) + 50, (3, 2)), [[0.0, 0.0], [shape[1], shape[0]]]])
        x, y, size = patch_boxes(shape, pos, (s + 0.5) / short)
        assert size == (min(s, short) // 2) * 2
        out += [(int(a), int(b), size) for a, b in zip(x, y)]
    return np.array(out, dtype=np.int32)


@pytest.mark.parametrize('shape,sizes', [
    (cases.SWEEP_SHAPES[0], list(cases.SMALL_SIZES) + [3, 100, 511, 600, min(cases.SWEEP_SHAPES[0])]),
    (cases.LADDER_SHAPES[0], cases.LADDER + [min(cases.LADDER_SHAPES[0])]),
    (cases.BIG_SHAPE, list(cases.BAND_SIZES)),
])
def test_crop_depth_is_pillow_nearest(shape, sizes):
    rng = np.random.default_rng(shape[0])
    depth = rng.random(shape, dtype=np.float32) * 10
    depth[rng.random(shape) < 0.1] = 0.0
    boxes = _crop_case_boxes(shape, sizes, rng)
    assert boxes[:, 2].min() == 2 or shape != cases.SWEEP_SHAPES[0]
    assert boxes[:, 2].max() == (min(shape) // 2) * 2                                     # the full-image box
    d = torch.from_numpy(depth).cuda()
    got = data._crop_depths([d] * len(boxes), torch.from_numpy(boxes).cuda(), 256).cpu().numpy()
    for i, (x, y, s) in enumerate(boxes.tolist()):
        want = oracle.pillow_nearest(depth[y:y + s, x:x + s])
        assert np.array_equal(got[i].view(np.int32), want.view(np.int32)), (x, y, s)      # bit for bit


def test_crop_capture():
    q, _ = synth_captures(21, 480, 640)
    for box in ((0, 0, 480), (638, 478, 2), (100, 50, 256), (33, 17, 301), (400, 300, 18)):
        z = data.crop_capture(q, box)
        x, y, s = box
        img, depth, K, c2w = oracle.crop(q, box)
        assert np.array_equal(z.depth.cpu().numpy().view(np.int32), depth.view(np.int32))
        assert np.array_equal(z.image.cpu().numpy(), img)
        scale = 256 / s
        assert np.array_equal(z.K, [[q.K[0, 0] * scale, 0, (q.K[0, 2] - x) * scale], [0, q.K[1, 1] * scale, (q.K[1, 2] - y) * scale],
                                    [0, 0, 1]])
        assert z.K.dtype == np.float64 and np.array_equal(z.c2w, q.c2w)
    z = data.crop_capture(q._replace(image=None), (5, 7, 300), out=37)                    # depth only: any output size
    assert z.image is None and np.array_equal(z.depth.cpu().numpy(), oracle.pillow_nearest(q.depth[7:307, 5:305], 37))


def _ulp_close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all())


def _check_sample(out, b, ref, num_kp, bidirectional):
    # no candidate of the sample lies within round-off of a decision: one flipped membership would change the count and
    # with it every trimmed row (the device forms the zoomed cameras in tensor arithmetic, the oracle in numpy)
    print('sample', b, 'smallest margin', ref['margin'])
    assert ref['margin'] >= MARGIN
    assert bool(out['valid'][b]) == ref['valid']
    if not ref['valid']:
        return
    assert torch.equal(out['image'][b].cpu(), torch.from_numpy(ref['image']))           # as tests/test_crop_resize_gpu.py, plus the flip
    corrs = out['corrs'][b].cpu().numpy()
    assert corrs.dtype == np.float32 and corrs.shape == (num_kp, 4)
    for name in ('corrs', 'queries', 'targets'):
        assert _ulp_close(out[name][b].cpu().numpy(), ref[name]), name
    assert out['queries'].shape[1] == (2 * num_kp if bidirectional else num_kp)
    assert (0.0 <= corrs[:, 0]).all() and (corrs[:, 0] <= 0.5).all() and (0.0 <= corrs[:, 1]).all() and (corrs[:, 1] <= 1.0).all()
    assert (0.5 <= corrs[:, 2]).all() and (corrs[:, 2] <= 1.0).all() and (0.0 <= corrs[:, 3]).all() and (corrs[:, 3] <= 1.0).all()


def _sparse_nn(q, n, keep=30):
    """the nn capture with depth at only ``keep`` pixels, all of which project into the query capture: the seed search
    succeeds, the zoomed count stays below any num_kp in the hundreds"""
    r = _oracle(n, q)
    px = r['index'][r['keep'] & (r['margin'] > 1e-3)][::97][:keep]
    depth = np.zeros_like(n.depth)
    depth.reshape(-1)[px] = n.depth.reshape(-1)[px]
    return n._replace(depth=depth)


def _zoom_rand(B, num_kp, seed, max_try=100):
    rng = np.random.default_rng(seed)
    rand = {'seed': rng.random((B, max_try)), 'zoom': rng.random(B), 'jitter': rng.random((B, 2)), 'trim': rng.random((B, num_kp)),
            'flip': rng.random(B)}
    rand['flip'][:2] = (0.25, 0.75)                                                       # a flip forced both ways
    return rand


@pytest.mark.parametrize('bidirectional', [True, False])
def test_make_zoom_batch_against_the_oracle(bidirectional):
    num_kp = 100
    pairs = [synth_captures(31, 480, 640), synth_captures(32, 480, 640), synth_captures(33, 300, 420), synth_captures(34, 480, 640),
             synth_captures(35, 480, 640)]
    pairs[3] = (pairs[3][0], _looking_away(pairs[3][1]))                                  # no overlap: the seed search fails
    pairs[4] = (pairs[4][0], _sparse_nn(*pairs[4]))                                       # num_kp above the count
    qs, ns = [p[0] for p in pairs], [p[1] for p in pairs]
    zooms = np.logspace(np.log10(1.0), np.log10(0.1), 10)
    rand = _zoom_rand(len(pairs), num_kp, 5)
    out = data.make_zoom_batch(qs, ns, num_kp, zooms, 0.125, bidirectional=bidirectional, rand=rand)
    ref = oracle.make_zoom_batch(qs, ns, num_kp, zooms, 0.125, bidirectional, rand)
    print([(r['valid'], r.get('boxes'), r.get('count')) for r in ref])
    assert [r['valid'] for r in ref] == [True, True, True, False, False]
    assert out['image'].shape == (5, 3, 256, 512) and out['valid'].dtype == torch.bool and out['image'].is_cuda
    for b in range(len(pairs)):
        _check_sample(out, b, ref[b], num_kp, bidirectional)
    again = data.make_zoom_batch(qs, ns, num_kp, zooms, 0.125, bidirectional=bidirectional, rand=rand)
    assert all(torch.equal(out[k], again[k]) for k in out)
    # device tensors in, a generator for the uniforms: valid samples keep the reference's ranges
    up = lambda c: Capture(torch.from_numpy(c.image).cuda(), torch.from_numpy(c.depth).cuda(), c.K, c.c2w)   # noqa: E731
    gen = torch.Generator(device='cuda').manual_seed(3)
    drawn = data.make_zoom_batch([up(c) for c in qs], [up(c) for c in ns], num_kp, zooms, 0.125, bidirectional=bidirectional, generator=gen)
    v = drawn['valid']
    assert v[:3].all() and not v[3:].any()
    c = drawn['corrs'][v]
    assert (c[..., 0] >= 0).all() and (c[..., 0] <= 0.5).all() and (c[..., 2] >= 0.5).all() and (c[..., 2] <= 1).all()


@pytest.mark.parametrize('bidirectional', [True, False])
def test_make_batch_against_the_oracle(bidirectional):
    num_kp = 150
    pairs = [synth_captures(41, 256, 256), synth_captures(42, 256, 256), synth_captures(43, 256, 256)]
    pairs[2] = (pairs[2][0], _sparse_nn(*pairs[2]))
    qs, ns = [p[0] for p in pairs], [p[1] for p in pairs]
    rand = {k: v for k, v in _zoom_rand(3, num_kp, 8).items() if k in ('trim', 'flip')}
    out = data.make_batch(qs, ns, num_kp, bidirectional=bidirectional, rand=rand)
    ref = oracle.make_batch(qs, ns, num_kp, bidirectional, rand)
    assert [r['valid'] for r in ref] == [True, True, False]
    for b in range(3):
        _check_sample(out, b, ref[b], num_kp, bidirectional)


def test_a_built_batch_trains():
    """smoke: synth_captures -> make_zoom_batch -> training.compute_loss gives a finite loss"""
    pairs = [synth_captures(51, 480, 640), synth_captures(52, 480, 640)]
    gen = torch.Generator(device='cuda').manual_seed(0)
    batch = cotr_amd.make_zoom_batch([p[0] for p in pairs], [p[1] for p in pairs], 50, [1.0, 0.5, 0.25], 0.125, generator=gen)
    assert batch['valid'].all()
    m = build_model(cotr_amd.default_args(dropout=0.0)).cuda()
    m.load_state_dict(synth_state_dict(0))
    m.train()
    loss, pred = training.compute_loss(m, batch['image'], batch['queries'], batch['targets'])
    assert pred.shape == (2, 100, 2) and torch.isfinite(loss).item()
