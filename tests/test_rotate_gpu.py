"""cotr_rotate_captures and its Python callers on the MI355X against the numpy restatement (tests/rotate_oracle.py): image bytes
and depth bits IDENTICAL, at sizes below, at and above the 64 x 16 tile, with widths that are and are not multiples of the four
pixels a lane writes (both store paths); mixed items in one call; run-to-run, side-stream and graph-replay identity; the
property that pose and image turn the same way, through the device's depth_corrs; the batch builders with ``rotations``
against the oracle's assembly on oracle-rotated captures."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from cotr_amd import _lib, data
from cotr_amd.data import Capture
from cotr_amd.utils.synth import synth_captures
from tests import dataset_oracle as do
from tests import rotate_oracle as ro
from tests import warp_oracle as wo
from tests.test_dataset_gpu import MARGIN, _check_sample, _zoom_rand      # the tolerances of the batch-builder tests, as they are

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (5, 7), (16, 64), (64, 16), (63, 65), (255, 257), (480, 640)]
BIG = (1200, 1600)
ANGLES = [1e-3, 17, -23.5, 45, 90, 180, 270, 359.999, -720.25]


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """(image, depth) of a shape, computed once and left unchanged; the depth carries -0.0, denormals, infinities and NaNs with payloads"""
    return wo.image(shape[0], shape[1], 3, shape[0] + shape[1]), ro.depth_map(shape[0], shape[1], shape[0] * 7 + shape[1])


def _cap(shape, image=True):
    img, depth = _inputs(shape)
    return Capture(img if image else None, depth, np.eye(3), np.eye(4))


def _same(got, want_image, want_depth, what):
    """image bytes as bytes, depth as its int32 view"""
    assert got.image.is_cuda and got.depth.is_cuda and got.image.dtype == torch.uint8 and got.depth.dtype == torch.float32
    assert np.array_equal(got.image.cpu().numpy(), want_image), what
    assert np.array_equal(got.depth.cpu().numpy().view(np.int32), want_depth.view(np.int32)), what


def _special_values_present(depth):
    bits = depth.view(np.uint32)
    return (bits == 0x80000000).any() and (bits == 0x00000001).any() and np.isinf(depth).any() and (bits == 0x7FC12345).any()


# ---- identical to the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES)
def test_image_and_depth_are_identical_to_the_restatement(shape):
    cap = _cap(shape)
    assert _special_values_present(cap.depth) or shape[0] * shape[1] < 64
    got = data.rotate_captures([cap] * len(ANGLES), ANGLES)                 # every angle in one launch
    for a, g in zip(ANGLES, got):
        m = ro.matrix(shape, a)
        _same(g, ro.warp_linear(cap.image, m), ro.warp_nearest(cap.depth, m), (shape, a))
        assert g.K is cap.K and np.abs(g.c2w - ro.rotated_c2w(cap.c2w, a)).max() <= 1e-12
    single = data.rotate_capture(cap, ANGLES[1])
    assert torch.equal(single.image, got[1].image) and torch.equal(single.depth.view(torch.int32), got[1].depth.view(torch.int32))


@pytest.mark.parametrize('angle', ANGLES)
def test_a_large_capture_is_identical_to_the_restatement(angle):
    cap = _cap(BIG)
    assert _special_values_present(cap.depth)
    m = ro.matrix(BIG, angle)
    _same(data.rotate_capture(cap, angle), ro.warp_linear(cap.image, m), ro.warp_nearest(cap.depth, m), angle)


def test_special_depth_values_arrive_unchanged():
    """a quarter turn of a square moves every pixel but those of one row: the words of -0.0, a denormal, inf and a NaN with a
    payload are found at their new places bit for bit"""
    N = 64
    depth = ro.depth_map(N, N, 5)
    assert _special_values_present(depth)
    got = data.rotate_image(depth, 90, nearest=True).cpu().numpy()
    want = np.zeros_like(depth)
    for y in range(1, N):
        want[y] = depth[:, N - y]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and _special_values_present(got)


# ---- one call with mixed items ----------------------------------------------------------------------------------------------
def test_one_call_with_mixed_shapes_absent_halves_and_zero_angles():
    shapes = [(63, 65), (5, 7), (255, 257), (16, 64), (480, 640), (2, 3), (64, 16)]
    angles = [17.0, 0.0, -23.5, 45.0, 0.0, 359.999, 90.0]
    caps = [_cap(s, image=k not in (2, 3)) for k, s in enumerate(shapes)]   # two depth-only captures, one of them turned
    dev = Capture(torch.from_numpy(caps[4].image.copy()).cuda(), torch.from_numpy(caps[4].depth.copy()).cuda(), caps[4].K, caps[4].c2w)
    caps[4] = dev
    got = data.rotate_captures(caps, angles)
    assert len(got) == len(caps)
    for k, (c, a, g) in enumerate(zip(caps, angles, got)):
        if a == 0:
            assert g is c and g.image is c.image and g.depth is c.depth           # the very same objects
            continue
        m = ro.matrix(shapes[k], a)
        assert g.K is c.K and np.array_equal(g.c2w, data.rotated_c2w(c.c2w, a))
        assert np.array_equal(g.depth.cpu().numpy().view(np.int32), ro.warp_nearest(c.depth, m).view(np.int32)), k
        if c.image is None:
            assert g.image is None
        else:
            assert np.array_equal(g.image.cpu().numpy(), ro.warp_linear(c.image, m)), k
    assert got[4].image is dev.image and got[4].depth is dev.depth
    # all angles zero: nothing is launched, nothing is uploaded
    assert all(g is c for g, c in zip(data.rotate_captures(caps[:2], [0.0, 0]), caps[:2]))
    # at the table level an item may also lack its depth: image-only, depth-only and both in one launch
    d = torch.device('cuda', torch.cuda.current_device())
    img_a, dep_b = torch.from_numpy(_inputs((63, 65))[0].copy()).to(d), torch.from_numpy(_inputs((255, 257))[1].copy()).to(d)
    img_c, dep_c = (torch.from_numpy(x.copy()).to(d) for x in _inputs((5, 7)))
    ma, mb, mc = ro.matrix((63, 65), 17), ro.matrix((255, 257), -23.5), ro.matrix((5, 7), 45)
    out = data._rotate_launch([(img_a, None, ma), (None, dep_b, mb), (img_c, dep_c, mc)], d)
    assert out[0][1] is None and out[1][0] is None
    assert np.array_equal(out[0][0].cpu().numpy(), ro.warp_linear(img_a.cpu().numpy(), ma))
    assert np.array_equal(out[1][1].cpu().numpy().view(np.int32), ro.warp_nearest(dep_b.cpu().numpy(), mb).view(np.int32))
    assert np.array_equal(out[2][0].cpu().numpy(), ro.warp_linear(img_c.cpu().numpy(), mc))
    assert np.array_equal(out[2][1].cpu().numpy().view(np.int32), ro.warp_nearest(dep_c.cpu().numpy(), mc).view(np.int32))


# ---- determinism, streams, graphs ----------------------------------------------------------------------------------------------
def _device_caps():
    d = torch.device('cuda', 0)
    shapes, angles = [(255, 257), (63, 65), (480, 640)], [17.0, -23.5, 45.0]
    caps = [Capture(torch.from_numpy(_inputs(s)[0].copy()).to(d), torch.from_numpy(_inputs(s)[1].copy()).to(d), np.eye(3), np.eye(4))
            for s in shapes]
    return caps, angles


def _flat(caps):
    return [c.image for c in caps] + [c.depth.view(torch.int32) for c in caps]


def test_run_to_run_side_stream_and_graph_replay_are_bit_identical():
    caps, angles = _device_caps()
    ref = _flat(data.rotate_captures(caps, angles))
    for c, a, img, dep in zip(caps, angles, ref[:3], ref[3:]):
        m = ro.matrix(tuple(c.depth.shape), a)
        assert np.array_equal(img.cpu().numpy(), ro.warp_linear(c.image.cpu().numpy(), m))
        assert np.array_equal(dep.cpu().numpy(), ro.warp_nearest(c.depth.cpu().numpy(), m).view(np.int32))
    for _ in range(2):
        assert all(torch.equal(x, y) for x, y in zip(_flat(data.rotate_captures(caps, angles)), ref))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = _flat(data.rotate_captures(caps, angles))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(s, ref))
    # a graph holds the launch, not the table upload: the C entry point on tables and destinations made before the capture
    d = caps[0].depth.device
    outs = [(torch.zeros_like(c.image), torch.zeros_like(c.depth)) for c in caps]
    ptrs = torch.tensor([[c.image.data_ptr(), o[0].data_ptr(), c.depth.data_ptr(), o[1].data_ptr()] for c, o in zip(caps, outs)],
                        dtype=torch.int64).to(d)
    shapes = torch.tensor([tuple(c.depth.shape) for c in caps], dtype=torch.int32).to(d)
    mats = torch.from_numpy(np.stack([data.rotation_matrix(tuple(c.depth.shape), a) for c, a in zip(caps, angles)])).to(d)
    lib = _lib.load_library()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.cotr_rotate_captures(ctypes.c_void_p(ptrs.data_ptr()), ctypes.c_void_p(shapes.data_ptr()), ctypes.c_void_p(mats.data_ptr()),
                                      3, 480, 640, _lib.current_stream_ptr())
    assert rc == 0
    for _ in range(2):                                           # replayed twice, from cleared destinations
        for o in outs:
            o[0].fill_(0), o[1].fill_(0)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip([o[0] for o in outs] + [o[1].view(torch.int32) for o in outs], ref))


# ---- rotate_image ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, 7), (63, 65), (480, 640)])
def test_rotate_image_in_both_modes(shape):
    img, depth = _inputs(shape)
    for a in (17, -123.4, 0):
        m = ro.matrix(shape, a)
        got = data.rotate_image(img, a)
        assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ro.warp_linear(img, m))
        got = data.rotate_image(torch.from_numpy(depth.copy()).cuda(), a, nearest=True)
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.int32), ro.warp_nearest(depth, m).view(np.int32))
    assert np.array_equal(data.rotate_image(img, 0).cpu().numpy(), img)          # the identity copies


# ---- the geometric property on the device -------------------------------------------------------------------------------------
@pytest.mark.parametrize('angle', [17, -40, 90])
def test_pose_and_image_turn_the_same_way_on_the_device(angle):
    cap, m = ro.property_case(angle)
    rot = data.rotate_capture(cap, angle)
    assert np.array_equal(rot.depth.cpu().numpy(), ro.warp_nearest(cap.depth, m)) and rot.image is None
    rows = data.depth_corrs(rot, cap)                                # the rotated capture into the original, on the device
    ro.check_turns_the_same_way(cap, rot, m, rows.cpu().numpy())


# ---- the batch builders with rotations -------------------------------------------------------------------------------------------
ZOOM_SEEDS, ZOOM_ROT = (63, 163), np.array([[17.0, -23.5], [0.0, 45.0]])
BATCH_SEEDS, BATCH_ROT = (81, 181), np.array([[-40.0, 0.0], [90.0, 17.0]])
ZOOMS = [1.0, 0.7, 0.5]


def _oracle_rotated(pairs, rot):
    qs = [ro.rotate_capture(p[0], a) for p, a in zip(pairs, rot[:, 0])]
    ns = [ro.rotate_capture(p[1], a) for p, a in zip(pairs, rot[:, 1])]
    return qs, ns


@pytest.mark.parametrize('bidirectional', [True, False])
def test_make_zoom_batch_with_rotations_against_the_oracle(bidirectional):
    num_kp = 50
    pairs = [synth_captures(s, 96, 128) for s in ZOOM_SEEDS]
    qs, ns = [p[0] for p in pairs], [p[1] for p in pairs]
    rand = _zoom_rand(2, num_kp, 5)
    out = data.make_zoom_batch(qs, ns, num_kp, ZOOMS, 0.125, bidirectional=bidirectional, rand=rand, rotations=ZOOM_ROT)
    ref = do.make_zoom_batch(*_oracle_rotated(pairs, ZOOM_ROT), num_kp, ZOOMS, 0.125, bidirectional, rand)
    print([(r['valid'], r.get('boxes'), r.get('count'), r['margin']) for r in ref])
    assert sum(r['margin'] < MARGIN for r in ref) == 0               # NO candidate within round-off of a decision (scene chosen so)
    assert [r['valid'] for r in ref] == [True, True]
    for b in range(2):
        _check_sample(out, b, ref[b], num_kp, bidirectional)
    plain = data.make_zoom_batch(qs, ns, num_kp, ZOOMS, 0.125, bidirectional=bidirectional, rand=rand)
    assert not torch.equal(out['image'], plain['image'])             # the rotation did change the batch


@pytest.mark.parametrize('bidirectional', [True, False])
def test_make_batch_with_rotations_against_the_oracle(bidirectional):
    num_kp = 150
    pairs = [synth_captures(s, 256, 256) for s in BATCH_SEEDS]
    qs, ns = [p[0] for p in pairs], [p[1] for p in pairs]
    rand = {k: v for k, v in _zoom_rand(2, num_kp, 8).items() if k in ('trim', 'flip')}
    out = data.make_batch(qs, ns, num_kp, bidirectional=bidirectional, rand=rand, rotations=BATCH_ROT)
    ref = do.make_batch(*_oracle_rotated(pairs, BATCH_ROT), num_kp, bidirectional, rand)
    print([(r['valid'], r['margin']) for r in ref])
    assert sum(r['margin'] < MARGIN for r in ref) == 0
    assert [r['valid'] for r in ref] == [True, True]
    for b in range(2):
        _check_sample(out, b, ref[b], num_kp, bidirectional)


def test_rotations_none_and_all_zero_take_todays_path(monkeypatch):
    num_kp = 50
    pairs = [synth_captures(s, 96, 128) for s in ZOOM_SEEDS]
    qs, ns = [p[0] for p in pairs], [p[1] for p in pairs]
    rand = _zoom_rand(2, num_kp, 5)
    squares = [synth_captures(s, 256, 256) for s in BATCH_SEEDS]
    sq, sn = [p[0] for p in squares], [p[1] for p in squares]
    brand = {k: rand[k] for k in ('trim', 'flip')}
    turned = data.make_zoom_batch(qs, ns, num_kp, ZOOMS, 0.125, rand=rand, rotations=ZOOM_ROT)

    def no_launch(*a, **k):
        raise AssertionError('cotr_rotate_captures was launched')
    monkeypatch.setattr(data, '_rotate_launch', no_launch)           # not one launch more
    base = data.make_zoom_batch(qs, ns, num_kp, ZOOMS, 0.125, rand=rand)
    bbase = data.make_batch(sq, sn, num_kp, rand=brand)
    for rotations in (None, np.zeros((2, 2)), [[0, 0], [0.0, -0.0]]):
        got = data.make_zoom_batch(qs, ns, num_kp, ZOOMS, 0.125, rand=rand, rotations=rotations)
        assert all(torch.equal(got[k], base[k]) for k in base)
        got = data.make_batch(sq, sn, num_kp, rand=brand, rotations=rotations)
        assert all(torch.equal(got[k], bbase[k]) for k in bbase)
    assert not torch.equal(turned['image'], base['image'])
