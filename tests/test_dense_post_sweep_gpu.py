"""cotr_dense_merge, cotr_resize_f32 and cotr_dense_cycle at the sizes, values and launch shapes the engine tests do not
reach, bit for bit against Pillow's mode-'F' BILINEAR and the reference's recipes as restated in oracle/dense_post.py
(float_image_resize, merge_flow_patches, cycle_maps).  The cases come from tests/image_kernel_cases.py;
tests/test_image_kernel_cases_cpu.py checks without a GPU that they contain what is claimed here."""
import numpy as np
import pytest
import torch

from cotr_amd import _lib
from oracle import dense_post
from tests import image_kernel_cases as cases

pytestmark = pytest.mark.gpu

COTR_ERR_ARG = -1
SENTINEL = -77.25


def merge(maps_d, boxes, side, shape):
    """cotr_dense_merge -> (flow [H,W,2], conf [H,W]) float32 numpy."""
    lib = _lib.load_library()
    bx = torch.tensor([list(b) for b in boxes], dtype=torch.int32).cuda()
    flow = torch.full((shape[0], shape[1], 2), SENTINEL, device='cuda')
    conf = torch.full((shape[0], shape[1]), SENTINEL, device='cuda')
    _lib.check(lib.cotr_dense_merge(maps_d.data_ptr(), bx.data_ptr(), len(boxes), side, shape[0], shape[1], flow.data_ptr(),
                                    conf.data_ptr(), _lib.current_stream_ptr()), None, 'cotr_dense_merge')
    torch.cuda.synchronize()
    return flow.cpu().numpy(), conf.cpu().numpy()


def assert_same_bits(got, want, what):
    """got float32 == want (float64 holding float32 values), NaN where the reference has NaN, and the same sign of zero."""
    got = got.astype(np.float64)
    assert np.array_equal(got, want, equal_nan=True), (what, int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum()))
    ok = ~np.isnan(want)
    assert np.array_equal(np.signbit(got[ok]), np.signbit(want[ok])), what


@pytest.mark.parametrize('side', [0, 1])
def test_merge_at_every_patch_size_class(side):
    """Patch sizes 1 ... 2047 (256 taps per axis down to 2; the 256 copy path) in one image, overlapping, on the borders, with
    uncovered strips in between: float_image_resize + merge_flow_patches, flow and conf."""
    boxes, shape = cases.merge_size_boxes(side), cases.MERGE_SHAPES[side]
    assert sorted(b[2] for b in boxes) == list(cases.MERGE_SIZES)
    maps = cases.random_maps(len(boxes), 40 + side)
    want_flow, want_conf, cmap, _ = cases.merge_reference(maps, boxes, side, shape)
    assert (want_conf == 100).sum() > 0 and (cmap == -1).sum() == 0      # uncovered pixels: 100 ties with 100, an entry "wins" them
    flow, conf = merge(torch.from_numpy(maps).cuda(), boxes, side, shape)
    assert_same_bits(conf, want_conf, 'conf')
    assert_same_bits(flow, want_flow, 'flow')


@pytest.mark.parametrize('side', [0, 1])
def test_merge_of_special_error_planes(side):
    """Ties, NaN in the earlier / the later / both entries, errors above 100, exactly 100, +inf, -0 against +0, NaN / inf /
    1e30 in the x / y planes: whatever merge_flow_patches (numpy's argmin) and Pillow's double accumulation make of them."""
    boxes, shape = cases.SPECIAL_BOXES[side], cases.SPECIAL_SHAPES[side]
    maps = cases.special_maps()
    want_flow, want_conf, cmap, entries = cases.merge_reference(maps, boxes, side, shape)
    found = cases.merge_situations(entries, want_flow, want_conf, cmap)
    assert all(v > 0 for v in found.values()), found
    flow, conf = merge(torch.from_numpy(maps).cuda(), boxes, side, shape)
    assert_same_bits(conf, want_conf, 'conf')
    assert_same_bits(flow, want_flow, 'flow')


@pytest.mark.parametrize('n_pairs', [1, 9])
@pytest.mark.parametrize('side', [0, 1])
def test_merge_of_one_and_of_nine_pairs(n_pairs, side):
    pairs = cases.nine_pairs()[:n_pairs]
    boxes, shape = [p[side] for p in pairs], cases.NINE_SHAPES[side]
    maps = cases.random_maps(n_pairs, 50 + n_pairs)
    want_flow, want_conf, _, _ = cases.merge_reference(maps, boxes, side, shape)
    flow, conf = merge(torch.from_numpy(maps).cuda(), boxes, side, shape)
    assert_same_bits(conf, want_conf, 'conf')
    assert_same_bits(flow, want_flow, 'flow')


def test_merge_argument_errors():
    """side outside {0, 1}, H * W above 2^30, a NULL pointer, no pairs: COTR_ERR_ARG from the host, nothing written."""
    lib = _lib.load_library()
    maps = torch.from_numpy(cases.random_maps(1, 0)).cuda()
    bx = torch.tensor([[0, 0, 16]], dtype=torch.int32).cuda()
    flow = torch.full((16, 16, 2), SENTINEL, device='cuda')
    conf = torch.full((16, 16), SENTINEL, device='cuda')
    s = _lib.current_stream_ptr()
    m, b, f, c = maps.data_ptr(), bx.data_ptr(), flow.data_ptr(), conf.data_ptr()
    bad = [(m, b, 1, 2, 16, 16, f, c), (m, b, 1, -1, 16, 16, f, c), (m, b, 1, 0, 32768, 32769, f, c), (m, b, 1, 0, 0, 16, f, c),
           (m, b, 1, 0, 16, -1, f, c), (m, b, 0, 0, 16, 16, f, c), (None, b, 1, 0, 16, 16, f, c), (m, None, 1, 0, 16, 16, f, c),
           (m, b, 1, 0, 16, 16, None, c), (m, b, 1, 0, 16, 16, f, None)]
    for args in bad:
        assert lib.cotr_dense_merge(*args, s) == COTR_ERR_ARG, args
    torch.cuda.synchronize()
    assert bool((flow == SENTINEL).all()) and bool((conf == SENTINEL).all())
    assert lib.cotr_dense_merge(m, b, 1, 0, 32768, 32768, None, c, s) == COTR_ERR_ARG      # 2^30 itself passes the size check
    assert lib.cotr_dense_merge(m, b, 1, 1, 16, 16, f, c, s) == 0
    torch.cuda.synchronize()
    assert not bool((conf == SENTINEL).any())


def resize(arr, dst_shape):
    lib = _lib.load_library()
    src = torch.from_numpy(arr).cuda()
    dst = torch.full((dst_shape[0], dst_shape[1], arr.shape[2]), SENTINEL, device='cuda')
    _lib.check(lib.cotr_resize_f32(src.data_ptr(), arr.shape[0], arr.shape[1], arr.shape[2], dst.data_ptr(), dst_shape[0],
                                   dst_shape[1], _lib.current_stream_ptr()), None, 'cotr_resize_f32')
    torch.cuda.synchronize()
    return dst.cpu().numpy()


@pytest.mark.parametrize('channels', [1, 2, 3])
@pytest.mark.parametrize('src_shape,dst_shape', cases.resize_cases())
def test_resize_f32_on_every_path(src_shape, dst_shape, channels):
    """{up, down, same} x {up, down, same}, 1-pixel axes on either end, 2048 <-> 3: utils.float_image_resize, bit for bit."""
    arr = cases.resize_input(src_shape, channels)
    want = dense_post.float_image_resize(arr, dst_shape)
    got = resize(arr, dst_shape)
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(np.signbit(got), np.signbit(want))


@pytest.mark.parametrize('src_shape,dst_shape', cases.resize_cases()[:9] + [((64, 48), (7, 5)), ((7, 5), (64, 48))])
def test_resize_f32_with_nan_inf_and_huge_values(src_shape, dst_shape):
    arr = cases.resize_input(src_shape, 3, special=True)
    want = dense_post.float_image_resize(arr, dst_shape)
    assert np.isnan(want).any() and np.isinf(want).any()
    got = resize(arr, dst_shape)
    assert np.array_equal(got, want, equal_nan=True)
    ok = ~np.isnan(want)
    assert np.array_equal(np.signbit(got[ok]), np.signbit(want[ok]))


@pytest.mark.parametrize('n_pairs', [1, 9])
def test_dense_cycle_of_one_and_of_nine_pairs(n_pairs):
    """cotr_dense_cycle with the affines of 3 x 3 patches of two non-square images vs cycle_maps + affine of the host recipe."""
    from cotr_amd.inference.zoom_engine import _patch_affines
    from tests.engine_fixtures import CyclicFakeModel
    pairs = cases.nine_pairs()[:n_pairs]
    shape_a, shape_b = cases.NINE_SHAPES
    jj, ii = np.meshgrid(np.arange(512), np.arange(256))
    q = torch.from_numpy(np.stack([jj / 512, ii / 256], -1).reshape(1, -1, 2)).float().expand(n_pairs, -1, -1)
    rng = np.random.default_rng(90 + n_pairs)
    img = torch.from_numpy(rng.standard_normal((n_pairs, 3, 256, 512)).astype(np.float32))
    pred = CyclicFakeModel()(img, q)['pred_corrs'].view(n_pairs, 256, 512, 2).clone()
    noise = torch.from_numpy(rng.standard_normal((n_pairs, 256, 512, 2)).astype(np.float32))
    pred[:, ::7, ::5] += noise[:, ::7, ::5]                      # answers far outside [0,1]: grid_sample's zero padding
    aff = np.stack([np.stack(_patch_affines(p_i, p_j, shape_a, shape_b)) for p_i, p_j in pairs])
    assert len({a.tobytes() for a in aff}) == n_pairs and not np.array_equal(aff[0][0], np.array([[1., 0, 0], [0, 1, 0]]))
    lib = _lib.load_library()
    aff_d = torch.from_numpy(np.ascontiguousarray(aff)).cuda()
    pred_d = pred.cuda()
    maps = torch.full((n_pairs, 256, 512, 3), SENTINEL, device='cuda')
    _lib.check(lib.cotr_dense_cycle(pred_d.data_ptr(), n_pairs, aff_d.data_ptr(), maps.data_ptr(), _lib.current_stream_ptr()),
               None, 'cotr_dense_cycle')
    got = maps.cpu().numpy()
    for k, (p_i, p_j) in enumerate(pairs):
        c_i, c_j = dense_post.cycle_maps(pred[k].numpy())
        t_i, t_j = dense_post.patch_affines(p_i, p_j, shape_a, shape_b)
        c_i[..., :2] = c_i[..., :2] @ t_i[:2, :2] + t_i[:, 2]
        c_j[..., :2] = c_j[..., :2] @ t_j[:2, :2] + t_j[:, 2]
        want = np.concatenate([c_i, c_j], axis=1)
        assert np.array_equal(got[k][..., :2], want[..., :2]), k
        assert np.array_equal(got[k][..., 2], want[..., 2]), k
