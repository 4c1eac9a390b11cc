"""The inputs of the image-kernel sweeps (tests/image_kernel_cases.py) are what the GPU tests claim they are, checked
without a GPU: the crop cases go through the numpy restatement of Pillow's 8-bit resample against Pillow itself, the
plain-Python LDS budget gives the tile-height bands the GPU test wants one launch in, the header states the limit that
budget ends at, and the reference's merge of the special planes really contains every situation the kernel must get right."""
import numpy as np
import pytest

from oracle.pil_resize import crop_resize_normalize
from tests import image_kernel_cases as cases


def _restated(img_a, img_b, boxes):
    return np.stack([crop_resize_normalize(img_a, img_b, tuple(b[:3]), tuple(b[3:])) for b in np.asarray(boxes).tolist()])


def test_every_8th_crop_size_matches_pillow_bit_for_bit():
    img_a, img_b = (cases.random_image(s, k) for k, s in enumerate(cases.SWEEP_SHAPES))
    launches = cases.every_size_launches(stride=8)
    for side in (0, 1):
        assert sorted(int(b[2 + 3 * side]) for boxes in launches for b in boxes) == list(range(2, 601, 8))
    for boxes in launches:
        assert np.array_equal(_restated(img_a, img_b, boxes), cases.pillow_crop_reference(img_a, img_b, boxes).numpy())


def test_ladder_up_to_1281_matches_pillow_bit_for_bit():
    img_a, img_b = (cases.random_image(s, 10 + k) for k, s in enumerate(cases.LADDER_SHAPES))
    boxes = cases.ladder_boxes(last=1281)
    assert {601, 767, 768, 769, 1023, 1024, 1025, 1279, 1280, 1281} <= set(boxes[:, 2].tolist()) & set(boxes[:, 5].tolist())
    assert np.array_equal(_restated(img_a, img_b, boxes), cases.pillow_crop_reference(img_a, img_b, boxes).numpy())


def test_sweeps_cover_what_they_promise():
    launches = cases.every_size_launches()
    for side in (0, 1):
        assert sorted(int(b[2 + 3 * side]) for boxes in launches for b in boxes) == list(range(2, 601))
    assert all(32 <= len(boxes) <= 64 for boxes in launches)
    # small and large crops share every launch
    assert all(boxes[:, [2, 5]].min() < 64 and boxes[:, [2, 5]].max() > 500 for boxes in launches)
    ladder = cases.ladder_boxes()
    need = {601, 767, 768, 769, 1023, 1024, 1025, 1279, 1280, 1281, 2047, 2048, 2049, 3295, 3296} | set(cases.SMALL_SIZES)
    assert need <= set(ladder[:, 2].tolist()) and need <= set(ladder[:, 5].tolist())
    for boxes, (shape_a, shape_b) in [(b, cases.SWEEP_SHAPES) for b in launches] + [(ladder, cases.LADDER_SHAPES)] + \
            [(cases.band_boxes(s), (cases.BIG_SHAPE, cases.BIG_SHAPE)) for s in cases.BAND_SIZES] + \
            [(cases.border_boxes(*cases.SWEEP_SHAPES), cases.SWEEP_SHAPES)]:
        for k, (h, w) in ((0, shape_a), (3, shape_b)):                  # every box inside its image
            x, y, s = boxes[:, k], boxes[:, k + 1], boxes[:, k + 2]
            assert (x >= 0).all() and (y >= 0).all() and (s >= 2).all() and (x + s <= w).all() and (y + s <= h).all()
    assert all(w % 4 for _, w in cases.SWEEP_SHAPES + cases.LADDER_SHAPES)


def test_lds_budget_formula_gives_the_band_edges_and_the_header_limit():
    """launch_crop_resize's choice of R, written out in Python: R = 8 up to 3296, 4 up to 4864, 2 up to 6528, 1 up to 7936,
    no fit from 7937; include/cotr_hip.h states that last size as COTR_CROP_MAX_SIZE."""
    rows = [cases.crop_tile_rows(m) for m in range(0, 16385)]
    for r, (first, last) in cases.BAND_EDGES.items():
        assert set(rows[first:last + 1]) == {r}, r
    assert set(rows[7937:]) == {0}
    assert [rows[m] for m in (3296, 3297, 4864, 4865, 6528, 6529, 7936, 7937)] == [8, 4, 4, 2, 2, 1, 1, 0]
    assert cases.header_crop_limit() == 7936 == cases.BAND_EDGES[1][1] == max(cases.BAND_SIZES)
    assert {cases.crop_tile_rows(s) for s in cases.BAND_SIZES} == {8, 4, 2, 1}


def test_launcher_source_states_the_restated_budget():
    """cases.crop_tile_rows restates these lines of launch_crop_resize; a change of the budget there has to come here too
    (the row window has 4 or more spare rows in every band, so no output would show a max_rows that is one too small)."""
    import os
    src = ' '.join(open(os.path.join(cases.ROOT, 'cotr_amd', 'csrc', 'crop_resize.hip')).read().split())
    for line in ('const double scale = max_size > OUT ? (double)max_size / OUT : 1.0;', 'const int sup = (int)ceil(scale);',
                 'const int ksize = sup * 2 + 1;', 'int R = 8;', 'for (; R >= 1; R >>= 1) {',
                 'max_rows = (int)ceil(R * scale) + 2 * sup + 3;',
                 'bytes = (size_t)max_rows * OUT * 4 + (size_t)OUT * ksize * 4 + (size_t)R * ksize * 4 + (size_t)R * 8;',
                 'if (bytes <= 160 * 1024) break;', '#define OUT 256'):
        assert line in src, line
    assert cases.LDS_BUDGET == 160 * 1024 and cases.OUT == 256


def test_lds_rows_suffice_in_every_band():
    """The row window of a workgroup (first input row of its first output row to one past the last input row of its last) never
    exceeds the launcher's max_rows, nor the tap count its ksize, for a box of any size <= max_size - checked at the band
    edges, where the budget is tightest, with Pillow's own bounds arithmetic."""
    import math
    for max_size in (2, 255, 256, 257, 600, 3296, 3297, 4864, 4865, 6528, 6529, 7936):
        r = cases.crop_tile_rows(max_size)
        scale = max(max_size / 256, 1.0)
        sup = math.ceil(scale)
        max_rows, ksize = math.ceil(r * scale) + 2 * sup + 3, 2 * sup + 1
        for size in {2, 3, 255, 256, 257, max_size - 1, max_size} - {1}:
            sc = size / 256
            support = max(sc, 1.0)
            yy = np.arange(256)
            center = (yy + 0.5) * sc
            lo = np.maximum((center - support + 0.5).astype(np.int64), 0)
            hi = np.minimum((center + support + 0.5).astype(np.int64), size)
            assert (hi - lo).max() <= ksize, (max_size, size)
            window = hi[r - 1::r] - lo[::r]
            assert window.max() <= max_rows, (max_size, size, int(window.max()), max_rows)


@pytest.mark.parametrize('side', [0, 1])
def test_merge_size_boxes_overlap_touch_borders_and_leave_gaps(side):
    boxes = cases.merge_size_boxes(side)
    assert sorted(b[2] for b in boxes) == list(cases.MERGE_SIZES)
    geo = cases.box_geometry(boxes, cases.MERGE_SHAPES[side])
    assert geo['every_box_overlaps'] and geo['borders'] == (True, True, True, True)
    assert geo['uncovered'] > 0 and geo['uncovered_between'] > 0


@pytest.mark.parametrize('side', [0, 1])
def test_special_merge_planes_contain_every_situation(side):
    """Exact ties, NaN in the earlier / later / both entries, errors above 100, exactly 100, +inf, -0 against +0, NaN in the
    flow, uncovered pixels between patches: each occurs in the reference's own merge of the special planes."""
    maps = cases.special_maps()
    flow, conf, cmap, entries = cases.merge_reference(maps, cases.SPECIAL_BOXES[side], side, cases.SPECIAL_SHAPES[side])
    found = cases.merge_situations(entries, flow, conf, cmap)
    assert all(v > 0 for v in found.values()), found
    assert np.signbit(conf[conf == 0]).any() and not np.signbit(conf[conf == 0]).all()     # both zeros survive the merge


@pytest.mark.parametrize('special', [False, True])
def test_resize_inputs_cover_every_path(special):
    combos = {(np.sign(d[0] - s[0]), np.sign(d[1] - s[1])) for s, d in cases.resize_cases()}
    assert len(combos) == 9
    shapes = cases.resize_cases()
    assert any(s[0] == 1 for s, _ in shapes) and any(s[1] == 1 for s, _ in shapes)
    assert any(d[0] == 1 for _, d in shapes) and any(d[1] == 1 for _, d in shapes)
    assert ((2048, 2048), (3, 3)) in shapes and ((3, 3), (2048, 2048)) in shapes
    arr = cases.resize_input((37, 53), 3, special=special)
    assert np.isnan(arr).any() == special and np.isinf(arr).any() == special and (arr == np.float32(1e30)).any() == special
