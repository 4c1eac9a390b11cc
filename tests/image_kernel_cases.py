"""Case generators for the sweeps of the engine's image kernels (crop_resize.hip, dense_post.hip) and the references they
are held against: Pillow itself (8-bit and mode-'F' BILINEAR) and the reference's recipes in oracle/dense_post.py.
Imported by the GPU sweeps (tests/test_crop_resize_sweep_gpu.py, tests/test_dense_post_sweep_gpu.py) and by
tests/test_image_kernel_cases_cpu.py, which checks on the CPU that the inputs are what the sweeps claim they are (the
tile-height bands, the situations in the merge planes).  Everything is generated from a seed.  Test infrastructure."""
import math
import os
import re

import numpy as np
import PIL.Image
import torch

from oracle import dense_post

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- cotr_crop_resize_pairs: the launcher's LDS budget, written out -----------------------------------------------------
LDS_BUDGET = 160 * 1024
OUT = 256
BAND_EDGES = {8: (2, 3296), 4: (3297, 4864), 2: (4865, 6528), 1: (6529, 7936)}   # R -> (first, last) max_size


def crop_tile_rows(max_size):
    """Output rows per workgroup (R) that launch_crop_resize picks for ``max_size``; 0 = no R fits the budget."""
    scale = max_size / OUT if max_size > OUT else 1.0
    sup = math.ceil(scale)
    ksize = 2 * sup + 1
    for rows in (8, 4, 2, 1):
        max_rows = math.ceil(rows * scale) + 2 * sup + 3
        if max_rows * OUT * 4 + OUT * ksize * 4 + rows * ksize * 4 + rows * 8 <= LDS_BUDGET:
            return rows
    return 0


def header_crop_limit():
    """COTR_CROP_MAX_SIZE as include/cotr_hip.h states it."""
    src = open(os.path.join(ROOT, 'include', 'cotr_hip.h')).read()
    found = re.findall(r'^#define COTR_CROP_MAX_SIZE (\d+)\b', src, flags=re.M)
    assert len(found) == 1, found
    return int(found[0])


# ---- crop cases ------------------------------------------------------------------------------------------------------
SWEEP_SHAPES = ((611, 797), (701, 623))            # (H, W) of images A and B: non-square, different, widths % 4 != 0
LADDER = [601, 767, 768, 769, 1023, 1024, 1025, 1279, 1280, 1281, 1535, 1536, 1537, 1791, 1792, 1793, 2047, 2048, 2049,
          2303, 2304, 2305, 2559, 2560, 2561, 2815, 2816, 2817, 3071, 3072, 3073, 3295, 3296]
LADDER_SHAPES = ((3301, 3399), (3397, 3298))
SMALL_SIZES = (2, 18, 255, 256, 257)
BIG_SHAPE = (7936, 7940)
BAND_SIZES = (3296, 3297, 4864, 4865, 6528, 6529, 7936)


def random_image(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, tuple(shape) + (3,), dtype=np.uint8)


def big_image():
    """7936 x 7940 x 3 uint8 (189 MB): per channel a different smooth gradient plus +-8 of noise, so that a tap that is off
    by one row or column, or a wrong weight, moves the result."""
    h, w = BIG_SHAPE
    rng = np.random.default_rng(7936)
    yy, xx = np.arange(h, dtype=np.float32)[:, None], np.arange(w, dtype=np.float32)[None, :]
    img = np.empty((h, w, 3), dtype=np.uint8)
    for c, (fx, fy) in enumerate(((255.0 / w, 0.0), (0.0, 255.0 / h), (130.0 / w, 120.0 / h))):
        plane = xx * np.float32(fx) + yy * np.float32(fy)
        plane += rng.integers(-8, 9, (h, w), dtype=np.int8)
        img[..., c] = np.clip(plane, 0, 255)
    return img


def place_boxes(sizes_a, sizes_b, shape_a, shape_b, rng):
    """Random in-image positions for the given crop sizes -> int32 [n,6] (xa, ya, sa, xb, yb, sb)."""
    rows = []
    for sa, sb in zip(sizes_a, sizes_b):
        assert 2 <= sa <= min(shape_a) and 2 <= sb <= min(shape_b), (sa, sb)
        rows.append((int(rng.integers(0, shape_a[1] - sa + 1)), int(rng.integers(0, shape_a[0] - sa + 1)), int(sa),
                     int(rng.integers(0, shape_b[1] - sb + 1)), int(rng.integers(0, shape_b[0] - sb + 1)), int(sb)))
    return np.array(rows, dtype=np.int32)


def every_size_launches(stride=1, seed=600):
    """Crop sizes 2 ... 600 (every ``stride``-th), each once on side A and once on side B, shuffled independently per side so that
    small and large crops share a launch; launches of at most 60 tasks.  -> list of int32 [n,6] boxes for SWEEP_SHAPES."""
    rng = np.random.default_rng(seed)
    sizes = np.arange(2, 601, stride)
    side_a, side_b = rng.permutation(sizes), rng.permutation(sizes)
    return [place_boxes(side_a[i:i + 60], side_b[i:i + 60], SWEEP_SHAPES[0], SWEEP_SHAPES[1], rng)
            for i in range(0, len(sizes), 60)]


def ladder_boxes(last=3296, seed=3296):
    """The ladder (each size on side A, the reversed ladder on side B) followed by the small sizes on both sides, for
    LADDER_SHAPES; ``last`` thins it for the CPU."""
    rng = np.random.default_rng(seed)
    sizes = [s for s in LADDER if s <= last]
    side_a = sizes + list(SMALL_SIZES)
    side_b = sizes[::-1] + list(SMALL_SIZES[::-1])
    return place_boxes(side_a, side_b, LADDER_SHAPES[0], LADDER_SHAPES[1], rng)


def band_boxes(size, seed=0):
    """One launch of the tile-height cases: the large crop once on side A and once on side B, next to the small sizes, all in
    BIG_SHAPE (the same image on both sides)."""
    rng = np.random.default_rng(size + seed)
    side_a = [size, 2, 18, 255, 256, 257]
    side_b = [257, size, 256, 18, 2, 255]
    return place_boxes(side_a, side_b, BIG_SHAPE, BIG_SHAPE, rng)


def border_boxes(shape_a, shape_b):
    """Boxes on every border of both images: the four corners, the middle of each edge, the largest square at both ends,
    a 2x2 crop in the last row / column."""
    def one(shape):
        h, w = shape
        s, big = 37, min(h, w)
        out = [(0, 0, s), (w - s, 0, s), (0, h - s, s), (w - s, h - s, s),                      # corners
               (w // 2 - 20, 0, s), (w // 2 - 20, h - s, s), (0, h // 2 - 20, s), (w - s, h // 2 - 20, s),   # edges
               (0, 0, big), (w - big, h - big, big),                                              # whole short side
               (w - 2, h - 2, 2), (0, h - 2, 2), (w - 2, 0, 2), (w - 256, h - 256, 256), (w - 257, h - 257, 257)]
        return out
    a, b = one(shape_a), one(shape_b)
    return np.array([list(p) + list(q) for p, q in zip(a, b[::-1])], dtype=np.int32)


def pillow_crop_reference(img_a, img_b, boxes):
    """The reference's recipe (refinement_task.py:105-120) with Pillow itself and torch's to_tensor / normalize arithmetic."""
    mean = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    out = []
    for xa, ya, sa, xb, yb, sb in np.asarray(boxes).tolist():
        ha = np.array(PIL.Image.fromarray(img_a[ya:ya + sa, xa:xa + sa]).resize((256, 256), resample=PIL.Image.BILINEAR))
        hb = np.array(PIL.Image.fromarray(img_b[yb:yb + sb, xb:xb + sb]).resize((256, 256), resample=PIL.Image.BILINEAR))
        canvas = np.concatenate([ha, hb], axis=1)
        t = torch.from_numpy(canvas.transpose(2, 0, 1).copy()).float().div(255)
        out.append((t - mean) / std)
    return torch.stack(out)


# ---- cotr_dense_merge cases ---------------------------------------------------------------------------------------------
MERGE_SIZES = (1, 2, 3, 5, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 1000, 2047)
MERGE_SHAPES = ((2060, 2200), (2210, 2055))          # (H, W) of the images of side 0 and side 1


def merge_size_boxes(side):
    """All of MERGE_SIZES in one image, (x, y, size) in entry order: every box overlaps another one, all four image borders
    are touched, and strips between the boxes stay uncovered."""
    h, w = MERGE_SHAPES[side]
    boxes = [(w - 2047, h - 2047, 2047),          # right and bottom border
             (0, 0, 1000),                          # top-left corner, overlaps the first
             (0, h - 513, 513),                     # bottom-left: the strip between it and the 1000-box stays uncovered
             (w - 512, 0, 512),                     # top-right
             (700, 700, 511), (950, 950, 300), (1100, 1100, 257), (1200, 1000, 256), (1300, 1200, 255),
             (1350, 1250, 129), (1400, 1300, 128), (1450, 1350, 127),
             (w - 2047 - 2, h - 2047 - 2, 5), (w - 2047 - 1, h - 2047 - 1, 3), (w - 2047, h - 2047 - 1, 2),
             (w - 2047 + 1, h - 2047, 1)]
    order = np.random.default_rng(side).permutation(len(boxes))
    boxes = [boxes[i] for i in order]
    assert sorted(b[2] for b in boxes) == sorted(MERGE_SIZES)
    return boxes


def random_maps(n, seed):
    """[n,256,512,3] float32: random x / y planes, cycle errors |N(0,1)| * 0.05 with a band of exact ties."""
    rng = np.random.default_rng(seed)
    maps = rng.standard_normal((n, 256, 512, 3)).astype(np.float32)
    maps[..., 2] = np.abs(maps[..., 2]) * 0.05
    maps[:, 100:140, :, 2] = 0.01
    return maps


SPECIAL_ERRORS = (0.01, np.nan, 150.0, 100.0, np.inf, -0.0, 0.0, None)     # None: the random values stay
SPECIAL_SHAPES = ((400, 520), (430, 390))
SPECIAL_BOXES = (((10, 10, 300), (30, 20, 290), (150, 130, 256), (330, 40, 60), (420, 300, 100), (415, 295, 30), (170, 140, 256)),
                 ((0, 0, 290), (20, 30, 300), (60, 100, 256), (330, 10, 60), (290, 330, 100), (285, 325, 30), (80, 120, 256)))


def _column_bands(plane):
    """SPECIAL_ERRORS in eight column bands of both halves of a [256,512] error plane."""
    for k, v in enumerate(SPECIAL_ERRORS):
        if v is not None:
            plane[:, 32 * k:32 * k + 32] = v
            plane[:, 256 + 32 * k:256 + 32 * k + 32] = v


def _row_bands(plane):
    """The same values in eight row bands, 0.0 and -0.0 swapped."""
    later = list(SPECIAL_ERRORS)
    later[5], later[6] = later[6], later[5]
    for k, v in enumerate(later):
        if v is not None:
            plane[32 * k:32 * k + 32, :] = v


def _sprinkle(planes, rng, count):
    """NaN, +-inf and 1e30 at random places of the x / y planes [256,512,2]."""
    flat = planes.reshape(-1)
    where = rng.choice(flat.size, 4 * count, replace=False)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e30)):
        flat[where[k::4]] = v


def special_maps(seed=2):
    """[7,256,512,3] for SPECIAL_BOXES.  Entries 0 (resized up) and 2 (size 256: the copy path, where -0.0 survives) carry
    SPECIAL_ERRORS in column bands of their error planes, the later entries 1 and 6, which overlap them, the same values in
    row bands: where the boxes overlap, every value of the earlier entry meets every value of the later one - exact ties,
    NaN in the earlier / the later / both, > 100, exactly 100, +inf, -0 against +0.  Entries 0 - 2 have NaN / +-inf / 1e30
    in their x / y planes, entry 3 (alone in its corner) is above 100 everywhere, entry 4 is exactly 100 with entry 5
    (lower errors, NaN in its lower half) on top of it."""
    rng = np.random.default_rng(seed)
    maps = rng.standard_normal((7, 256, 512, 3)).astype(np.float32)
    maps[..., 2] = np.abs(maps[..., 2]) * 0.05
    for k in (0, 2):
        plane = maps[k, ..., 2]
        _column_bands(plane)
    for k in (1, 6):
        plane = maps[k, ..., 2]
        _row_bands(plane)
    for k in (0, 1, 2):
        xy = np.ascontiguousarray(maps[k, ..., :2])
        _sprinkle(xy, rng, 60)
        maps[k, ..., :2] = xy
    maps[3, ..., 2] = 100.0 + np.abs(maps[3, ..., 2]) * 1000
    maps[4, ..., 2] = 100.0
    maps[5, 128:, :, 2] = np.nan
    return maps


def merge_entries(maps, boxes, side, shape):
    """What inference_helper.py:159-160 hands to merge_flow_patches: every entry's half resized to its patch with Pillow."""
    entries = []
    for k, (x, y, s) in enumerate(boxes):
        half = np.ascontiguousarray(maps[k][:, side * 256:(side + 1) * 256])
        entries.append((dense_post.float_image_resize(half, (s, s)), x, y, s, s, shape[1], shape[0]))
    return entries


def merge_reference(maps, boxes, side, shape):
    """-> (flow [H,W,2], conf [H,W], cmap [H,W], entries) of the reference's recipe."""
    entries = merge_entries(maps, boxes, side, shape)
    flow, conf, cmap = dense_post.merge_flow_patches(entries)
    return flow, conf, cmap, entries


def merge_situations(entries, flow, conf, cmap):
    """Counts of the situations the merge must get right, taken from the REFERENCE's inputs and result: per name the
    number of pixels of the image where it occurs."""
    h, w = conf.shape
    n = len(entries)
    cover = np.zeros((n, h, w), dtype=bool)
    err = np.zeros((n, h, w), dtype=np.float32)
    for k, (patch, x, y, pw, ph, _, _) in enumerate(entries):
        cover[k, y:y + ph, x:x + pw] = True
        err[k, y:y + ph, x:x + pw] = patch[..., 2]
    nan = cover & np.isnan(err)
    out = {'uncovered': int((~cover.any(0)).sum()), 'nan_conf': int(np.isnan(conf).sum()),
           'above_100_loses': int(((cover & (err > 100) & ~np.isinf(err)).any(0) & (conf == 100)).sum()),
           'exactly_100': int((cover & (err == 100)).any(0).sum()), 'inf': int((cover & np.isposinf(err)).any(0).sum()),
           'nan_in_flow': int(np.isnan(flow).sum()), 'tie_later_wins': 0, 'nan_earlier_only': 0, 'nan_later_only': 0, 'nan_both': 0,
           'neg_zero_then_zero': 0, 'zero_then_neg_zero': 0,
           'uncovered_between': int((~cover.any(0) & (np.cumsum(cover.any(0), 1) > 0)
                                     & (np.cumsum(cover.any(0)[:, ::-1], 1)[:, ::-1] > 0)).sum())}
    with np.errstate(invalid='ignore'):
        for i in range(n):
            for j in range(i + 1, n):
                both = cover[i] & cover[j]
                if not both.any():
                    continue
                tie = both & (err[i] == err[j]) & (conf == err[j]) & (err[j] != 100)
                out['tie_later_wins'] += int((tie & (cmap >= j)).sum())
                out['nan_earlier_only'] += int((both & nan[i] & ~nan[j]).sum())
                out['nan_later_only'] += int((both & ~nan[i] & nan[j]).sum())
                out['nan_both'] += int((both & nan[i] & nan[j]).sum())
                zero = both & (err[i] == 0) & (err[j] == 0)
                out['neg_zero_then_zero'] += int((zero & np.signbit(err[i]) & ~np.signbit(err[j])).sum())
                out['zero_then_neg_zero'] += int((zero & ~np.signbit(err[i]) & np.signbit(err[j])).sum())
    return out


# ---- cotr_resize_f32 cases ----------------------------------------------------------------------------------------------
def resize_cases():
    """(src (H, W), dst (H, W)): {up, down, same} per axis in all nine combinations, then the edges."""
    src = (37, 53)
    heights = {'up': 91, 'down': 11, 'same': 37}
    widths = {'up': 140, 'down': 17, 'same': 53}
    cases = [(src, (heights[v], widths[hz])) for v in ('up', 'down', 'same') for hz in ('up', 'down', 'same')]
    cases += [((1, 53), (40, 53)), ((1, 53), (40, 20)), ((37, 1), (37, 64)), ((37, 1), (5, 64)), ((1, 1), (7, 9)),     # 1-pixel source
              ((37, 53), (1, 53)), ((37, 53), (37, 1)), ((37, 53), (1, 1)), ((37, 53), (1, 200)),                      # 1-pixel destination
              ((2048, 5), (3, 5)), ((5, 2048), (5, 3)), ((2048, 2048), (3, 3)),                                        # strong down-scale
              ((3, 5), (2048, 5)), ((5, 3), (5, 2048)), ((3, 3), (2048, 2048))]                                        # strong up-scale
    return cases


def resize_input(src_shape, channels, special=False):
    rng = np.random.default_rng(src_shape[0] * 7 + src_shape[1] * 3 + channels)
    arr = rng.standard_normal(tuple(src_shape) + (channels,)).astype(np.float32)
    arr[::7, ::5] = 100.0
    if special:
        flat = arr.reshape(-1)
        where = rng.choice(flat.size, max(4, flat.size // 50), replace=False)
        for k, v in enumerate((np.nan, np.inf, -np.inf, 1e30)):
            flat[where[k::4]] = v
    return arr


def box_geometry(boxes, shape):
    """What the placement of (x, y, size) boxes in an [H, W] image offers: does every box overlap another one, which image
    borders are touched, how many pixels stay uncovered, how many of those lie between covered pixels of their row."""
    h, w = shape
    count = np.zeros((h, w), dtype=np.int32)
    for x, y, s in boxes:
        assert 0 <= x and 0 <= y and x + s <= w and y + s <= h and s >= 1, (x, y, s)
        count[y:y + s, x:x + s] += 1
    covered = count > 0
    between = ~covered & (np.cumsum(covered, 1) > 0) & (np.cumsum(covered[:, ::-1], 1)[:, ::-1] > 0)
    return {'every_box_overlaps': all(bool((count[y:y + s, x:x + s] > 1).any()) for x, y, s in boxes),
            'borders': (bool(covered[0].any()), bool(covered[-1].any()), bool(covered[:, 0].any()), bool(covered[:, -1].any())),
            'uncovered': int((~covered).sum()), 'uncovered_between': int(between.sum())}


# ---- 3 x 3 patch pairs of two non-square images (cotr_dense_cycle, cotr_dense_merge with n_pairs = 9) -----------------
NINE_SHAPES = ((300, 420), (350, 330))


def nine_pairs():
    """[((xa, ya, sa), (xb, yb, sb))] x 9: three overlapping square patches along the long axis of each image."""
    pa = [(0, 0, 300), (60, 0, 300), (120, 0, 300)]
    pb = [(0, 0, 330), (0, 10, 330), (0, 20, 330)]
    return [(i, j) for i in pa for j in pb]
