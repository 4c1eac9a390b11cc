"""cotr_crop_resize_pairs against Pillow itself (8-bit BILINEAR + to_tensor + normalize) at every size class, bit for bit:
every crop size from 2 to 600 and a ladder of integer-scale neighbours up to 3296, every tile height the launcher's LDS
budget can choose (R = 8, 4, 2, 1) with small crops sharing the large tap layout, max_size as an upper bound, boxes on
every image border, launches of 1 and of 1000 tasks, and the argument checks around the largest crop the call accepts.
The cases come from tests/image_kernel_cases.py; tests/test_image_kernel_cases_cpu.py checks them without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from cotr_amd import _lib
from tests import image_kernel_cases as cases

pytestmark = pytest.mark.gpu

COTR_ERR_ARG = -1
SENTINEL = -77.25


def _dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr)).to('cuda:0')


def call(ta, tb, boxes, out, max_size):
    """One cotr_crop_resize_pairs call on device images [H,W,3] uint8 -> return code."""
    lib = _lib.load_library()
    n = len(boxes)
    bx = _dev(np.asarray(boxes, dtype=np.int32).reshape(-1, 6)) if n else torch.zeros((1, 6), dtype=torch.int32, device='cuda:0')
    rc = lib.cotr_crop_resize_pairs(ctypes.c_void_p(ta.data_ptr()), ta.shape[0], ta.shape[1], ctypes.c_void_p(tb.data_ptr()),
                                    tb.shape[0], tb.shape[1], ctypes.c_void_p(bx.data_ptr()), n, ctypes.c_void_p(out.data_ptr()),
                                    int(max_size), _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return rc


def run(ta, tb, boxes, max_size=None):
    """-> out [n,3,256,512] on the host; max_size defaults to the largest edge among the boxes."""
    boxes = np.asarray(boxes, dtype=np.int32)
    out = torch.full((len(boxes), 3, 256, 512), SENTINEL, device='cuda:0')
    rc = call(ta, tb, boxes, out, boxes[:, [2, 5]].max() if max_size is None else max_size)
    assert rc == 0, rc
    return out.cpu()


@pytest.fixture(scope='module')
def sweep_images():
    imgs = [cases.random_image(s, k) for k, s in enumerate(cases.SWEEP_SHAPES)]
    return imgs, [_dev(i) for i in imgs]


@pytest.fixture(scope='module')
def big():
    """The 7936 x 7940 image, built and uploaded once."""
    img = cases.big_image()
    return img, _dev(img)


def test_every_crop_size_from_2_to_600(sweep_images):
    (img_a, img_b), (ta, tb) = sweep_images
    for boxes in cases.every_size_launches():
        out, ref = run(ta, tb, boxes), cases.pillow_crop_reference(img_a, img_b, boxes)
        bad = [boxes[i].tolist() for i in range(len(boxes)) if not torch.equal(out[i], ref[i])]
        assert not bad, bad


def test_ladder_of_integer_scale_neighbours_up_to_3296():
    imgs = [cases.random_image(s, 10 + k) for k, s in enumerate(cases.LADDER_SHAPES)]
    boxes = cases.ladder_boxes()
    assert cases.crop_tile_rows(int(boxes[:, [2, 5]].max())) == 8
    out, ref = run(_dev(imgs[0]), _dev(imgs[1]), boxes), cases.pillow_crop_reference(imgs[0], imgs[1], boxes)
    bad = [boxes[i].tolist() for i in range(len(boxes)) if not torch.equal(out[i], ref[i])]
    assert not bad, bad


def test_every_tile_height(big):
    """Crops on both sides of every edge of the launcher's R bands, each launch with small crops that share its tap layout."""
    img, t = big
    bands = set()
    for size in cases.BAND_SIZES:
        boxes = cases.band_boxes(size)
        assert int(boxes[:, [2, 5]].max()) == size
        bands.add(cases.crop_tile_rows(size))
        out, ref = run(t, t, boxes), cases.pillow_crop_reference(img, img, boxes)
        bad = [boxes[i].tolist() for i in range(len(boxes)) if not torch.equal(out[i], ref[i])]
        assert not bad, (size, bad)
    assert bands == {8, 4, 2, 1}
    assert max(cases.BAND_SIZES) == cases.header_crop_limit()     # the largest accepted crop itself was compared above


def test_max_size_as_an_upper_bound(sweep_images):
    """max_size only sizes the LDS layout: the true maximum and a bound in each higher band give the same bits."""
    (img_a, img_b), (ta, tb) = sweep_images
    rng = np.random.default_rng(5)
    boxes = cases.place_boxes([2, 18, 255, 256, 257, 300, 600, 3], [600, 257, 256, 255, 18, 2, 301, 599], *cases.SWEEP_SHAPES, rng)
    ref = cases.pillow_crop_reference(img_a, img_b, boxes)
    bounds = [600, 601, 3296, 3297, 4865, 6529, cases.header_crop_limit()]
    assert {cases.crop_tile_rows(m) for m in bounds} == {8, 4, 2, 1}
    for max_size in bounds:
        assert torch.equal(run(ta, tb, boxes, max_size=max_size), ref), max_size


@pytest.mark.parametrize('shapes', [cases.SWEEP_SHAPES, ((263, 263), (301, 258)), ((257, 259), (258, 257))])
def test_boxes_on_every_border(shapes):
    """Corners, edges, the whole image when it is square, 2x2 crops in the last row / column; widths that are no multiple of 4."""
    imgs = [cases.random_image(s, 20 + k) for k, s in enumerate(shapes)]
    boxes = cases.border_boxes(*shapes)
    if shapes[0][0] == shapes[0][1]:
        assert [0, 0, shapes[0][0]] in boxes[:, :3].tolist()
    out, ref = run(_dev(imgs[0]), _dev(imgs[1]), boxes), cases.pillow_crop_reference(imgs[0], imgs[1], boxes)
    bad = [boxes[i].tolist() for i in range(len(boxes)) if not torch.equal(out[i], ref[i])]
    assert not bad, bad


def test_one_task_and_a_thousand_tasks_in_one_call(sweep_images):
    (img_a, img_b), (ta, tb) = sweep_images
    rng = np.random.default_rng(1000)
    sizes = rng.integers(2, 301, (2, 1000))
    sizes[:, :4] = [[256, 2, 300, 255], [2, 256, 257, 300]]
    boxes = cases.place_boxes(sizes[0], sizes[1], *cases.SWEEP_SHAPES, rng)
    assert torch.equal(run(ta, tb, boxes[:1]), cases.pillow_crop_reference(img_a, img_b, boxes[:1]))
    out = torch.full((1000, 3, 256, 512), SENTINEL, device='cuda:0')
    assert call(ta, tb, boxes, out, boxes[:, [2, 5]].max()) == 0
    for i in range(0, 1000, 100):                                   # compared in slices: the whole output is 1.5 GB
        assert torch.equal(out[i:i + 100].cpu(), cases.pillow_crop_reference(img_a, img_b, boxes[i:i + 100])), i


def test_no_task_is_no_work(sweep_images):
    _, (ta, tb) = sweep_images
    out = torch.full((2, 3, 256, 512), SENTINEL, device='cuda:0')
    for max_size in (256, 0, 100000):
        assert call(ta, tb, np.zeros((0, 6), np.int32), out, max_size) == 0
    assert bool((out == SENTINEL).all())


def test_the_limit_of_max_size(sweep_images):
    """The largest max_size include/cotr_hip.h promises is accepted and bit-exact; the next one, and 1, 0, -1, are refused on
    the host with COTR_ERR_ARG before anything is launched: `out` keeps its sentinel.  (Every box lies inside its image and is
    no larger than any max_size passed: these are argument checks, not out-of-range launches.)"""
    (img_a, img_b), (ta, tb) = sweep_images
    limit = cases.header_crop_limit()
    assert cases.crop_tile_rows(limit) == 1 and cases.crop_tile_rows(limit + 1) == 0
    boxes = cases.place_boxes([2, 2], [2, 2], *cases.SWEEP_SHAPES, np.random.default_rng(9))
    assert torch.equal(run(ta, tb, boxes, max_size=limit), cases.pillow_crop_reference(img_a, img_b, boxes))
    out = torch.full((2, 3, 256, 512), SENTINEL, device='cuda:0')
    for max_size in (limit + 1, 16384, 2 ** 31 - 1, 1, 0, -1):
        assert call(ta, tb, boxes, out, max_size) == COTR_ERR_ARG, max_size
        assert bool((out == SENTINEL).all()), max_size
    assert call(ta, tb, boxes, out, 2) == 0 and not bool((out == SENTINEL).any())      # the smallest accepted value


def test_device_cropper_raises_on_a_refused_call():
    """_DeviceCropper.__call__ turns a non-zero return code into CotrHipError (here: a stand-in library that answers
    COTR_ERR_ARG; the boxes lie inside the images and nothing is launched)."""
    from cotr_amd.inference.zoom_engine import _DeviceCropper
    img_a, img_b = cases.random_image((40, 52), 1), cases.random_image((44, 38), 2)
    cropper = _DeviceCropper(img_a, img_b, torch.device('cuda:0'))
    boxes = np.array([[3, 4, 20, 5, 6, 30]], dtype=np.int32)
    out = torch.full((1, 3, 256, 512), SENTINEL, device='cuda:0')
    assert torch.equal(cropper(boxes, out).cpu(), cases.pillow_crop_reference(img_a, img_b, boxes))    # the real library first
    seen = []

    class Refusing:
        def cotr_crop_resize_pairs(self, *args):
            seen.append(args)
            return COTR_ERR_ARG

    cropper.lib = Refusing()
    out.fill_(SENTINEL)
    with pytest.raises(_lib.CotrHipError, match='cotr_crop_resize_pairs failed'):
        cropper(boxes, out)
    assert len(seen) == 1 and seen[0][7] == 1 and seen[0][9] == 30          # n and max_size as handed to the library
    assert bool((out == SENTINEL).all())
