"""Writes tests/golden/dataset_corrs.npz: what the reference's own COTRZoomDataset.get_corrs (COTR/datasets/cotr_dataset.py,
and through it COTR/projector/pcd_projector.py) returns on a cotr_amd.utils.synth.synth_captures scene - every pixel of the
query view projected into the nn view, and a subset with repeats in both directions.  The method is imported and called
as it is; nothing of it is restated here.  The scene is regenerated from its seed by the test; the file holds the recorded
results only.  Authoring container only (needs /root/reference)."""
import os
import sys
import tempfile
from types import SimpleNamespace
from unittest import mock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from cotr_amd.utils.synth import synth_captures  # noqa: E402
from oracle import ref_import  # noqa: E402

SEED, H, W = 5, 64, 96
SUBSET_SEED, SUBSET_LEN = 11, 300


def as_reference_capture(cap):
    """the attributes of a reference capture that get_corrs reads"""
    return SimpleNamespace(depth_map=cap.depth, image=cap.image, pinhole_cam=SimpleNamespace(intrinsic_mat=cap.K),
                           cam_pose=SimpleNamespace(camera_to_world=cap.c2w, world_to_camera=np.linalg.inv(cap.c2w)))


def main():
    work = tempfile.mkdtemp()                            # the reference's global config wants ./out and ./tb_out to exist
    for d in ('out', 'tb_out'):
        os.makedirs(os.path.join(work, d))
    os.chdir(work)
    ref_import.import_reference_models()                 # installs the stubs (cv2, ...), puts the reference on sys.path
    from COTR.datasets.cotr_dataset import COTRZoomDataset
    query, nn = synth_captures(SEED, H, W)
    out = {'seed': SEED, 'shape': (H, W), 'q2n': COTRZoomDataset.get_corrs(None, as_reference_capture(query), as_reference_capture(nn))}
    for name, a, b in (('q2n', query, nn), ('n2q', nn, query)):
        pick = np.random.default_rng(SUBSET_SEED).integers(0, int((a.depth > 0).sum()), SUBSET_LEN)   # valid pixels, with repeats
        with mock.patch('numpy.random.choice', lambda n, size, replace: pick):
            out[name + '_subset'] = COTRZoomDataset.get_corrs(None, as_reference_capture(a), as_reference_capture(b), reduced_size=SUBSET_LEN)
        out[name + '_pick'] = pick
    print({k: np.shape(v) for k, v in out.items()})
    path = os.path.join(ROOT, 'tests', 'golden', 'dataset_corrs.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
