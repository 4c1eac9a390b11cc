"""Writes tests/golden/scene_overlap.npz: what the reference's own distance_between_two_caps (scripts/prepare_nn_distance_mat.py,
and through it COTR/projector/pcd_projector.py) returns for every ordered pair of two cotr_amd.utils.synth.synth_scene scenes,
and what its ReprojRatioKnnSearch.get_knn (COTR/sfm_scenes/knn_search.py) returns on those matrices for every query at
k in {1, 2, 5} with and without a db_mask.  Both are imported and called as they are; nothing of them is restated here.  The
scenes are regenerated from their seeds by the tests; the file holds seeds and recorded results only.

The script also ASSERTS that the fixture is one the tests can be strict on (with tests/scene_oracle.py): no candidate of any
pair within 1e-9 of a decision, no world point within round-off of a float32 tie, no tie among the positive overlaps of a
row, and the last-in-source-order canvas matters (a z-buffer and a first-writer canvas each change `good` in some pair).
Authoring container only (needs /root/reference)."""
import importlib.util
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from cotr_amd.utils.synth import synth_scene  # noqa: E402
from oracle import ref_import  # noqa: E402
from tests import scene_oracle as oracle  # noqa: E402

N, H, W = 6, 48, 64
SCENES = {'plain': dict(seed=25, scale=None), 'mixed': dict(seed=24, scale=(2.0, 0.5, 1.0, 1.5, 1.0, 0.5))}
KS = (1, 2, 5)
DB_MASK = np.array([0, 1, 3, 5])


def as_reference_capture(cap, projector):
    """the attributes of a reference capture that distance_between_two_caps reads; point_cloud_world as Capture.point_cloud_world
    makes it (the reference's own un-projection, cast to its DEFAULT_PRECISION)"""
    pcd = projector.img_2d_to_pcd_3d_np(cap.depth, cap.K, img=None, motion=cap.c2w).astype('float32')
    return SimpleNamespace(depth_map=cap.depth, point3d_id=np.array([0]), point_cloud_world=pcd,
                           pinhole_cam=SimpleNamespace(intrinsic_mat=cap.K, shape=cap.depth.shape),
                           cam_pose=SimpleNamespace(camera_to_world=cap.c2w, world_to_camera=np.linalg.inv(cap.c2w)))


def reference_knn(knn_search, dist, work):
    """get_knn of every query at every k, with and without the db_mask -> {key: int64 [N, k] padded with -1}"""
    scene_dir = tempfile.mkdtemp(dir=work)
    os.makedirs(os.path.join(scene_dir, 'dist_mat'))
    np.save(os.path.join(scene_dir, 'dist_mat', 'dist_mat.npy'), dist)
    captures = [SimpleNamespace(depth_path=os.path.join(scene_dir, 'depths', f'{i}.h5'), img_path=f'{i}.jpg') for i in range(N)]
    scene = SimpleNamespace(captures=captures, img_path_to_index_dict={c.img_path: i for i, c in enumerate(captures)},
                            get_captures_given_index_list=lambda ind: [int(i) for i in ind])
    search = knn_search.ReprojRatioKnnSearch(scene)
    out = {}
    for k in KS:
        for tag, mask in (('all', None), ('db', DB_MASK)):
            lists = np.full((N, k), -1, dtype=np.int64)
            for i, c in enumerate(captures):
                ind = search.get_knn(c, k, db_mask=mask)
                lists[i, :len(ind)] = ind
            out[f'knn_k{k}_{tag}'] = lists
    return out


def main():
    work = tempfile.mkdtemp()                            # the reference's global config wants ./out and ./tb_out to exist
    for d in ('out', 'tb_out'):
        os.makedirs(os.path.join(work, d))
    os.chdir(work)
    ref_import.import_reference_models()                 # installs the stubs (cv2, ...), puts the reference on sys.path
    from COTR.datasets import colmap_helper
    from COTR.projector.pcd_projector import PointCloudProjector
    from COTR.sfm_scenes import knn_search
    colmap_helper.COVISIBILITY_CHECK = colmap_helper.LOAD_PCD = True      # the script's own asserts demand it
    spec = importlib.util.spec_from_file_location('prepare_nn_distance_mat',
                                                  os.path.join(ref_import.REFERENCE_ROOT, 'scripts', 'prepare_nn_distance_mat.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)

    out = {'n': N, 'shape': (H, W), 'ks': np.array(KS), 'db_mask': DB_MASK}
    rule_matters = {'first': 0, 'minz': 0}
    for name, cfg in SCENES.items():
        caps = synth_scene(cfg['seed'], N, H, W, scale=cfg['scale'])
        ref_caps = [as_reference_capture(c, PointCloudProjector) for c in caps]
        dist = np.zeros((N, N), dtype=np.float32)        # the dtype of the reference's load_dist_mat
        for i in range(N):
            for j in range(N):
                dist[i][j] = script.distance_between_two_caps([ref_caps[i], ref_caps[j]])
        pairs = np.argwhere(np.ones((N, N), dtype=bool))
        ratio, counts, amb = oracle.overlap_pairs(caps, pairs)
        assert amb.sum() == 0, f'{name}: {amb.sum()} candidates within 1e-9 of a decision; pick another seed'
        assert sum(oracle.float32_ties(c) for c in caps) == 0, f'{name}: a world point at a float32 tie; pick another seed'
        assert np.array_equal(ratio.reshape(N, N), dist), f'{name}: the oracle does not restate the reference'
        for row in dist:
            pos = row[row > 0]
            assert np.unique(pos).size == pos.size, f'{name}: a tie among the positive overlaps of a row; pick another seed'
        for rule in rule_matters:
            other = oracle.overlap_pairs(caps, pairs, canvas_rule=rule)[1]
            rule_matters[rule] += int((other[:, 0] != counts[:, 0]).sum())
        out.update({f'{name}_seed': cfg['seed'], f'{name}_scale': np.array(cfg['scale'] or [1.0] * N), f'{name}_dist': dist})
        out.update({f'{name}_{k}': v for k, v in reference_knn(knn_search, dist, work).items()})
        print(name, '\n', dist.round(3), '\nnum_pos', oracle.num_pos(dist), 'with db_mask', oracle.num_pos(dist, DB_MASK))
    assert all(rule_matters.values()), f'the last-in-order rule does not show: {rule_matters}; pick other seeds'
    print('pairs whose `good` another canvas rule changes:', rule_matters)
    path = os.path.join(ROOT, 'tests', 'golden', 'scene_overlap.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
