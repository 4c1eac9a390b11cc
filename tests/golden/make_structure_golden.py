"""Writes tests/golden/structure_demo.npz: two posed cameras, 96 correspondences on a quarter-pixel grid (float32 holds them
exactly) and, for each camera, what the reference's own PointCloudProjector.pcd_2d_to_pcd_3d_np returns for those pixels at
depth 2 through the camera-to-world matrix - the ray points demo_reconstruction.py builds before it subtracts the camera
centre.  The projector is imported and called as it is; nothing of it is restated here.  The file holds the inputs and the
recorded ray points only; the tests take the point on ray A nearest ray B from them with tests/structure_oracle.py.
Authoring container only (needs /root/reference)."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests import structure_oracle as so  # noqa: E402

N = 96


def main():
    work = tempfile.mkdtemp()                            # the reference's global config wants ./out and ./tb_out to exist
    for d in ('out', 'tb_out'):
        os.makedirs(os.path.join(work, d))
    os.chdir(work)
    ref_import.import_reference_models()                 # installs the stubs (cv2, ...), puts the reference on sys.path
    from COTR.projector.pcd_projector import PointCloudProjector

    rng = np.random.default_rng(11)
    K_a = np.array([[520.0, 0.0, 322.5], [0.0, 515.0, 238.0], [0.0, 0.0, 1.0]])
    K_b = np.array([[480.0, 0.0, 310.0], [0.0, 490.0, 245.5], [0.0, 0.0, 1.0]])
    c2w_a = np.eye(4)
    c2w_a[:3, :3], c2w_a[:3, 3] = so.rotation([0.02, -0.03, 0.01]), [0.3, -0.2, 0.1]
    c2w_b = np.eye(4)
    c2w_b[:3, :3], c2w_b[:3, 3] = so.rotation([-0.04, 0.12, 0.03]), [1.4, -0.1, 0.25]
    X = np.stack([rng.uniform(-1.5, 2.5, N), rng.uniform(-1.5, 1.5, N), rng.uniform(4, 9, N)], axis=1)
    cams = np.array([[K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]] for K in (K_a, K_b)])
    poses = np.stack([so.pose_of_c2w(c2w_a), so.pose_of_c2w(c2w_b)])
    pts, z = so.observe(X, cams, poses)
    assert (z > 0).all()
    pts = np.round((pts + rng.normal(size=pts.shape) * 0.5) * 4) / 4
    assert np.array_equal(pts, so.f32(pts))
    two = np.ones((N, 1)) * 2
    rays_a = PointCloudProjector.pcd_2d_to_pcd_3d_np(pts[0], two, K_a, motion=c2w_a)
    rays_b = PointCloudProjector.pcd_2d_to_pcd_3d_np(pts[1], two, K_b, motion=c2w_b)
    assert rays_a.shape == rays_b.shape == (N, 3)
    path = os.path.join(ROOT, 'tests', 'golden', 'structure_demo.npz')
    np.savez_compressed(path, points_a=pts[0], points_b=pts[1], K_a=K_a, K_b=K_b, c2w_a=c2w_a, c2w_b=c2w_b, rays_a=rays_a, rays_b=rays_b)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
