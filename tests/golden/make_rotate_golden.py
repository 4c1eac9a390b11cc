"""Writes tests/golden/rotate_pose.npz: what the reference's own rotate_camera_pose (COTR/cameras/camera_pose.py) returns for
a dozen poses and angles.  The function is imported and called as it is; nothing of it is restated here.  Stored per case: the
angle, the ``camera_to_world`` of the pose handed in (as the reference's CameraPose reports it, so the float32 storage of the
INPUT is already in it) and the ``camera_to_world`` of the pose that comes back.  What is left between that and
cotr_amd.data.rotated_c2w is the float32 quaternion + translation storage of the RESULT.  Authoring container only (needs
/root/reference)."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402

ANGLES = [0.0, 17.0, -17.0, 45.0, 90.0, 180.0, -123.4, 17.0, -17.0, 45.0, 90.0, 180.0, -123.4]
SEED = 3


def random_c2w(rng):
    """a proper rotation (QR of a normal matrix, determinant +1) and a camera centre a few units from the origin"""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    m = np.eye(4)
    m[:3, :3] = q
    m[:3, 3] = rng.uniform(-8, 8, 3)
    return m


def main():
    work = tempfile.mkdtemp()                            # the reference's global config wants ./out and ./tb_out to exist
    for d in ('out', 'tb_out'):
        os.makedirs(os.path.join(work, d))
    os.chdir(work)
    ref_import.import_reference_models()                 # installs the stubs (cv2, ...), puts the reference on sys.path
    from COTR.cameras.camera_pose import CameraPose, rotate_camera_pose
    rng = np.random.default_rng(SEED)
    c2w_in, c2w_out = [], []
    for angle in ANGLES:
        pose = CameraPose.from_camera_to_world(random_c2w(rng))
        c2w_in.append(np.array(pose.camera_to_world, dtype=np.float64))
        c2w_out.append(np.array(rotate_camera_pose(pose, angle).camera_to_world, dtype=np.float64))
    out = {'angles': np.array(ANGLES), 'c2w_in': np.stack(c2w_in), 'c2w_out': np.stack(c2w_out)}
    print({k: v.shape for k, v in out.items()})
    path = os.path.join(ROOT, 'tests', 'golden', 'rotate_pose.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
