"""The calls behind tests/golden/wrapper_errors.json: every public function of the geometry wrappers (guided, homography,
essential, pnp, structure, bundle, rigid3d, icp, triangulate, warp under cotr_amd/inference/) with one wrong argument at a
time, its CPU-tensor refusal, two doubly-wrong calls that pin the order of its checks, and the non-integer counts it accepts;
and the chained calls whose sequence of library calls the same file pins.  tests/golden/make_wrapper_errors.py records
what they raise and call, tests/test_wrapper_errors_cpu.py replays them.  Nothing here touches a device or the built library:
whoever runs the cases first replaces the wrappers' device rule by ``reached_device`` (a call that gets that far passed every
check) or, for the call logs, by the CPU with ``Recorder`` in the library's place."""
import contextlib
import ctypes
import importlib
import types

import numpy as np
import torch


class DeviceReached(Exception):
    """raised in place of picking a device: every check before it passed"""


def reached_device(device=None):
    raise DeviceReached()


def reached_library():
    raise AssertionError('load_library() reached before the device was picked')


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def function(path):
    module, name = path.split('.')
    return getattr(importlib.import_module('cotr_amd.inference.' + module), name)


def outcome(path, base, over):
    """-> [exception type, message] of one call; a callable override is built only now (the large ones)"""
    kw = dict(base, **over)
    kw = {k: v() if callable(v) else v for k, v in kw.items()}
    try:
        function(path)(**kw)
    except DeviceReached:
        return ['DeviceReached', '']
    except Exception as e:   # noqa: BLE001
        return [type(e).__name__, str(e)]
    return ['returned', '']


# ---- arguments that pass ------------------------------------------------------------------------------------------------
def _pts(n, d=2, seed=0):
    return np.random.default_rng(seed).uniform(1, 60, (n, d))


K = np.array([[500.0, 0, 32], [0, 500, 24], [0, 0, 1]])
K_NAN = np.array([[500.0, 0, np.nan], [0, 500, 24], [0, 0, 1]])
K_F0 = np.array([[0.0, 0, 32], [0, 500, 24], [0, 0, 1]])
K_SUM0 = np.array([[1.0, 0, 32], [0, -1, 24], [0, 0, 1]])
DEPTH = np.full((48, 64), 2.0, np.float32)
C2W = np.eye(4)
C2W_NAN = np.where(np.eye(4) > 0, np.nan, 0.0)
IMG = np.zeros((48, 64, 3), np.uint8)
CAP = types.SimpleNamespace(depth=DEPTH, K=K, c2w=C2W)
VIEWS = np.stack([_pts(6, 2, 1), _pts(6, 2, 2), _pts(6, 2, 3)])
POSES = np.tile(np.eye(3, 4), (3, 1, 1))
QUAD = np.array([[0.0, 0], [10, 0], [0, 10], [10, 10]])


def big(*shape):
    return lambda: np.zeros(shape)   # untouched pages: only its shape is read


PAIRS = dict(points1=_pts(20), points2=_pts(20, 2, 1))
RANSAC = [('max_iters_0', dict(max_iters=0)), ('threshold_0', dict(threshold=0)), ('threshold_inf', dict(threshold=np.inf)),
          ('threshold_nan', dict(threshold=np.nan)), ('confidence_0', dict(confidence=0)), ('confidence_1', dict(confidence=1))]


def pair_cases(a, b, few):
    return [(f'{a}_shape', {a: _pts(20, 3)}), (f'{b}_shape', {b: _pts(20, 3)}), (f'{a}_1d', {a: np.zeros(4)}),
            ('length', {b: _pts(19)}), ('too_few', {a: _pts(few), b: _pts(few)}),
            ('too_many', {a: big((1 << 24) + 1, 2), b: big((1 << 24) + 1, 2)})]


def camera_cases(name):
    return [(f'{name}_shape', {name: np.eye(4)}), (f'{name}_nan', {name: K_NAN}), (f'{name}_focal_0', {name: K_F0})]


def depth_cases(name):
    return [(f'{name}_float64', {name: DEPTH.astype(np.float64)}), (f'{name}_1d', {name: np.zeros(5, np.float32)}),
            (f'{name}_empty', {name: np.zeros((0, 5), np.float32)}),
            (f'{name}_too_large', {name: lambda: np.broadcast_to(np.float32(1), (1 << 15, (1 << 13) + 1))})]


def pose_cases(name):
    return [(f'{name}_shape', {name: np.eye(3)}), (f'{name}_nan', {name: C2W_NAN})]


TABLE = {}

# ---- guided.py ------------------------------------------------------------------------------------------------------------
_nm = dict(pred_ab=_pts(5), kp_b=_pts(6), pred_ba=_pts(6), kp_a=_pts(5))
TABLE['guided.nearest_mutual'] = (_nm, [(f'{k}_shape', {k: _pts(5, 3)}) for k in _nm] + [
    ('pred_ab_rows', dict(pred_ab=_pts(4))), ('pred_ba_rows', dict(pred_ba=_pts(5))),
    ('no_keypoints', dict(kp_a=_pts(0), pred_ab=_pts(0))),
    ('order_pred_ab_before_kp_a', dict(pred_ab=_pts(5, 3), kp_a=_pts(5, 3))),
    ('order_rows_before_empty', dict(kp_b=_pts(0), pred_ba=_pts(0), pred_ab=_pts(4))),
    ('cpu_tensor_accepted', dict(pred_ab=T(_pts(5)))), ('passes', {})])
_mm = dict(corrs_a_b=_pts(5, 4), corrs_b_a=_pts(6, 4), kp_a=_pts(5), kp_b=_pts(6))
TABLE['guided.mutual_matches'] = (_mm, [('corrs_a_b_shape', dict(corrs_a_b=_pts(5, 3))), ('corrs_b_a_shape', dict(corrs_b_a=_pts(6))),
                                        ('order_a_b_before_b_a', dict(corrs_a_b=_pts(5, 3), corrs_b_a=_pts(6))),
                                        ('order_corrs_before_keypoints', dict(corrs_b_a=_pts(6), kp_a=_pts(5, 3)))])
TABLE['guided.ransac_fundamental'] = (PAIRS, pair_cases('points1', 'points2', 14) + RANSAC + [
    ('max_iters_over', dict(max_iters=65537)), ('order_points_before_max_iters', dict(points1=_pts(20, 3), max_iters=0)),
    ('order_max_iters_before_threshold', dict(max_iters=0, threshold=0)), ('max_iters_not_integer_accepted', dict(max_iters=10.5)),
    ('cpu_tensor_accepted', dict(points1=T(_pts(20)))), ('passes', {})])
TABLE['guided.find_fundamental_mat'] = (PAIRS, [('too_few', dict(points1=_pts(14), points2=_pts(14))),
                                                ('threshold_0', dict(ransac_reproj_threshold=0)),
                                                ('order_points_before_confidence', dict(points2=_pts(20, 3), confidence=2)),
                                                ('order_max_iters_before_confidence', dict(max_iters=0, confidence=2))])
TABLE['guided.filter_guided_matches'] = (_mm, [('corrs_a_b_shape', dict(corrs_a_b=_pts(5, 3)))])

# ---- homography.py --------------------------------------------------------------------------------------------------------
TABLE['homography.ransac_homography'] = (PAIRS, pair_cases('points1', 'points2', 3) + RANSAC + [
    ('max_iters_over', dict(max_iters=65537)), ('refine_iters_under', dict(refine_iters=-1)), ('refine_iters_over', dict(refine_iters=65)),
    ('order_too_few_before_refine_iters', dict(points1=_pts(3), points2=_pts(3), refine_iters=-1)),
    ('order_threshold_before_refine_iters', dict(threshold=0, refine_iters=65)),
    ('refine_iters_not_integer_accepted', dict(refine_iters=2.5)), ('max_iters_not_integer_accepted', dict(max_iters=10.5)),
    ('cpu_tensor_accepted', dict(points2=T(_pts(20)))), ('passes', {})])
_fh = dict(src=_pts(20), dst=_pts(20, 2, 1))
TABLE['homography.find_homography'] = (_fh, [('src_shape', dict(src=_pts(20, 3))), ('max_iters_0', dict(max_iters=0)),
                                             ('order_length_before_threshold', dict(dst=_pts(19), ransac_reproj_threshold=0)),
                                             ('order_max_iters_before_confidence', dict(max_iters=0, confidence=0))])
_ph = dict(picture=IMG, pts_picture=_pts(6), pts_b=_pts(6, 2, 1), img_b=IMG)
TABLE['homography.paste_by_homography'] = (_ph, [
    ('picture_float', dict(picture=IMG.astype(np.float32))), ('img_b_channels', dict(img_b=np.zeros((8, 8, 2), np.uint8))),
    ('points_shapes', dict(pts_b=_pts(5))), ('too_few', dict(pts_picture=_pts(3), pts_b=_pts(3))),
    ('four_points_check_keywords', dict(pts_picture=QUAD, pts_b=QUAD, max_iters=0)),
    ('order_picture_before_points', dict(picture=IMG.astype(np.float32), pts_b=_pts(5))),
    ('order_shapes_before_too_few', dict(pts_picture=_pts(3), pts_b=_pts(2)))])

# ---- essential.py ---------------------------------------------------------------------------------------------------------
_e = dict(PAIRS, K1=K)
_ek = camera_cases('K1') + camera_cases('K2')
TABLE['essential.ransac_essential'] = (_e, pair_cases('points1', 'points2', 4) + _ek + RANSAC + [
    ('max_iters_over', dict(max_iters=6554)), ('focal_sum_0', dict(K1=K_SUM0)), ('threshold_over_focal_0', dict(threshold=1e-170)),
    ('order_points_before_K1', dict(points1=_pts(20, 3), K1=np.eye(4))), ('order_K1_before_max_iters', dict(K1=K_NAN, max_iters=0)),
    ('max_iters_not_integer_accepted', dict(max_iters=10.5)), ('cpu_tensor_accepted', dict(points1=T(_pts(20)))), ('passes', {})])
_fe = dict(PAIRS, camera_matrix1=K)
TABLE['essential.find_essential_mat'] = (_fe, [('too_few', dict(points1=_pts(4), points2=_pts(4))), ('prob_1', dict(prob=1)),
                                               ('order_K_before_prob', dict(camera_matrix1=K_F0, prob=1)),
                                               ('order_max_iters_before_threshold', dict(max_iters=0, threshold=-1))])
_pe = dict(_e, E=np.eye(3))
_mask_cases = [('mask_length', dict(mask=np.ones(19)))]
TABLE['essential.pose_of_essential'] = (_pe, pair_cases('points1', 'points2', 4) + _ek + _mask_cases + [
    ('distance_0', dict(distance_thresh=0)), ('distance_inf', dict(distance_thresh=np.inf)), ('E_size', dict(E=np.eye(4))),
    ('order_distance_before_E', dict(distance_thresh=0, E=np.eye(4))), ('order_E_before_mask', dict(E=np.eye(2), mask=np.ones(3))),
    ('cpu_tensor_accepted', dict(E=T(np.eye(3)), mask=T(np.ones(20)))), ('passes', {})])
_rp = dict(_fe, E=np.eye(3))
TABLE['essential.recover_pose'] = (_rp, [('E_size', dict(E=np.eye(4))), ('mask_length', dict(mask=np.ones(19))),
                                         ('order_K_before_distance', dict(camera_matrix2=np.eye(2), distance_thresh=0)),
                                         ('order_points_before_E', dict(points1=_pts(20, 3), E=np.eye(4)))])
_rt = dict(_e, R=np.eye(3), t=np.array([1.0, 0, 0]))
_rt_cases = [('threshold_0', dict(threshold=0)), ('threshold_nan', dict(threshold=np.nan)), ('focal_sum_0', dict(K1=K_SUM0)),
             ('distance_0', dict(distance_thresh=0)), ('rounds_0', dict(rounds=0)), ('rounds_over', dict(rounds=9)),
             ('refine_iters_under', dict(refine_iters=-1)), ('refine_iters_over', dict(refine_iters=65)), ('R_size', dict(R=np.eye(4))),
             ('t_size', dict(t=np.zeros(4)))]
TABLE['essential.refine_pose_tensors'] = (_rt, pair_cases('points1', 'points2', 4) + _ek + _rt_cases + _mask_cases + [
    ('cpu_tensor_R', dict(R=T(np.eye(3)))), ('cpu_tensor_found', dict(found=torch.ones(1, dtype=torch.int32))),
    ('order_threshold_before_rounds', dict(threshold=0, rounds=0)), ('order_R_before_cpu_tensor', dict(R=np.eye(4), points1=T(_pts(20)))),
    ('order_rounds_before_refine_iters', dict(rounds=9, refine_iters=65)),
    ('rounds_not_integer_accepted', dict(rounds=1.5)), ('refine_iters_not_integer_accepted', dict(refine_iters=2.5)), ('passes', {})])
TABLE['essential.refine_relative_pose'] = (_rt, [('R_size', dict(R=np.eye(4))), ('rounds_over', dict(rounds=9)),
                                                 ('cpu_tensor_t', dict(t=torch.ones(3, dtype=torch.float64))),
                                                 ('order_distance_before_t', dict(distance_thresh=-1, t=np.zeros(2))),
                                                 ('order_mask_before_cpu_tensor', dict(mask=np.ones(3), points2=T(_pts(20))))])
TABLE['essential.relative_pose_tensors'] = (_e, pair_cases('points1', 'points2', 4) + _ek + RANSAC + [
    ('max_iters_over', dict(max_iters=6554)), ('focal_sum_0', dict(K1=K_SUM0)), ('distance_0', dict(distance_thresh=0)),
    ('refine_rounds_over', dict(refine_rounds=9)), ('refine_rounds_under', dict(refine_rounds=-1)),
    ('refine_iters_over', dict(refine_rounds=4, refine_iters=65)), ('refine_iters_unread_without_rounds', dict(refine_iters=65)),
    ('order_max_iters_before_distance', dict(max_iters=0, distance_thresh=0)),
    ('order_distance_before_refine_rounds', dict(distance_thresh=0, refine_rounds=9)),
    ('refine_rounds_not_integer_accepted', dict(refine_rounds=1.5)),
    ('refine_iters_not_integer_accepted', dict(refine_rounds=4, refine_iters=2.5)),
    ('max_iters_not_integer_accepted', dict(max_iters=10.5)), ('cpu_tensor_accepted', dict(points2=T(_pts(20)))), ('passes', {})])
TABLE['essential.relative_pose'] = (_e, [('too_few', dict(points1=_pts(4), points2=_pts(4))), ('refine_rounds_over', dict(refine_rounds=9)),
                                         ('order_K2_before_confidence', dict(K2=K_NAN, confidence=0)),
                                         ('order_threshold_before_distance', dict(threshold=0, distance_thresh=0))])

# ---- pnp.py ---------------------------------------------------------------------------------------------------------------
_lp = dict(points=_pts(10), depth=DEPTH, K=K)
TABLE['pnp.lift_pixels'] = (_lp, depth_cases('depth') + camera_cases('K') + pose_cases('c2w') + [
    ('points_shape', dict(points=_pts(10, 3))), ('points_cv2_shape_accepted', dict(points=_pts(10).reshape(10, 1, 2))),
    ('points_none', dict(points=_pts(0))), ('points_too_many', dict(points=big((1 << 24) + 1, 2))),
    ('cpu_tensor_points', dict(points=T(_pts(10)))), ('cpu_tensor_depth', dict(depth=T(DEPTH))),
    ('order_points_before_depth', dict(points=_pts(10, 3), depth=DEPTH.astype(np.float64))),
    ('order_depth_before_K', dict(depth=np.zeros(5, np.float32), K=K_NAN)),
    ('order_c2w_before_cpu_tensor', dict(c2w=np.eye(3), points=T(_pts(10)))), ('passes', {})])
_pnp = dict(object_points=_pts(12, 3), image_points=_pts(12), K=K)
_sq = [('squared_threshold_0', dict(threshold=1e-30)), ('squared_threshold_inf', dict(threshold=1e30))]
_ri = [('refine_iters_under', dict(refine_iters=-1)), ('refine_iters_over', dict(refine_iters=65)),
       ('refine_iters_not_integer', dict(refine_iters=2.5))]
TABLE['pnp.ransac_pnp'] = (_pnp, camera_cases('K') + RANSAC + _sq + _ri + [
    ('image_points_shape', dict(image_points=_pts(12, 3))), ('object_points_shape', dict(object_points=_pts(12))),
    ('cv2_shapes_accepted', dict(object_points=_pts(12, 3).reshape(12, 1, 3), image_points=_pts(12).reshape(12, 1, 2))),
    ('length', dict(object_points=_pts(11, 3))), ('too_few', dict(object_points=_pts(3, 3), image_points=_pts(3))),
    ('too_many', dict(object_points=big((1 << 24) + 1, 3), image_points=big((1 << 24) + 1, 2))), ('max_iters_over', dict(max_iters=65537)),
    ('cpu_tensor_object_points', dict(object_points=T(_pts(12, 3)))), ('cpu_tensor_image_points', dict(image_points=T(_pts(12)))),
    ('order_image_before_object', dict(image_points=_pts(12, 3), object_points=_pts(12))),
    ('order_squared_threshold_before_refine_iters', dict(threshold=1e-30, refine_iters=65)),
    ('order_length_before_too_few', dict(object_points=_pts(2, 3), image_points=_pts(3))),
    ('max_iters_not_integer_accepted', dict(max_iters=10.5)), ('passes', {})])
_sp = dict(object_points=_pts(12, 3), image_points=_pts(12), camera_matrix=K)
TABLE['pnp.solve_pnp_ransac'] = (_sp, [('dist_coeffs', dict(dist_coeffs=np.array([0.1, 0, 0, 0]))), ('dist_coeffs_zero_accepted', dict(dist_coeffs=np.zeros(5))),
                                       ('iterations_count_0', dict(iterations_count=0)), ('reprojection_error_0', dict(reprojection_error=0)),
                                       ('order_dist_coeffs_before_points', dict(dist_coeffs=np.ones(4), image_points=_pts(12, 3))),
                                       ('order_K_before_confidence', dict(camera_matrix=K_F0, confidence=1))])
TABLE['pnp.rodrigues'] = (dict(x=np.zeros(3)), [('shape', dict(x=np.zeros((2, 2))))])
_lt = dict(points_a=_pts(12), points_b=_pts(12, 2, 1), depth_a=DEPTH, K_a=K, c2w_a=C2W, K_b=K)
TABLE['pnp.localize_tensors'] = (_lt, pair_cases('points_a', 'points_b', 3) + depth_cases('depth_a') + camera_cases('K_a') + camera_cases('K_b')
                                 + pose_cases('c2w_a') + RANSAC + _sq + _ri + [
    ('cv2_shapes_accepted', dict(points_a=_pts(12).reshape(12, 1, 2), points_b=_pts(12).reshape(12, 1, 2))), ('no_pose_accepted', dict(c2w_a=None)),
    ('cpu_tensor_points_b', dict(points_b=T(_pts(12)))), ('cpu_tensor_depth_a', dict(depth_a=T(DEPTH))),
    ('order_too_few_before_depth', dict(points_a=_pts(3), points_b=_pts(3), depth_a=DEPTH.astype(np.float64))),
    ('order_K_b_before_c2w', dict(K_b=K_NAN, c2w_a=np.eye(3))), ('order_c2w_before_max_iters', dict(c2w_a=C2W_NAN, max_iters=0)),
    ('max_iters_not_integer_accepted', dict(max_iters=10.5)), ('passes', {})])
_lo = dict(points_a=_pts(12), points_b=_pts(12, 2, 1), cap_a=CAP, K_b=K)
TABLE['pnp.localize'] = (_lo, [('length', dict(points_b=_pts(11))), ('refine_iters_over', dict(refine_iters=65)),
                               ('cpu_tensor_points_a', dict(points_a=T(_pts(12)))),
                               ('order_points_before_K_b', dict(points_a=_pts(12, 3), K_b=np.eye(2))),
                               ('order_threshold_before_cpu_tensor', dict(threshold=0, points_a=T(_pts(12))))])

# ---- structure.py ---------------------------------------------------------------------------------------------------------
_tv = dict(points=VIEWS, cameras=K, poses=POSES)
_view_cases = [('points_shape', dict(points=_pts(6))), ('one_view', dict(points=VIEWS[:1])), ('too_many_views', dict(points=np.zeros((33, 2, 2)))),
               ('no_points', dict(points=np.zeros((3, 0, 2)))), ('cameras_nan', dict(cameras=K_NAN)), ('cameras_focal_0', dict(cameras=K_F0)),
               ('cameras_shape', dict(cameras=np.ones((3, 4)))), ('cameras_rows_focal_0', dict(cameras=np.zeros((3, 5)))),
               ('poses_shape', dict(poses=POSES[:2])), ('poses_2d', dict(poses=np.zeros((3, 11)))), ('visible_shape', dict(visible=np.ones((3, 5))))]
_tv_checks = [('threshold_0', dict(threshold=0)), ('threshold_inf', dict(threshold=np.inf)), ('squared_threshold_0', dict(threshold=1e-30)),
              ('squared_threshold_inf', dict(threshold=1e30)), ('min_angle_under', dict(min_angle=-1)), ('min_angle_over', dict(min_angle=181)),
              ('distance_0', dict(distance_thresh=0))] + _ri + [
              ('rule', dict(rule='nearest')), ('demo_three_views', dict(rule='demo', robust=False, refine_iters=0)),
              ('order_threshold_before_min_angle', dict(threshold=0, min_angle=-1)),
              ('order_refine_iters_before_rule', dict(refine_iters=65, rule='nearest'))]
TABLE['structure.triangulate_views'] = (_tv, _view_cases + _tv_checks + [
    ('too_many_points', dict(points=big(2, (1 << 24) + 1, 2))),
    ('demo_robust', dict(points=VIEWS[:2], poses=POSES[:2], rule='demo', refine_iters=0)),
    ('demo_refine', dict(points=VIEWS[:2], poses=POSES[:2], rule='demo', robust=False)),
    ('cpu_tensor_points', dict(points=T(VIEWS))), ('cpu_tensor_visible', dict(visible=torch.ones((3, 6), dtype=torch.bool))),
    ('cpu_tensor_found', dict(found=torch.ones(1, dtype=torch.int32))),
    ('order_points_before_cameras', dict(points=_pts(6), cameras=K_NAN)), ('order_poses_before_visible', dict(poses=POSES[:2], visible=np.ones(3))),
    ('order_rule_before_cpu_tensor', dict(rule='nearest', poses=T(POSES))), ('passes', {})])
_tp = dict(PAIRS, K1=K, R=np.eye(3), t=np.array([1.0, 0, 0]))
_no_rt = dict(R=None, t=None)
TABLE['structure.triangulate_points_tensors'] = (_tp, pair_cases('points1', 'points2', 0)[:4] + _ek + _tv_checks + [
    ('none', dict(points1=_pts(0), points2=_pts(0))), ('no_pose', _no_rt), ('both_poses', dict(c2w1=C2W, c2w2=C2W)), ('R_without_t', dict(t=None)),
    ('one_c2w', dict(_no_rt, c2w1=C2W)), ('R_size', dict(R=np.eye(4))), ('t_size', dict(t=np.zeros(2))), ('cpu_tensor_R', dict(R=T(np.eye(3)))),
    ('c2w1_shape', dict(_no_rt, c2w1=np.eye(3), c2w2=C2W)), ('c2w2_nan', dict(_no_rt, c2w1=C2W, c2w2=C2W_NAN)),
    ('c2w_accepted', dict(_no_rt, c2w1=C2W, c2w2=C2W)), ('cpu_tensor_points1', dict(points1=T(_pts(20)))),
    ('cpu_tensor_visible', dict(visible=torch.ones((2, 20), dtype=torch.bool))),
    ('order_K1_before_poses', dict(K1=K_NAN, t=None)), ('order_R_before_threshold', dict(R=np.eye(4), threshold=0)),
    ('order_t_before_cpu_tensor', dict(R=T(np.eye(3)), t=np.zeros(2))), ('passes', {})])
TABLE['structure.triangulate_points'] = (_tp, [('no_pose', _no_rt), ('rule', dict(rule='nearest')),
                                               ('order_points_before_K2', dict(points2=_pts(19), K2=K_F0)),
                                               ('order_distance_before_cpu_tensor', dict(distance_thresh=0, points2=T(_pts(20))))])
_c4 = np.concatenate([_pts(6), _pts(6, 2, 1)], axis=1)
TABLE['structure.stack_views'] = (dict(corrs_list=[_c4, _c4]), [
    ('empty', dict(corrs_list=[])), ('shape', dict(corrs_list=[_c4, _c4[:, :3]])), ('lengths', dict(corrs_list=[_c4, _c4[:5]])),
    ('queries_differ', dict(corrs_list=[_c4, _c4[::-1]])), ('order_shape_before_queries', dict(corrs_list=[_c4, _c4[::-1], _c4[:2]])),
    ('passes', {})])
_rc = dict(corrs=np.concatenate([_pts(20), _pts(20, 2, 1)], axis=1), img_a=IMG, img_b=IMG, K_a=K, K_b=K)
TABLE['structure.reconstruct_tensors'] = (_rc, [
    ('corrs_shape', dict(corrs=_pts(20))), ('one_pose', dict(c2w_a=C2W)), ('img_a_shape', dict(img_a=IMG[..., 0])),
    ('img_b_channels', dict(img_b=IMG[..., :2])), ('bundle_rounds_under', dict(bundle_rounds=-1)),
    ('bundle_rounds_not_integer', dict(bundle_rounds=1.5)), ('order_corrs_before_poses', dict(corrs=_pts(20), c2w_b=C2W)),
    ('order_img_a_before_img_b', dict(img_a=IMG[..., 0], img_b=IMG[..., :2])),
    ('order_img_b_before_bundle_rounds', dict(img_b=IMG[..., 0], bundle_rounds=-1)), ('passes', {})])

# ---- bundle.py ------------------------------------------------------------------------------------------------------------
_ba = dict(_tv, X=_pts(6, 3))
_ba_cases = _view_cases + [
    ('too_many_points', dict(points=big(3, (1 << 20) + 1, 2))), ('X_shape', dict(X=_pts(5, 3))), ('fixed_mask_shape', dict(fixed_views=np.array([True, False]))),
    ('fixed_index', dict(fixed_views=(3,))), ('fixed_negative', dict(fixed_views=(-1,))), ('none_fixed', dict(fixed_views=())),
    ('all_fixed', dict(fixed_views=(0, 1, 2))), ('fixed_mask_accepted', dict(fixed_views=np.array([True, False, False]))),
    ('threshold_0', dict(threshold=0)), ('squared_threshold_0', dict(threshold=1e-30)), ('squared_threshold_inf', dict(threshold=1e30)),
    ('distance_0', dict(distance_thresh=0)), ('distance_nan', dict(distance_thresh=np.nan)), ('rounds_0', dict(rounds=0)), ('rounds_over', dict(rounds=9)),
    ('rounds_not_integer', dict(rounds=1.5)), ('iters_under', dict(iters=-1)), ('iters_over', dict(iters=65)), ('iters_not_integer', dict(iters=2.5)),
    ('lambda0_under', dict(lambda0=0)), ('lambda0_over', dict(lambda0=1e13))]
TABLE['bundle.bundle_adjust_tensors'] = (_ba, _ba_cases + [
    ('cpu_tensor_X', dict(X=T(_pts(6, 3)))), ('cpu_tensor_cameras', dict(cameras=T(K))),
    ('order_X_before_visible', dict(X=_pts(5, 3), visible=np.ones(2))), ('order_fixed_before_threshold', dict(fixed_views=(), threshold=0)),
    ('order_rounds_before_iters', dict(rounds=0, iters=65)), ('order_lambda0_before_cpu_tensor', dict(lambda0=0, points=T(VIEWS))), ('passes', {})])
TABLE['bundle.bundle_adjust'] = (_ba, [('X_shape', dict(X=_pts(6))), ('iters_over', dict(iters=65)),
                                       ('order_points_before_X', dict(points=VIEWS[:1], X=_pts(5, 3))),
                                       ('order_distance_before_lambda0', dict(distance_thresh=0, lambda0=0))])

# ---- rigid3d.py -----------------------------------------------------------------------------------------------------------
_r3 = dict(src=_pts(10, 3), dst=_pts(10, 3, 1), threshold=0.05)
_r3_checks = RANSAC + _sq + [('max_iters_over', dict(max_iters=65537)), ('with_scale_2', dict(with_scale=2)), ('with_scale_word', dict(with_scale='yes')),
                             ('rounds_under', dict(rounds=-1)), ('rounds_over', dict(rounds=9)), ('rounds_not_integer', dict(rounds=1.5))]
TABLE['rigid3d.ransac_rigid3d'] = (_r3, _r3_checks + [
    ('src_shape', dict(src=_pts(10))), ('dst_shape', dict(dst=_pts(10, 4))), ('src_cv2_shape_refused', dict(src=_pts(10, 3).reshape(10, 1, 3))),
    ('length', dict(dst=_pts(9, 3))), ('too_few', dict(src=_pts(2, 3), dst=_pts(2, 3))),
    ('too_many', dict(src=big((1 << 24) + 1, 3), dst=big((1 << 24) + 1, 3))), ('cpu_tensor_src', dict(src=T(_pts(10, 3)))),
    ('cpu_tensor_dst', dict(dst=T(_pts(10, 3)))), ('order_src_before_dst', dict(src=_pts(10), dst=_pts(10))),
    ('order_length_before_threshold', dict(dst=_pts(9, 3), threshold=0)), ('order_with_scale_before_rounds', dict(with_scale=2, rounds=9)),
    ('max_iters_not_integer_accepted', dict(max_iters=10.5)), ('passes', {})])
TABLE['rigid3d.register_points'] = (_r3, [('too_few', dict(src=_pts(2, 3), dst=_pts(2, 3))), ('rounds_over', dict(rounds=9)),
                                          ('order_dst_before_confidence', dict(dst=_pts(10), confidence=0)),
                                          ('order_squared_threshold_before_with_scale', dict(threshold=1e-30, with_scale=3))])
_rct = dict(points_a=_pts(12), points_b=_pts(12, 2, 1), depth_a=DEPTH, K_a=K, c2w_a=C2W, depth_b=DEPTH, K_b=K)
_small = np.ones((2, 5), np.float32)
TABLE['rigid3d.register_captures_tensors'] = (_rct, pair_cases('points_a', 'points_b', 2) + depth_cases('depth_a') + depth_cases('depth_b')
                                              + camera_cases('K_a') + camera_cases('K_b') + pose_cases('c2w_a') + _r3_checks + [
    ('icp_iters_under', dict(icp_iters=-1)), ('icp_iters_over', dict(icp_iters=65)), ('icp_iters_not_integer', dict(icp_iters=1.5)),
    ('icp_with_scale', dict(icp_iters=3, with_scale=True)), ('icp_depth_a_small', dict(icp_iters=3, depth_a=_small)),
    ('icp_depth_b_small', dict(icp_iters=3, depth_b=_small)), ('small_maps_accepted_without_icp', dict(depth_a=_small, depth_b=_small)),
    ('icp_max_dist_0', dict(icp_iters=3, icp_max_dist=0)), ('icp_max_dist_unread_without_icp', dict(icp_max_dist=0)),
    ('cpu_tensor_points_a', dict(points_a=T(_pts(12)))), ('cpu_tensor_depth_b', dict(depth_b=T(DEPTH))),
    ('order_depth_a_before_depth_b', dict(depth_a=DEPTH.astype(np.float64), depth_b=np.zeros(5, np.float32))),
    ('order_rounds_before_icp_iters', dict(rounds=9, icp_iters=65)), ('order_icp_before_cpu_tensor', dict(icp_iters=3, with_scale=True, depth_a=T(DEPTH))),
    ('max_iters_not_integer_accepted', dict(max_iters=10.5)), ('icp_passes', dict(icp_iters=3)), ('passes', {})])
_rcap = dict(points_a=_pts(12), points_b=_pts(12, 2, 1), cap_a=CAP, cap_b=CAP)
TABLE['rigid3d.register_captures'] = (_rcap, [('too_few', dict(points_a=_pts(2), points_b=_pts(2))), ('icp_iters_over', dict(icp_iters=65)),
                                              ('cpu_tensor_points_b', dict(points_b=T(_pts(12)))),
                                              ('order_points_before_threshold', dict(points_b=_pts(12, 3), threshold=0)),
                                              ('order_with_scale_before_icp_iters', dict(with_scale=5, icp_iters=-1))])

# ---- icp.py ---------------------------------------------------------------------------------------------------------------
_icp = dict(depth_a=DEPTH, K_a=K, depth_b=DEPTH, K_b=K, R0=np.eye(3), t0=np.zeros(3), max_dist=0.1)
TABLE['icp.icp_depth'] = (_icp, depth_cases('depth_a') + depth_cases('depth_b') + camera_cases('K_a') + camera_cases('K_b') + pose_cases('c2w_a') + [
    ('depth_a_small', dict(depth_a=_small)), ('depth_b_small', dict(depth_b=_small.T)), ('R0_shape', dict(R0=np.eye(4))),
    ('R0_flat_accepted', dict(R0=np.eye(3).reshape(9))), ('t0_shape', dict(t0=np.zeros(4))), ('t0_column_accepted', dict(t0=np.zeros((3, 1)))),
    ('t0_row_refused', dict(t0=np.zeros((1, 3)))), ('src_mask_shape', dict(src_mask=np.ones((48, 63), bool))),
    ('src_mask_float', dict(src_mask=np.ones((48, 64)))), ('src_mask_accepted', dict(src_mask=np.ones((48, 64), np.uint8))),
    ('max_dist_0', dict(max_dist=0)), ('max_dist_inf', dict(max_dist=np.inf)), ('normal_cos_over', dict(normal_cos=2)),
    ('normal_cos_nan', dict(normal_cos=np.nan)), ('edge_0', dict(edge=0)), ('cond_tol_0', dict(cond_tol=0)), ('cond_tol_1', dict(cond_tol=1)),
    ('iters_under', dict(iters=-1)), ('iters_over', dict(iters=65)), ('iters_not_integer', dict(iters=1.5)), ('stride_0', dict(stride=0)),
    ('stride_over', dict(stride=65)), ('stride_not_integer', dict(stride=1.5)), ('cpu_tensor_depth_a', dict(depth_a=T(DEPTH))),
    ('cpu_tensor_R0', dict(R0=T(np.eye(3)))), ('cpu_tensor_src_mask', dict(src_mask=torch.ones((48, 64), dtype=torch.bool))),
    ('order_depth_a_before_depth_b', dict(depth_a=_small, depth_b=DEPTH.astype(np.float64))), ('order_K_b_before_R0', dict(K_b=K_NAN, R0=np.eye(2))),
    ('order_src_mask_before_max_dist', dict(src_mask=np.ones(3, bool), max_dist=0)), ('order_stride_before_cpu_tensor', dict(stride=0, t0=torch.zeros(3))),
    ('passes', {})])
_rr = dict(cap_a=CAP, cap_b=CAP, c2w_b=C2W)
TABLE['icp.refine_registration'] = (_rr, [('c2w_b_none', dict(c2w_b=None)), ('c2w_b_shape', dict(c2w_b=np.eye(3))), ('c2w_b_nan', dict(c2w_b=C2W_NAN)),
                                          ('max_dist_0', dict(max_dist=0)), ('iters_over', dict(iters=65)),
                                          ('order_c2w_b_before_max_dist', dict(c2w_b=np.eye(3), max_dist=0)),
                                          ('order_edge_before_stride', dict(edge=-1, stride=0))])

# ---- triangulate.py -------------------------------------------------------------------------------------------------------
TABLE['triangulate.delaunay'] = (dict(points=_pts(8)), [('shape', dict(points=_pts(8, 3))), ('list_shape', dict(points=[1.0, 2.0])),
                                                        ('too_many', dict(points=big(65537, 2)))])
_tc = dict(corr=_c4, from_shape=(48, 64, 3), to_shape=(48, 64, 3))
TABLE['triangulate.triangulate_corr'] = (_tc, [
    ('simplices_word', dict(simplices='host')), ('corr_shape', dict(corr=_pts(6), simplices=np.zeros((1, 3), np.int64))),
    ('simplices_float', dict(simplices=np.zeros((1, 3)))), ('simplices_shape', dict(simplices=np.zeros((3, 2), np.int64))),
    ('simplices_index', dict(simplices=np.array([[0, 1, 6]]))), ('simplices_negative', dict(simplices=np.array([[0, 1, -1]]))),
    ('device_corr_shape', dict(corr=_pts(6), simplices='device')), ('device_too_many', dict(corr=big(65537, 4), simplices='device')),
    ('order_word_before_corr', dict(simplices='host', corr=_pts(6))), ('order_corr_before_simplices', dict(corr=_pts(6), simplices=np.zeros((1, 3))))])

# ---- warp.py --------------------------------------------------------------------------------------------------------------
_map = np.zeros((8, 9, 2), np.float32)
_image_cases = [('img_float', dict(img=IMG.astype(np.float32))), ('img_4d', dict(img=IMG[None])), ('img_channels', dict(img=IMG[..., :2])),
                ('img_too_large', dict(img=lambda: np.broadcast_to(np.uint8(0), (16385, 4))))]
_wm = dict(img=IMG, map=_map)
TABLE['warp.warp_by_map'] = (_wm, _image_cases + [
    ('map_int', dict(map=_map.astype(np.int32))), ('map_shape', dict(map=_map[..., 0])),
    ('map_too_large', dict(map=lambda: np.broadcast_to(np.float32(0), (4, 16385, 2)))), ('background_shape', dict(background=IMG)), ('background_float', dict(background=np.zeros((8, 9, 3)))),
    ('background_dims', dict(img=IMG[..., 0], background=np.zeros((8, 9, 1), np.uint8))), ('cpu_tensor_img', dict(img=T(IMG))),
    ('cpu_tensor_map', dict(map=T(_map))), ('order_img_before_map', dict(img=IMG[None], map=_map[..., 0])),
    ('order_background_before_cpu_tensor', dict(background=IMG, map=T(_map)))])
_wp = dict(img=IMG, M=np.eye(3), dsize=(9, 8))
TABLE['warp.warp_perspective'] = (_wp, _image_cases + [
    ('dsize_length', dict(dsize=(9, 8, 3))), ('dsize_not_integer', dict(dsize=(9.5, 8))), ('dsize_0', dict(dsize=(0, 8))), ('dsize_over', dict(dsize=(9, 16385))),
    ('background_shape', dict(background=IMG)), ('M_shape', dict(M=np.eye(2))), ('M_nan', dict(M=np.full((3, 3), np.nan))), ('M_singular', dict(M=np.ones((3, 3)))),
    ('M_singular_inverse_map', dict(M=np.eye(2), inverse_map=True)), ('cpu_tensor_img', dict(img=T(IMG))),
    ('cpu_tensor_background', dict(background=torch.zeros((8, 9, 3), dtype=torch.uint8))),
    ('order_dsize_before_M', dict(dsize=(0, 8), M=np.eye(2))), ('order_M_before_cpu_tensor', dict(M=np.ones((3, 3)), img=T(IMG)))])
TABLE['warp.invert_perspective'] = (dict(M=np.eye(3)), [('shape', dict(M=np.eye(4))), ('nan', dict(M=np.full((3, 3), np.inf))),
                                                       ('singular', dict(M=np.zeros((3, 3)))), ('passes', {})])
TABLE['warp.get_perspective_transform'] = (dict(src=QUAD, dst=QUAD), [
    ('src_shape', dict(src=QUAD[:3])), ('dst_shape', dict(dst=QUAD.T)), ('nan', dict(dst=QUAD * np.nan)), ('on_a_line', dict(src=np.outer(np.arange(4.0), [1, 1]))),
    ('order_shape_before_finite', dict(src=QUAD[:3], dst=QUAD * np.nan)), ('passes', {})])
TABLE['warp.paste_by_corners'] = (dict(picture=IMG, corners_b=QUAD, img_b=IMG), [
    ('picture_float', dict(picture=IMG.astype(np.float64))), ('img_b_4d', dict(img_b=IMG[None])), ('corners_shape', dict(corners_b=QUAD[:3])),
    ('corners_on_a_line', dict(corners_b=np.outer(np.arange(4.0), [1, 1]))), ('order_picture_before_img_b', dict(picture=IMG[None], img_b=IMG[None])),
    ('order_img_b_before_corners', dict(img_b=IMG[..., :2], corners_b=QUAD[:3]))])
TABLE['warp.warp_by_corr'] = (dict(img_a=IMG, img_b=IMG, corrs=_c4), [
    ('img_a_float', dict(img_a=IMG.astype(np.float32))), ('img_b_channels', dict(img_b=IMG[..., :2])), ('cpu_tensor_img_a', dict(img_a=T(IMG))),
    ('order_img_a_before_img_b', dict(img_a=IMG[None], img_b=IMG[None])), ('order_img_b_before_cpu_tensor', dict(img_b=IMG[None], img_a=T(IMG)))])
TABLE['warp.picture_corners'] = (dict(picture_shape=(4, 6, 3)), [('passes', {})])


def cases():
    """-> [(function, case id, base arguments, overrides)] in the table's order"""
    return [(path, cid, base, over) for path, (base, rows) in TABLE.items() for cid, over in rows]


# ---- the device sequences -------------------------------------------------------------------------------------------------
class Recorder:
    """Stands where ``_lib.load_library()`` returns the library: every entry point appends (its name, its arguments that are
    not addresses) to ``log`` and returns 0.  A pointer is logged as 'ptr' or 'null', a camera matrix as its 9 doubles."""

    def __init__(self):
        self.log = []

    @staticmethod
    def _plain(a):
        if a is None:
            return 'null'
        if isinstance(a, ctypes.c_void_p):
            return 'null' if a.value is None else 'ptr'
        if isinstance(a, ctypes.Array):
            return [float(v) for v in a]
        if isinstance(a, bool) or isinstance(a, (int, np.integer)):
            return 'ptr' if int(a) >= 1 << 32 else int(a)   # (the fixed-view mask of cotr_bundle_adjust goes as a host address)
        if isinstance(a, (float, np.floating)):
            return float(a)
        return type(a).__name__   # ctypes.byref(...): where a scratch size is written (it stays 0)

    def __getattr__(self, name):
        def entry(*args):
            self.log.append([name, [self._plain(a) for a in args]])
            return 0
        return entry


def _scene():
    pa, pb = _pts(24, 2, 5), _pts(24, 2, 6)
    return pa, pb, np.concatenate([pa, pb], axis=1)


def sequences():
    """{name: the call}; each runs on the CPU once ``cpu_patches`` are in place and the Recorder is the library"""
    from cotr_amd.inference.essential import relative_pose_tensors
    from cotr_amd.inference.pnp import localize_tensors
    from cotr_amd.inference.rigid3d import register_captures_tensors
    from cotr_amd.inference.structure import reconstruct_tensors
    pa, pb, corrs = _scene()
    K2 = K + np.array([[20.0, 0.5, 3], [0, 10, 2], [0, 0, 0]])
    return {
        'relative_pose_tensors(refine_rounds=4)': lambda: relative_pose_tensors(pa, pb, K, K2, threshold=1.5, max_iters=200, seed=3, refine_rounds=4,
                                                                                refine_iters=7),
        'relative_pose_tensors()': lambda: relative_pose_tensors(pa, pb, K, seed=-1),
        'register_captures_tensors(icp_iters=3)': lambda: register_captures_tensors(pa, pb, DEPTH, K, C2W, DEPTH, K2, threshold=0.04, seed=9, icp_iters=3),
        'register_captures_tensors(with_scale)': lambda: register_captures_tensors(pa, pb, DEPTH, K, None, DEPTH, K2, with_scale=True, rounds=0,
                                                                                   icp_max_dist=0.2),
        'localize_tensors': lambda: localize_tensors(pa, pb, DEPTH, K, C2W, K2, threshold=4.0, max_iters=50, seed=2, refine_iters=5),
        'reconstruct_tensors(bundle_rounds=2)': lambda: reconstruct_tensors(corrs, IMG, IMG, K, K2, bundle_rounds=2, threshold=3.0,
                                                                            pose_kw=dict(seed=4, max_iters=100)),
        'reconstruct_tensors(poses, demo)': lambda: reconstruct_tensors(corrs, IMG, IMG, K, None, C2W, np.linalg.inv(np.vstack([POSES[0], [0, 0, 0, 1]])
                                                                                                                          + np.eye(4, k=3)), rule='demo'),
    }


def cpu_patches(patch, recorder):
    """``patch(object, name, value)`` (pytest's monkeypatch.setattr) of everything the wrappers share that names the GPU; the
    wrappers' own device rule and CPU-tensor refusal are the caller's to replace, since where they live is what the golden
    file outlasts."""
    from cotr_amd import _lib
    patch(_lib, 'load_library', lambda: recorder)
    patch(_lib, 'current_stream_ptr', lambda: None)
    patch(torch.cuda, 'device', lambda device: contextlib.nullcontext())
