"""Host-side engines for the MI355X model object.

The reference's own engines (``COTR/inference/sparse_engine.py``) keep working unchanged against
``cotr_amd.models.build_model`` (same call contract).  ``ZoomEngine`` is the MI355X-native way to run the
same recursive zoom-in: it stays host-side Python as the reference's is, but every zoom level is ONE
device-side crop+resize launch and one batched encode/decode instead of one PIL resize, one H2D copy and
one backbone pass per query per level.  ``triangulate_corr`` densifies the sparse correspondences they return (one
rasterisation launch sequence on the device).  ``mutual_matches``, ``find_fundamental_mat`` and ``filter_guided_matches``
are the guided-matching post-processing of demo_guided_matching.py (nearest keypoints, mutual check, F-matrix RANSAC) as
device calls; ``ZoomEngine.guided_match`` runs the whole demo.  ``warp_by_map``, ``warp_perspective`` and
``get_perspective_transform`` are the demos' ``cv2.remap`` / ``cv2.warpPerspective`` / ``cv2.getPerspectiveTransform`` (8-bit
bilinear, one launch each); ``warp_by_corr`` and ``paste_by_corners`` are the last lines of demo_single_pair.py and
demo_homography.py.  ``find_homography`` is ``cv2.findHomography(..., cv2.RANSAC)`` on the device (RANSAC, then a
least-squares refit on the inliers), ``paste_by_homography`` the robust form of ``paste_by_corners`` and
``ZoomEngine.homography`` the robust form of the whole demo.  ``find_essential_mat`` and ``recover_pose`` are
``cv2.findEssentialMat(..., cv2.RANSAC)`` (five-point RANSAC) and ``cv2.recoverPose`` on the device, ``ransac_essential`` the
former with device tensors, ``relative_pose`` both as one device sequence and ``ZoomEngine.relative_pose`` the pose after
demo_wbs.py's correspondences; ``refine_relative_pose`` refits such a pose on its inliers (Gauss-Newton on the Sampson error,
the inliers re-counted between rounds), ``refine_pose_tensors`` the same with device tensors, and ``relative_pose(...,
refine_rounds=4)`` runs it third in the same device sequence.  ``solve_pnp_ransac`` is ``cv2.solvePnPRansac(..., flags=cv2.SOLVEPNP_P3P)`` on the device (P3P RANSAC,
then a Gauss-Newton refit on the inliers), ``ransac_pnp`` the same with device tensors, ``lift_pixels`` the 3D points of pixels of
a depth map, ``rodrigues`` ``cv2.Rodrigues``, and ``localize`` / ``ZoomEngine.localize`` the metric pose of a new image against a
posed RGB-D capture.  ``triangulate_views`` triangulates correspondences seen in 2 to 32 posed views in one device call (the views
of a point that agree are voted on, the point is refitted on its reprojection error), ``triangulate_points`` is its two-view form
after ``relative_pose`` or ``localize``, ``stack_views`` shapes one query set matched against several images for it, and
``ZoomEngine.reconstruct`` is demo_reconstruction.py up to its viewer.  ``bundle_adjust`` refines the poses of such views and
their points together (Levenberg-Marquardt by the Schur complement, one device call), ``bundle_adjust_tensors`` the same with device
tensors, and ``reconstruct(..., bundle_rounds=2)`` runs it after the triangulation.  ``register_points`` is the robust absolute
orientation of 3D-3D correspondences (3-point RANSAC on Horn's closed form, a closed-form refit on the inliers; a similarity with
``with_scale=True``), ``ransac_rigid3d`` the same with device tensors, and ``register_captures`` / ``ZoomEngine.register`` the
metric pose of one RGB-D capture against another from both depth maps.  ``icp_depth`` refines a rigid motion on every pixel of two
depth maps (projective association, point-to-plane Gauss-Newton), ``refine_registration`` the same on two captures, and
``register_captures(..., icp_iters=10)`` runs it behind the sparse registration.  ``icp_multiview`` refines the poses of 2 to 32 depth maps
together on every pixel of every overlapping ordered pair (multi-way ICP, one normal system per step), ``vertex_normal_maps`` makes the
maps it reads, ``refine_poses`` is the same on captures, and ``ZoomEngine.fuse(..., joint_iters=4)`` runs it before the fusion.  ``TsdfVolume`` is a truncated signed distance volume on
the device, ``integrate_depths`` averages posed depth maps into it and ``fuse_captures`` posed captures, ``raycast_volume`` is the depth
map (and normals) of its surface seen from a pose, ``track_capture`` ``icp_depth`` against such a map (frame-to-model tracking),
``extract_mesh`` its surface as an indexed triangle mesh (``write_ply`` puts it into a file), and ``ZoomEngine.fuse`` registers a list
of captures against the first and fuses those it placed.  ``depth_from_corr`` turns the correspondence maps of a posed reference view into 1 to 31 posed
neighbours into its depth map (a depth per pixel voted on over the neighbours and refitted on the reprojection error), ``flow_to_corr`` takes
``ZoomEngine.flow``'s map to the pixels it reads, ``filter_depths`` checks 2 to 32 depth maps against each other (``filter_captures`` on captures),
and ``ZoomEngine.depth_map`` / ``ZoomEngine.fuse_images`` run them from posed photographs to a fused volume.  ``refine_depth_photo``
checks such a depth map against the pixels it describes (a photometric plane sweep around each pixel's depth over the posed neighbour images,
``to_grey`` of them; ``refine_captures_photo`` on captures), and ``depth_map(..., photo_sweeps=2)`` runs it behind ``depth_from_corr``.
``average_rotations`` turns relative rotations over a graph of view pairs into the rotations of 2 to 32 views (a greedy tree, then
annealed robust steps on the graph; every edge comes back with its residual and inlier flag), ``solve_positions`` places the camera
centres and the points on the tracks with those rotations (the points eliminated, the smallest eigenvector of the reduced matrix),
``reconstruct_views_tensors`` chains the two-view poses, both, the triangulation and the bundle adjustment as one device sequence,
and ``ZoomEngine.reconstruct_views`` runs it from photographs and intrinsics to the poses ``fuse_images`` takes.
``build_tracks_tensors`` turns the keypoint index pairs of ``mutual_matches`` over many view pairs into multi-view tracks (the
connected components of the match graph, a view seen twice in conflict; ``build_tracks`` with host arrays),
``reconstruct_tracks_tensors`` chains the two-view poses, their inlier masks, the tracks and the same tail, and
``ZoomEngine.reconstruct_keypoints`` runs it from photographs, intrinsics and keypoints.  ``detect_keypoints_tensors`` makes those
keypoints (a corner score on the integer structure tensor of 8-bit images, non-maximum suppression and the best K under a total
order, sub-pixel positions; defined exactly), ``detect_keypoints`` is its host form, and ``ZoomEngine.detect_keypoints`` the
same on the engine: ``guided_match`` and ``reconstruct_keypoints`` call it when they are given no keypoints."""
from .bundle import bundle_adjust, bundle_adjust_tensors
from .depth import depth_from_corr, filter_captures, filter_depths, flow_to_corr, refine_captures_photo, refine_depth_photo, to_grey
from .essential import find_essential_mat, ransac_essential, recover_pose, refine_pose_tensors, refine_relative_pose, relative_pose
from .global_pose import average_rotations, average_rotations_host, solve_positions, solve_positions_host
from .guided import filter_guided_matches, find_fundamental_mat, mutual_matches
from .homography import find_homography, paste_by_homography, ransac_homography
from .keypoints import detect_keypoints, detect_keypoints_tensors
from .icp import icp_depth, refine_registration
from .icp_multi import icp_multiview, refine_poses, vertex_normal_maps
from .pnp import lift_pixels, localize, ransac_pnp, rodrigues, solve_pnp_ransac
from .rigid3d import ransac_rigid3d, register_captures, register_captures_tensors, register_points
from .structure import reconstruct_tensors, reconstruct_views_tensors, stack_views, triangulate_points, triangulate_points_tensors, triangulate_views
from .tracks import build_tracks, build_tracks_tensors, reconstruct_tracks_tensors
from .triangulate import delaunay, triangulate_corr
from .tsdf import (TsdfVolume, color_depth_map, extract_mesh, fuse_captures, integrate_colors, integrate_depths, raycast_volume, sample_colors,
                   track_capture, write_ply)
from .warp import get_perspective_transform, paste_by_corners, warp_by_corr, warp_by_map, warp_perspective
from .zoom_engine import FasterSparseEngine, RefineResult, SparseEngine, ZoomEngine, patch_boxes

__all__ = ['ZoomEngine', 'SparseEngine', 'FasterSparseEngine', 'patch_boxes', 'RefineResult', 'triangulate_corr', 'delaunay',
           'mutual_matches', 'find_fundamental_mat', 'filter_guided_matches', 'warp_by_map', 'warp_perspective',
           'get_perspective_transform', 'warp_by_corr', 'paste_by_corners', 'find_homography', 'ransac_homography',
           'paste_by_homography', 'find_essential_mat', 'ransac_essential', 'recover_pose', 'relative_pose',
           'refine_pose_tensors', 'refine_relative_pose',
           'lift_pixels', 'ransac_pnp', 'solve_pnp_ransac', 'rodrigues', 'localize',
           'triangulate_views', 'triangulate_points', 'triangulate_points_tensors', 'stack_views', 'reconstruct_tensors',
           'bundle_adjust', 'bundle_adjust_tensors', 'average_rotations', 'average_rotations_host', 'solve_positions', 'solve_positions_host',
           'reconstruct_views_tensors', 'build_tracks', 'build_tracks_tensors', 'reconstruct_tracks_tensors',
           'ransac_rigid3d', 'register_points', 'register_captures', 'register_captures_tensors',
           'icp_depth', 'refine_registration', 'vertex_normal_maps', 'icp_multiview', 'refine_poses',
           'TsdfVolume', 'integrate_depths', 'fuse_captures', 'raycast_volume', 'track_capture', 'extract_mesh', 'write_ply',
           'integrate_colors', 'sample_colors', 'color_depth_map', 'depth_from_corr', 'flow_to_corr', 'filter_depths', 'filter_captures',
           'to_grey', 'refine_depth_photo', 'refine_captures_photo', 'detect_keypoints', 'detect_keypoints_tensors']
