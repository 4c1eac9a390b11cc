"""Multi-view tracks from pairwise keypoint matches, on the device: the step between ``mutual_matches`` and the N-view calls
(``solve_positions``, ``triangulate_views``, ``bundle_adjust``), which consume points [V,N,2] and visible [V,N].

``build_tracks_tensors`` is one ``cotr_build_tracks`` call (cotr_amd/csrc/tracks.hip, rules in DESIGN.md 3h-21) on the current
device and stream: the connected components of the match graph over the keypoints of all views, a component's label its
smallest node, a view that a component holds twice in conflict, the tracks numbered by label.  All of it is integer work: the
result does not depend on the order of the matches.  ``build_tracks`` is the host form, from the per-pair index pairs that
``mutual_matches`` returns.  ``reconstruct_tracks_tensors`` chains the two-view poses of the pairs, their inlier masks as the
matches kept, the tracks, and the tail of ``structure.reconstruct_views_tensors``.  No CPU fallback."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .._lib import check_op, on, ptr
from . import _args
from ._args import F64, I32, MAX_VIEWS, U8

MAX_NODES = 1 << 21
MAX_MATCHES = 1 << 24
MIN_PAIR_MATCHES = 5    # what the five-point estimator needs
CONFLICTS = ('drop', 'views')
_SUBJECT = 'the tracks are built'


def _keypoint_sets(keypoints):
    """a list of V arrays or tensors [k_v, 2] -> (float64 tensors where they were, offsets int64 [V + 1])"""
    kps = [_args.points(k, f'keypoints[{v}]') if len(k) else torch.zeros((0, 2), dtype=F64) for v, k in enumerate(keypoints)]
    return kps, np.concatenate([[0], np.cumsum([int(k.shape[0]) for k in kps])]).astype(np.int64)


def _nodes(nodes):
    """``offsets`` [V + 1] (host integers) or a list of V keypoint sets -> (offsets int64 [V + 1], the keypoint tensors or None)"""
    if isinstance(nodes, (list, tuple)) and len(nodes) and hasattr(nodes[0], 'shape') and len(nodes[0].shape) == 2:
        kps, offsets = _keypoint_sets(nodes)
    else:
        if torch.is_tensor(nodes) and nodes.is_cuda:
            raise ValueError('offsets must be host integers (K = offsets[V] sizes the call)')
        a = np.asarray(nodes.numpy() if torch.is_tensor(nodes) else nodes)
        if a.ndim != 1 or a.dtype.kind not in 'iu':
            raise ValueError(f'offsets must be integers [V + 1], or a list of [k, 2] keypoint sets, got {a.dtype} {a.shape}')
        kps, offsets = None, a.astype(np.int64)
    V = len(offsets) - 1
    if not 2 <= V <= MAX_VIEWS:
        raise ValueError(f'between 2 and {MAX_VIEWS} views, got {V}')
    if offsets[0] != 0 or (np.diff(offsets) < 0).any():
        raise ValueError('offsets must not decrease and must start at 0')
    if not 1 <= offsets[V] <= MAX_NODES:
        raise ValueError(f'between 1 and 2^21 keypoints in all, got {offsets[V]}')
    return offsets, kps


def _policy(conflict):
    if conflict not in CONFLICTS:
        raise ValueError(f'conflict must be one of {CONFLICTS}, got {conflict!r}')
    return CONFLICTS.index(conflict)


def _enqueue_tracks(lib, offsets, matches, keep, keypoints, V, K, M, min_views, policy, cap, device):
    """every tensor on ``device`` already, every argument checked -> the dict of ``build_tracks_tensors``"""
    count = ctypes.c_size_t()
    check_op(lib.cotr_build_tracks_work_ints(K, M, ctypes.byref(count)), 'cotr_build_tracks_work_ints')
    track_of_node, node, visible, info, work = _args.empty(device, (K, I32), ((V, cap), I32), ((V, cap), U8), (8, I32), (count.value, I32))
    points = None if keypoints is None else torch.empty((V, cap, 2), dtype=F64, device=device)
    check_op(lib.cotr_build_tracks(ptr(offsets), ptr(matches), ptr(keep), ptr(keypoints), V, K, M, int(min_views), policy, cap, ptr(track_of_node),
                                   ptr(node), ptr(visible), ptr(points), ptr(info), ptr(work), _lib.current_stream_ptr()), 'cotr_build_tracks')
    return dict(track_of_node=track_of_node, node=node, visible=visible.bool(), points=points, info=info, offsets=offsets)


def build_tracks_tensors(nodes, matches, keep=None, min_views=2, conflict='drop', cap=None, device=None):
    """One ``cotr_build_tracks`` call on the current stream.  ``nodes``: the host table offsets [V + 1] (node g
    is keypoint g - offsets[v] of view v when offsets[v] <= g < offsets[v + 1]), or a list of V keypoint sets [k_v, 2], which
    gives the table and the coordinates; matches int [M, 2] of node ids, keep [M] (None: every match; 0: the match is dead, as
    is one with an id out of range or both ids in one view), arrays or device tensors -> dict of device tensors: track_of_node
    int32 [K] (-1: not written), node int32 [V, cap] (the keypoint's index in its view, -1 where not visible), visible bool
    [V, cap], points float64 [V, cap, 2] (NaN where not visible; None without keypoints), info int32 [8] = (tracks found,
    tracks written, observations written, live matches, components, components with a view in conflict, components that are
    too short, views of the longest written track), offsets int32 [V + 1].  A component of the live matches that holds two
    keypoints of one view has that view in conflict: 'drop' drops the component, 'views' takes those views out of it; what is
    left is a track when it spans at least ``min_views`` views.  Tracks are numbered by their smallest node; the first ``cap``
    are written (None: min(K // 2, M), which cannot overflow), columns from info[1] on are empty."""
    offsets, kps = _nodes(nodes)
    V, K = len(offsets) - 1, int(offsets[-1])
    m = _args.tensor(matches, np.int32)
    if m.dim() != 2 or m.shape[1] != 2 or m.dtype not in (torch.int32, torch.int64):
        raise ValueError(f'matches must be int [M, 2], got {m.dtype} {tuple(m.shape)}')
    M = int(m.shape[0])
    if M > MAX_MATCHES:
        raise ValueError(f'at most 2^24 matches, got {M}')
    k = None if keep is None else _args.tensor(keep, None)
    if k is not None and tuple(k.shape) != (M,):
        raise ValueError(f'keep must be [M] = [{M}], got shape {tuple(k.shape)}')
    _args.check_int_range('min_views', min_views, 2, V)
    policy = _policy(conflict)
    cap = min(K // 2, M) if cap is None else cap
    _args.check_int_range('cap', cap, 0, K // 2)
    _args.no_cpu_tensors(_SUBJECT, matches, keep, *(nodes if kps is not None else ()))
    device = _args.device(device)
    m = on(m.to(dtype=I32), device).contiguous()
    kp = None if kps is None else on(torch.cat([t.to(device) for t in kps]), device).contiguous()
    with torch.cuda.device(device):
        return _enqueue_tracks(_lib.load_library(), on(torch.from_numpy(offsets.astype(np.int32)), device), m, _args.mask_u8(k, (M,), device), kp,
                               V, K, M, min_views, policy, int(cap), device)


def _pair_matches(offsets, pair_matches):
    """{(i, j): int [m, 2] of indices local to views i and j} -> [((i, j), int64 [m, 2] of node ids)] in the dict's order"""
    V, out = len(offsets) - 1, []
    for key, m in pair_matches.items():
        if not isinstance(key, tuple) or len(key) != 2 or not all(0 <= int(v) < V for v in key) or int(key[0]) == int(key[1]):
            raise ValueError(f'a pair must be (i, j) of two different views in [0, {V}), got {key!r}')
        i, j = int(key[0]), int(key[1])
        a = np.asarray(m.cpu() if torch.is_tensor(m) else m)
        if a.size == 0:
            a = np.zeros((0, 2), np.int64)
        if a.ndim != 2 or a.shape[1] != 2 or a.dtype.kind not in 'iu':
            raise ValueError(f'the matches of pair {key} must be int [m, 2], got {a.dtype} {a.shape}')
        a = a.astype(np.int64)
        sizes = np.array([offsets[i + 1] - offsets[i], offsets[j + 1] - offsets[j]])
        if (a < 0).any() or (a >= sizes).any():
            raise ValueError(f'the matches of pair {key} must index the {sizes[0]} and {sizes[1]} keypoints of its views')
        out.append(((i, j), a + np.array([offsets[i], offsets[j]])))
    return out


def build_tracks(keypoints, pair_matches, min_views=2, conflict='drop', cap=None):
    """The host form: ``keypoints`` a list of V arrays [k_v, 2], ``pair_matches`` a dict {(i, j): int [m, 2]} of index pairs
    local to views i and j, as ``mutual_matches`` returns them -> dict of host arrays trimmed to the n tracks written: points
    float64 [V, n, 2], visible uint8 [V, n], node int32 [V, n], track_of_node int32 [K], info int32 [8], offsets int32 [V + 1]."""
    offsets, _ = _nodes(list(keypoints))
    pairs = _pair_matches(offsets, pair_matches)
    matches = np.concatenate([m for _, m in pairs]) if pairs else np.zeros((0, 2), np.int64)
    r = build_tracks_tensors(list(keypoints), matches, min_views=min_views, conflict=conflict, cap=cap)
    out = {k: v.cpu().numpy() for k, v in r.items()}
    n = int(out['info'][1])
    out['points'], out['node'], out['visible'] = out['points'][:, :n], out['node'][:, :n], out['visible'][:, :n].astype(np.uint8)
    return out


def reconstruct_tracks_tensors(keypoints, pair_matches, cameras, root=0, pose_kw=None, track_kw=None, rotation_kw=None, position_kw=None,
                               bundle_rounds=2, device=None, **kw):
    """The poses of V views (2 to 32) and the points they see from keypoints and their pairwise matches, as one device
    sequence with no host wait.  ``keypoints``: a list of V sets [k_v, 2]; ``pair_matches``: a dict
    {(i, j): int [m, 2]} of local index pairs (``mutual_matches``); ``cameras`` as for ``reconstruct_views_tensors``, host.  Per
    pair ``relative_pose_tensors`` on the matched keypoints (``pose_kw``; refine_rounds 4 unless given) gives the edge (i, j)
    its rotation, its inlier count as weight and its found flag; a pair with fewer than 5 matches is left out.  The inlier
    masks, each ANDed with its found flag, are the ``keep`` of ``build_tracks_tensors`` (``track_kw``: min_views, conflict,
    cap) over all pairs' matches, so a wrong match that the two-view geometry refuses ties nothing together.  The tracks then
    take the tail of ``reconstruct_views_tensors``: ``average_rotations`` (``rotation_kw``), ``solve_positions``
    (``position_kw``), ``triangulate_views`` (``kw``) and ``bundle_adjust_tensors`` (``bundle_rounds``).  -> its dict (N = the
    tracks' cap: columns past the tracks written are empty and masked out) plus ``tracks``, the dict of ``build_tracks_tensors``."""
    from .essential import relative_pose_tensors
    from .structure import _enqueue_view_poses
    offsets, kps = _nodes(list(keypoints))
    V = len(offsets) - 1
    pairs_in = [(key, m) for key, m in _pair_matches(offsets, pair_matches) if m.shape[0] >= MIN_PAIR_MATCHES]
    if not pairs_in:
        raise ValueError(f'reconstruct_tracks needs at least one pair with {MIN_PAIR_MATCHES} matches')
    if len(pairs_in) > V * (V - 1):
        raise ValueError(f'at most V (V - 1) = {V * (V - 1)} view pairs, got {len(pairs_in)}')
    rows = _args.cam_rows(cameras, V)
    if rows.is_cuda:
        raise ValueError('cameras must be host arrays (the two-view estimators read them on the host)')
    if int(bundle_rounds) != bundle_rounds or bundle_rounds < 0:
        raise ValueError(f'bundle_rounds must be an integer >= 0, got {bundle_rounds}')
    _args.check_int_range('root', root, 0, V - 1)
    _args.no_cpu_tensors(_SUBJECT, *keypoints)
    rows = rows.numpy()
    Ks = [np.array([[r[0], r[4], r[2]], [0.0, r[1], r[3]], [0.0, 0.0, 1.0]]) for r in rows]
    device = _args.device(device)
    with torch.cuda.device(device):
        kp = torch.cat([t.to(device) for t in kps])
        matches = torch.from_numpy(np.concatenate([m for _, m in pairs_in])).to(device)
        edges, pairs, keeps, at = [], [], [], 0
        for (i, j), m in pairs_in:
            g = matches[at:at + m.shape[0]]
            pose = relative_pose_tensors(kp[g[:, 0]].contiguous(), kp[g[:, 1]].contiguous(), Ks[i], Ks[j], device=device,
                                         **dict(dict(refine_rounds=4), **(pose_kw or {})))
            keeps.append(pose['mask'] & (pose['info'][0] != 0))
            edges.append((i, j))
            pairs.append(pose)
            at += m.shape[0]
        tracks = build_tracks_tensors(list(keypoints), matches, keep=torch.cat(keeps), device=device, **(track_kw or {}))
        if tracks['points'].shape[1] < 1:
            raise ValueError('reconstruct_tracks needs room for at least one track (cap >= 1)')
        r = _enqueue_view_poses(tracks['points'], tracks['visible'], rows, edges, pairs, V, root, rotation_kw, position_kw, bundle_rounds, kw, device)
    r['tracks'] = tracks
    return r
