"""Which captures of a scene to pair for training: the overlap ("distance") matrix of a list of RGB-D captures, the
neighbour pool of every capture and a draw from it, on the device - what the reference prepares in numpy with
``scripts/prepare_nn_distance_mat.py`` (``distance_between_two_caps``, saved as ``dist_mat.npy``) and reads back in
``COTR/sfm_scenes/knn_search.py`` (``ReprojRatioKnnSearch.get_knn``) and ``megadepth_dataset.get_query_with_knn``.

    dist = overlap_matrix(caps)                      # float32 [N, N] on the device
    pool, counts = knn_pool(dist, k)                 # every query row at once
    nn = draw_pairs(pool, counts, u)                 # one neighbour per query from uniforms u
    make_zoom_batch([caps[i] for i in queries], [caps[j] for j in nn[queries].tolist()], ...)

The geometry runs in ``cotr_amd/csrc/overlap.hip`` (``cotr_world_points``, ``cotr_overlap_pairs``); the rule, the launch
structure, the scratch formula and the measured times are in DESIGN.md 3k.  ``knn_pool`` and ``draw_pairs`` are selection
on an N x N matrix: torch tensor operations on the device.  Captures are ``cotr_amd.data.Capture`` and go through that
module's checks: a CPU tensor is refused, there is no CPU fallback."""
import numpy as np
import torch

from . import _lib
from ._lib import check_op, on, ptr
from .data import _check_capture, _device_of, _pick

# Canvas scratch of one overlap_pairs call: one uint32 per pixel of the largest capture per pair in flight.  256 MiB holds
# 218 pairs of 480 x 640 captures, so a scene's matrix takes a handful of tiles and the per-tile launches do not show;
# the bound is a memory budget, not a tuned value.
SCRATCH_BYTES = 256 << 20
NN_THRESH = 0.1        # VALID_NN_OVERLAPPING_THRESH of the reference


def _check_caps(caps):
    caps = list(caps)
    if not caps:
        raise ValueError('caps must be a non-empty list of Capture')
    if len(caps) > 65535:
        raise ValueError('at most 65535 captures')
    shapes = [_check_capture(c, f'caps[{i}]', need_image=False) for i, c in enumerate(caps)]
    return caps, shapes


def _check_pairs(pairs, n_caps):
    """-> (host int32 [n, 2] or None, device tensor or None); host pairs are range-checked here, before any upload"""
    if torch.is_tensor(pairs):
        if not pairs.is_cuda:
            raise _lib.CotrHipError('pairs: got a CPU tensor; pass a numpy array or move the tensor with .cuda()')
        if pairs.dtype not in (torch.int32, torch.int64) or pairs.dim() != 2 or pairs.shape[1] != 2:
            raise ValueError('pairs must be an integer [n, 2] array of (q, d) capture indices')
        return None, pairs.to(torch.int32).contiguous()
    p = np.asarray(pairs)
    if p.size == 0:
        p = p.reshape(0, 2).astype(np.int32)
    if p.ndim != 2 or p.shape[1] != 2 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError('pairs must be an integer [n, 2] array of (q, d) capture indices')
    if p.size and (p.min() < 0 or p.max() >= n_caps):
        raise ValueError(f'pairs: capture indices must be in [0, {n_caps})')
    if p.shape[0] > 1 << 24:
        raise ValueError('at most 2^24 pairs in one call')
    return np.ascontiguousarray(p, dtype=np.int32), None


def _tables(depths, xyz, shapes, device):
    """caps [n, 2] uint64 (as int64) and shapes [n, 2] int32, uploaded; xyz[i] None -> address 0"""
    ptrs = [(d.data_ptr(), x.data_ptr() if x is not None else 0) for d, x in zip(depths, xyz)]
    return torch.tensor(ptrs, dtype=torch.int64).to(device), torch.tensor(shapes, dtype=torch.int32).to(device)


def _world_points(caps, shapes, depths, need, device):
    """cotr_world_points for the captures with need[i] -> list of xyz float32 [H W, 3] (None where not needed)"""
    xyz = [torch.empty((h * w, 3), dtype=torch.float32, device=device) if nd else None for (h, w), nd in zip(shapes, need)]
    sel = [i for i, nd in enumerate(need) if nd]
    if sel:
        cams = np.stack([np.concatenate([np.linalg.inv(np.asarray(caps[i].K)).ravel(), np.asarray(caps[i].c2w).ravel()]) for i in sel])
        ptrs, shp = _tables([depths[i] for i in sel], [xyz[i] for i in sel], [shapes[i] for i in sel], device)
        cams = torch.from_numpy(cams).to(device)
        with torch.cuda.device(device):
            check_op(_lib.load_library().cotr_world_points(ptr(ptrs), ptr(shp), ptr(cams), len(sel), max(h * w for h, w in shapes),
                                                           _lib.current_stream_ptr()), 'cotr_world_points')
    return xyz


def world_points(caps):
    """``Capture.point_cloud_world`` of every capture, kept per pixel: per capture ``(xyz float32 [H W, 3], valid bool [H W])``
    on the device, in row-major pixel order.  A pixel is valid iff its depth and the z of its camera-space point are > 0
    (and the homogeneous w is not 0); the reference's point cloud is ``xyz[valid]``.  xyz of an invalid pixel is NaN.
    Rule: DESIGN.md 3k step 1 (float64 arithmetic, the result rounded to float32)."""
    caps, shapes = _check_caps(caps)
    device = _device_of(caps)
    depths = [on(c.depth, device) for c in caps]
    xyz = _world_points(caps, shapes, depths, [True] * len(caps), device)
    return [(x, ~torch.isnan(x[:, 2])) for x in xyz]


def overlap_pairs(caps, pairs, max_pairs_in_flight=None):
    """``distance_between_two_caps((caps[q], caps[d]))`` for every row ``(q, d)`` of ``pairs`` (int [n, 2]; a numpy array or
    list, range-checked on the host, or a device tensor, where a row with an index out of range scores 0) ->
    ``(ratio float32 [n], counts int32 [n, 2] = (good, union))`` on the device, ratio = float32(good / union).
    The world points of a capture are computed once, however many pairs name it as ``d`` (for a device ``pairs``: of every
    capture).  max_pairs_in_flight bounds the canvas scratch, 4 bytes x the pixels of the largest capture per pair in
    flight; default: as many as ``SCRATCH_BYTES`` (256 MiB) holds.  The result does not depend on it, and two runs return
    the same bytes.  No host wait."""
    caps, shapes = _check_caps(caps)
    host_pairs, dev_pairs = _check_pairs(pairs, len(caps))
    if max_pairs_in_flight is not None and (int(max_pairs_in_flight) != max_pairs_in_flight or max_pairs_in_flight < 1):
        raise ValueError('max_pairs_in_flight must be a positive integer')
    device = _device_of(caps)
    n = host_pairs.shape[0] if host_pairs is not None else dev_pairs.shape[0]
    ratio = torch.zeros(n, dtype=torch.float32, device=device)
    counts = torch.zeros((n, 2), dtype=torch.int32, device=device)
    if n == 0:
        return ratio, counts
    lib = _lib.load_library()
    depths = [on(c.depth, device) for c in caps]
    need = [True] * len(caps) if host_pairs is None else [bool(x) for x in np.isin(np.arange(len(caps)), host_pairs[:, 1])]
    xyz = _world_points(caps, shapes, depths, need, device)
    max_px = max(h * w for h, w in shapes)
    per = lib.cotr_overlap_scratch(1, max_px)
    in_flight = min(n, 65535, int(max_pairs_in_flight) if max_pairs_in_flight is not None else max(1, SCRATCH_BYTES // per))
    nbytes = lib.cotr_overlap_scratch(in_flight, max_px)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)
    ptrs, shp = _tables(depths, xyz, shapes, device)
    proj = np.stack([np.matmul(np.asarray(c.K), np.linalg.inv(np.asarray(c.c2w))[0:3, :]).ravel() for c in caps])
    proj = torch.from_numpy(proj).to(device)
    dpairs = dev_pairs.to(device) if dev_pairs is not None else torch.from_numpy(host_pairs).to(device)
    with torch.cuda.device(device):
        check_op(lib.cotr_overlap_pairs(ptr(ptrs), ptr(shp), ptr(proj), len(caps), ptr(dpairs), n, max_px, ptr(ratio), ptr(counts),
                                        ptr(scratch), nbytes, _lib.current_stream_ptr()), 'cotr_overlap_pairs')
    return ratio, counts


def overlap_matrix(caps, covisible=None, max_pairs_in_flight=None):
    """The reference's ``dist_mat`` of a scene -> float32 [N, N] on the device, ``[i, j] = overlap(caps[i], caps[j])`` with
    caps[i] the query (its depth support is compared) and caps[j] the database capture (its points are projected).  The
    diagonal is computed like any other cell.
    covisible: optional host bool [N, N]; a False cell is 0 and is not computed (the reference's ``fill_covisibility`` and
    its shared-3D-point early-out, with the SfM knowledge supplied by the caller)."""
    caps, _ = _check_caps(caps)
    n = len(caps)
    if covisible is None:
        cov = np.ones((n, n), dtype=bool)
    else:
        if torch.is_tensor(covisible):
            raise ValueError('covisible must be a host bool [N, N] array (the cells to compute are chosen on the host)')
        cov = np.asarray(covisible)
        if cov.dtype != np.bool_ or cov.shape != (n, n):
            raise ValueError(f'covisible must be a bool [{n}, {n}] array, got {cov.dtype} {cov.shape}')
    pairs = np.argwhere(cov).astype(np.int32)
    ratio, _ = overlap_pairs(caps, pairs, max_pairs_in_flight)
    dist = torch.zeros(n * n, dtype=torch.float32, device=ratio.device)
    if pairs.shape[0]:
        dist[torch.from_numpy(pairs[:, 0].astype(np.int64) * n + pairs[:, 1]).to(ratio.device)] = ratio
    return dist.view(n, n)


def _check_dist(dist):
    if not torch.is_tensor(dist):
        raise ValueError('dist must be a device tensor (overlap_matrix returns one)')
    if not dist.is_cuda:
        raise _lib.CotrHipError('dist: got a CPU tensor; move it with .cuda()')
    if dist.dtype != torch.float32 or dist.dim() != 2 or dist.shape[0] != dist.shape[1] or dist.shape[0] < 1:
        raise ValueError(f'dist must be float32 [N, N], got {dist.dtype} {tuple(dist.shape)}')
    return dist.shape[0]


def knn_pool(dist, k, db_mask=None):
    """``ReprojRatioKnnSearch.get_knn(query, k, db_mask)`` for EVERY query row of ``dist`` (float32 [N, N], device) at once ->
    ``(indices int64 [N, k], counts int64 [N])`` on the device; row i lists counts[i] >= 1 neighbours by descending
    overlap and is padded with -1.  db_mask: optional list of the capture indices that may be neighbours (as in the
    reference); the others are set to -1 before the ranking.  Branch for branch: num_pos = #(row > 0.1) over the db_mask;
    num_pos > k: the top k + 1, minus the query itself if it is among them, else minus the last; otherwise the top
    max(num_pos, 1), the query itself NOT removed (so a capture without a valid neighbour gets one entry of overlap <= 0.1,
    possibly itself: check ``dist`` at the drawn pair).  Ties go to the lower index (the reference leaves them undefined)."""
    n = _check_dist(dist)
    if int(k) != k or k < 1:
        raise ValueError('k must be a positive integer')
    k = int(k)
    device = dist.device
    inside = torch.ones(n, dtype=torch.bool, device=device)
    if db_mask is not None:
        m = np.asarray(db_mask.cpu() if torch.is_tensor(db_mask) else db_mask)
        if m.ndim != 1 or not np.issubdtype(m.dtype, np.integer) or (m.size and (m.min() < 0 or m.max() >= n)):
            raise ValueError(f'db_mask must be a list of capture indices in [0, {n})')
        host = np.zeros(n, dtype=bool)
        host[m] = True
        inside = torch.from_numpy(host).to(device)
    num_pos = ((dist > NN_THRESH) & inside).sum(1)
    temp = torch.where(inside, dist, torch.full_like(dist, -1.0))
    order = torch.sort(temp, dim=1, descending=True, stable=True).indices                # ties: the lower index first
    width = k + 1
    if n < width:
        order = torch.cat([order, torch.full((n, width - n), -1, dtype=order.dtype, device=device)], 1)
    top = order[:, :width]
    me = torch.arange(n, device=device).unsqueeze(1)
    j = torch.arange(k, device=device).unsqueeze(0)
    is_me = top == me
    self_at = torch.where(is_me.any(1), is_me.to(torch.int64).argmax(1), torch.full((n,), width, device=device)).unsqueeze(1)
    enough = (num_pos > k).unsqueeze(1)
    without_me = torch.gather(top, 1, j + (self_at <= j).to(torch.int64))                # the top k + 1 with the query taken out
    few = torch.clamp(num_pos, min=1).unsqueeze(1)
    short = torch.where(j < few, top[:, :k], torch.full_like(top[:, :k], -1))
    indices = torch.where(enough, without_me, short)
    counts = torch.where(enough[:, 0], torch.full_like(num_pos, k), few[:, 0])
    return indices, counts


def draw_pairs(pool, counts, u):
    """One neighbour per query out of ``knn_pool``'s lists: entry floor(u count) of every row -> int64 [N] on the device.
    u: uniforms in [0, 1), float64 [N] (numpy or device) - the ``random.sample(pool, 1)`` of
    ``megadepth_dataset.get_query_with_knn`` under the randomness contract of ``cotr_amd.data``."""
    for name, t in (('pool', pool), ('counts', counts)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.CotrHipError(f'{name} must be a device tensor (knn_pool returns one)')
    if torch.is_tensor(u) and not u.is_cuda:
        raise _lib.CotrHipError('u: got a CPU tensor; pass a numpy array or move the tensor with .cuda()')
    if pool.dim() != 2 or tuple(counts.shape) != (pool.shape[0],):
        raise ValueError('pool must be [N, k] and counts [N]')
    u = on(np.asarray(u, dtype=np.float64) if not torch.is_tensor(u) else u, pool.device).double()
    if tuple(u.shape) != (pool.shape[0],):
        raise ValueError(f'u must have shape ({pool.shape[0]},), got {tuple(u.shape)}')
    return torch.gather(pool, 1, _pick(u.unsqueeze(1), counts))[:, 0]
