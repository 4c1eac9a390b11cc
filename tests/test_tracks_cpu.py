"""build_tracks without a GPU: the restatement (tests/tracks_oracle.py) against scipy's connected components and against
hand-made graphs for every rule of DESIGN.md 3h-21, the argument errors of the C ABI (refused before any HIP call) and of the
wrappers, and the host logic of the drivers with the device calls replaced."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from cotr_amd import _lib
from cotr_amd.inference import ZoomEngine, essential, guided, structure, tracks
from tests import tracks_oracle as to

OUTPUTS = ('track_of_node', 'node', 'visible', 'points', 'info', 'label')


def same(a, b):
    for k in OUTPUTS:
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True), k


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V,K,M,seed', [(2, 40, 30, 1), (5, 300, 400, 2), (32, 257, 300, 3), (8, 1000, 700, 4)])
def test_partition_equals_scipy_connected_components(V, K, M, seed):
    g = to.random_graph(V, K, M, seed)
    r = to.build_tracks(g['offsets'], g['matches'], keep=g['keep'], keypoints=g['keypoints'])
    m, view = g['matches'].astype(np.int64), to.node_views(g['offsets'], V, K)
    live = (m >= 0).all(1) & (m < K).all(1) & (g['keep'] != 0)
    live[live] = view[m[live, 0]] != view[m[live, 1]]
    assert r['info'][3] == live.sum() and 0 < live.sum() < M
    e = m[live]
    n, lab = connected_components(coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(K, K)), directed=False)
    touched = np.zeros(K, bool)
    touched[e.reshape(-1)] = True
    smallest = np.full(n, K)
    np.minimum.at(smallest, lab, np.arange(K))
    want = np.where(touched, smallest[lab], -1)
    assert np.array_equal(r['label'], want) and r['info'][4] == len(np.unique(want[touched]))


@pytest.mark.parametrize('conflict', [0, 1])
def test_outputs_do_not_depend_on_the_order_of_the_matches(conflict):
    g = to.random_graph(6, 400, 500, 7)
    kw = dict(keypoints=g['keypoints'], min_views=2, conflict=conflict)
    first = to.build_tracks(g['offsets'], g['matches'], keep=g['keep'], **kw)
    assert first['info'][1] > 10 and first['info'][5] > 0
    p = np.random.default_rng(0).permutation(g['M'])
    same(first, to.build_tracks(g['offsets'], g['matches'][p], keep=g['keep'][p], **kw))
    same(first, to.build_tracks(g['offsets'], g['matches'][:, ::-1], keep=g['keep'], **kw))
    twice = to.build_tracks(g['offsets'], np.concatenate([g['matches'], g['matches'][::-1]]), keep=np.concatenate([g['keep'], g['keep'][::-1]]),
                            cap=first['node'].shape[1], **kw)
    assert twice['info'][3] == 2 * first['info'][3]
    twice['info'][3] = first['info'][3]
    same(first, twice)


# ---- the rules on hand-made graphs ----------------------------------------------------------------------------------------
def test_a_clean_three_view_track():
    offsets = [0, 2, 4, 6]
    kp = np.arange(12.0).reshape(6, 2)
    r = to.build_tracks(offsets, [(1, 2), (2, 5)], keypoints=kp, cap=3)
    assert r['info'].tolist() == [1, 1, 3, 2, 1, 0, 0, 3] and r['track_of_node'].tolist() == [-1, 0, 0, -1, -1, 0]
    assert r['node'][:, 0].tolist() == [1, 0, 1] and r['visible'][:, 0].tolist() == [1, 1, 1] and np.array_equal(r['points'][:, 0], kp[[1, 2, 5]])
    assert (r['node'][:, 1:] == -1).all() and not r['visible'][:, 1:].any() and np.isnan(r['points'][:, 1:]).all()
    assert to.build_tracks(offsets, [(1, 2), (2, 5)], min_views=3)['info'][0] == 1
    two = to.build_tracks(offsets, [(1, 2)], min_views=3, cap=3)                      # too short: counted, not written
    assert two['info'].tolist() == [0, 0, 0, 1, 1, 0, 1, 0] and (two['track_of_node'] == -1).all()


def test_two_tracks_bridged_by_one_wrong_match():
    offsets = [0, 2, 4, 6]                                                            # tracks {0, 2, 4} and {1, 3, 5}
    good = [(0, 2), (2, 4), (1, 3), (3, 5)]
    clean = to.build_tracks(offsets, good, cap=3)
    assert clean['info'].tolist() == [2, 2, 6, 4, 2, 0, 0, 3] and clean['track_of_node'].tolist() == [0, 1, 0, 1, 0, 1]
    drop = to.build_tracks(offsets, good + [(0, 3)], conflict=0, cap=3)               # one component, every view twice
    assert drop['info'].tolist() == [0, 0, 0, 5, 1, 1, 0, 0] and (drop['track_of_node'] == -1).all()
    views = to.build_tracks(offsets, good + [(0, 3)], conflict=1, cap=3)              # every view in conflict: nothing is left
    assert views['info'].tolist() == [0, 0, 0, 5, 1, 1, 1, 0]


def test_a_view_seen_twice():
    offsets = [0, 2, 3, 4, 5]                                                         # nodes 0, 1 in view 0; 2, 3, 4 in views 1, 2, 3
    m = [(0, 2), (2, 3), (3, 4), (4, 1)]
    drop = to.build_tracks(offsets, m, conflict=0, cap=2)
    assert drop['info'].tolist() == [0, 0, 0, 4, 1, 1, 0, 0]
    views = to.build_tracks(offsets, m, conflict=1, cap=2)
    assert views['info'].tolist() == [1, 1, 3, 4, 1, 1, 0, 3] and views['track_of_node'].tolist() == [-1, -1, 0, 0, 0]
    assert views['node'][:, 0].tolist() == [-1, 0, 0, 0] and views['visible'][:, 0].tolist() == [0, 1, 1, 1]
    assert to.build_tracks(offsets, m, conflict=1, min_views=4, cap=2)['info'].tolist() == [0, 0, 0, 4, 1, 1, 1, 0]   # in both [5] and [6]


def test_a_chain_of_32_views():
    offsets, m = to.chain(32)
    for order in to.orders(m).values():
        r = to.build_tracks(offsets, order, min_views=32, cap=1)
        assert r['info'].tolist() == [1, 1, 32, 31, 1, 0, 0, 32] and (r['track_of_node'] == 0).all() and r['visible'].all()
    assert to.build_tracks(offsets, m[:-1], min_views=32, cap=1)['info'].tolist() == [0, 0, 0, 30, 1, 0, 1, 0]


def test_every_kind_of_dead_match():
    offsets = [0, 3, 6]
    dead = [(-1, 4), (0, 6), (7, 1), (1, 1), (0, 2), (4, 5)]                          # below 0, at K, above K, a = b, one view (twice)
    r = to.build_tracks(offsets, dead + [(2, 3)], keep=[1] * 6 + [0], cap=3)
    assert r['info'].tolist() == [0, 0, 0, 0, 0, 0, 0, 0] and (r['label'] == -1).all()
    r = to.build_tracks(offsets, dead + [(2, 3), (3, 2), (2, 3)], cap=3)              # repeated and reversed: each is live
    assert r['info'].tolist() == [1, 1, 2, 3, 1, 0, 0, 2] and r['label'].tolist() == [-1, -1, 2, 2, -1, -1]


def test_views_without_keypoints():
    offsets = [0, 0, 2, 2, 4, 4]                                                      # views 0, 2 and 4 are empty
    assert to.node_views(offsets, 5, 4).tolist() == [1, 1, 3, 3]
    r = to.build_tracks(offsets, [(0, 2), (1, 3), (0, 1)], cap=2)
    assert r['info'].tolist() == [2, 2, 4, 2, 2, 0, 0, 2] and r['node'].tolist() == [[-1, -1], [0, 1], [-1, -1], [0, 1], [-1, -1]]
    g = to.random_graph(6, 200, 300, 11, empty_views=(0, 3, 5))
    r = to.build_tracks(g['offsets'], g['matches'], keep=g['keep'])
    assert r['info'][1] > 5 and not r['visible'][[0, 3, 5]].any() and r['visible'][[1, 2, 4]].any()


def test_cap_at_and_around_the_count():
    g = to.random_graph(5, 300, 300, 13)
    full = to.build_tracks(g['offsets'], g['matches'], keep=g['keep'], keypoints=g['keypoints'], cap=150)
    n = int(full['info'][0])
    assert 10 < n < 149
    for cap in (0, n - 1, n, n + 1):
        r = to.build_tracks(g['offsets'], g['matches'], keep=g['keep'], keypoints=g['keypoints'], cap=cap)
        w = min(n, cap)
        assert r['info'][0] == n and r['info'][1] == w and r['node'].shape == (5, cap) and r['info'][3:7].tolist() == full['info'][3:7].tolist()
        assert np.array_equal(r['node'][:, :w], full['node'][:, :w]) and np.array_equal(r['points'][:, :w], full['points'][:, :w], equal_nan=True)
        assert np.array_equal(r['track_of_node'], np.where(full['track_of_node'] < w, full['track_of_node'], -1))
        assert r['info'][2] == r['visible'].sum() == (r['track_of_node'] >= 0).sum() and not r['visible'][:, w:].any()
        assert r['info'][7] == (r['visible'].sum(axis=0).max() if w else 0)


def test_a_table_that_decreases_still_gives_views_in_range():
    for offsets in ([0, 9, 3, 12], [5, 0, 0, 0, 12], [0, 12, 12, -4, 12]):
        V = len(offsets) - 1
        view = to.node_views(offsets, V, 12)
        assert view.min() >= 0 and view.max() < V


# ---- argument errors ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from cotr_amd.build import build_library
    build_library()
    return _lib.load_library()


def test_abi_argument_errors(lib):
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd4, odd2 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 2)
    count = ctypes.c_size_t()
    assert lib.cotr_build_tracks_work_ints(1, 0, ctypes.byref(count)) == 0 and count.value == 7 * 64       # seven regions of 256 bytes
    assert lib.cotr_build_tracks_work_ints(257, 5, ctypes.byref(count)) == 0 and count.value == 4 * 5 * 64 + 2 * 64 + 2 * 64   # touched: 512 bytes
    assert lib.cotr_build_tracks_work_ints(1 << 21, 1 << 24, ctypes.byref(count)) == 0 and count.value == (4 * 4 + 1) * (1 << 19) + (1 << 13) + 64
    for K, M in ((0, 1), ((1 << 21) + 1, 1), (4, -1), (4, (1 << 24) + 1)):
        assert lib.cotr_build_tracks_work_ints(K, M, ctypes.byref(count)) == -1
    assert lib.cotr_build_tracks_work_ints(4, 4, None) == -1

    def call(V=3, K=10, M=4, min_views=2, conflict=0, cap=5, offsets=p, matches=p, kp=p, ton=p, node=p, vis=p, pts=p, info=p, work=p):
        return lib.cotr_build_tracks(offsets, matches, None, kp, V, K, M, min_views, conflict, cap, ton, node, vis, pts, info, work, None)
    for kw, msg in ((dict(V=1), 'V must be in [2, 32]'), (dict(V=33), 'V must be'), (dict(K=0), 'K must be in [1, 2^21]'), (dict(K=(1 << 21) + 1), 'K must be'),
                    (dict(M=-1), 'M must be in [0, 2^24]'), (dict(M=(1 << 24) + 1), 'M must be'), (dict(min_views=1), 'min_views must be in [2, V]'),
                    (dict(min_views=4), 'min_views'), (dict(conflict=2), 'conflict'), (dict(conflict=-1), 'conflict'), (dict(cap=-1), 'cap must be in [0, K / 2]'),
                    (dict(cap=6), 'cap must be'), (dict(offsets=None), 'must not be NULL'), (dict(matches=None), 'must not be NULL'),
                    (dict(ton=None), 'must not be NULL'), (dict(node=None), 'must not be NULL'), (dict(vis=None), 'must not be NULL'),
                    (dict(info=None), 'must not be NULL'), (dict(work=None), 'must not be NULL'), (dict(pts=None), 'exactly when'),
                    (dict(kp=None), 'exactly when'), (dict(kp=odd4), 'aligned'), (dict(pts=odd4), 'aligned'), (dict(offsets=odd2), 'aligned'),
                    (dict(matches=odd2), 'aligned'), (dict(ton=odd2), 'aligned'), (dict(node=odd2), 'aligned'), (dict(info=odd2), 'aligned'),
                    (dict(work=odd2), 'aligned')):
        assert call(**kw) == -1 and msg in lib.cotr_raster_last_error().decode(), kw


def test_wrapper_argument_errors():
    off, m = np.array([0, 4, 8, 12]), np.array([(0, 4), (4, 8)])
    bt = tracks.build_tracks_tensors
    for args, kw, msg in (((np.array([0, 4]), m), {}, 'between 2 and 32 views'), ((np.arange(34), m), {}, 'between 2 and 32 views'),
                          ((np.array([1, 4, 8]), m), {}, 'must start at 0'), ((np.array([0, 8, 4]), m), {}, 'must not decrease'),
                          ((np.array([0, 0, 0]), m), {}, 'keypoints in all'), ((np.array([0.0, 4.0, 8.0]), m), {}, 'offsets must be integers'),
                          ((np.array([0, 1 << 21, (1 << 21) + 1]), m), {}, '2\\^21'), ((off, m[:, :1]), {}, 'matches must be'),
                          ((off, torch.zeros((2, 2))), {}, 'matches must be'),
                          ((off, m), dict(keep=[1]), 'keep must be'), ((off, m), dict(min_views=1), 'min_views'), ((off, m), dict(min_views=4), 'min_views'),
                          ((off, m), dict(min_views=2.5), 'min_views'), ((off, m), dict(conflict='merge'), 'conflict must be'), ((off, m), dict(cap=7), 'cap'),
                          ((off, m), dict(cap=-1), 'cap'), (([np.zeros((3, 3)), np.zeros((3, 2))], m), {}, r'keypoints\[0\] must be')):
        with pytest.raises(ValueError, match=msg):
            bt(*args, **kw)
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        bt(off, torch.from_numpy(m))
    kps = [np.zeros((4, 2)), np.zeros((3, 2)), np.zeros((0, 2))]
    for pm, msg in (({(0, 3): m}, 'a pair must be'), ({(1, 1): m}, 'a pair must be'), ({0: m}, 'a pair must be'), ({(0, 1): m[:, :1]}, 'must be int'),
                    ({(0, 1): np.zeros((2, 2))}, 'must be int'), ({(0, 1): np.array([(0, 3)])}, 'must index'), ({(0, 1): np.array([(-1, 0)])}, 'must index'),
                    ({(0, 2): np.array([(0, 0)])}, 'must index')):
        with pytest.raises(ValueError, match=msg):
            tracks.build_tracks(kps, pm)
    cams = np.tile([500.0, 500, 320, 240, 0], (3, 1))
    five = np.stack([np.arange(3), np.arange(3)], axis=1)
    rt = tracks.reconstruct_tracks_tensors
    for pm, kw, msg in (({(0, 1): five}, {}, 'at least one pair with 5 matches'), ({(0, 3): five}, {}, 'a pair must be')):
        with pytest.raises(ValueError, match=msg):
            rt(kps, pm, cams, **kw)
    kps = [np.zeros((6, 2))] * 3
    six = np.stack([np.arange(6), np.arange(6)], axis=1)
    for kw, msg in ((dict(bundle_rounds=-1), 'bundle_rounds'), (dict(root=3), 'root')):
        with pytest.raises(ValueError, match=msg):
            rt(kps, {(0, 1): six}, cams, **kw)
    with pytest.raises(ValueError, match='cameras must be'):
        rt(kps, {(0, 1): six}, cams[:2])
    with pytest.raises(_lib.CotrHipError, match='no CPU fallback'):
        rt([torch.zeros((6, 2))] * 3, {(0, 1): six}, cams)


# ---- the drivers' host logic ----------------------------------------------------------------------------------------------
def test_reconstruct_tracks_tensors_host_logic(monkeypatch):
    """the device calls replaced: what each is handed"""
    log = []
    dev = torch.device('cpu')
    monkeypatch.setattr(tracks._args, 'device', lambda d: dev)
    monkeypatch.setattr(torch.cuda, 'device', lambda d: contextlib.nullcontext())
    monkeypatch.setattr(tracks._args, 'no_cpu_tensors', lambda *a: None)

    def fake_pose(p1, p2, K1, K2, device=None, **kw):
        log.append(('pose', p1, p2, float(K1[0, 0]), float(K2[0, 0]), kw))
        n = len([e for e in log if e[0] == 'pose'])
        return dict(R=torch.eye(3, dtype=torch.float64) * n, mask=torch.arange(p1.shape[0]) % 2 == 0,
                    info=torch.tensor([0 if n == 2 else 1, 0, 0, 0], dtype=torch.int32))

    def fake_tracks(nodes, matches, keep=None, device=None, **kw):
        log.append(('tracks', nodes, matches, keep, kw))
        return dict(points=torch.zeros((3, 4, 2), dtype=torch.float64), visible=torch.ones((3, 4), dtype=torch.bool), info='track_info')

    def fake_tail(points, visible, rows, edges, pairs, V, root, rotation_kw, position_kw, bundle_rounds, kw, device):
        log.append(('tail', points, visible, rows, edges, pairs, V, root, rotation_kw, position_kw, bundle_rounds, kw))
        return dict(poses='poses')
    monkeypatch.setattr(essential, 'relative_pose_tensors', fake_pose)
    monkeypatch.setattr(tracks, 'build_tracks_tensors', fake_tracks)
    monkeypatch.setattr(structure, '_enqueue_view_poses', fake_tail)
    cams = np.array([[500.0, 500, 320, 240, 0], [510.0, 510, 320, 240, 0], [520.0, 520, 320, 240, 0]])
    kps = [np.arange(16.0).reshape(8, 2), 100 + np.arange(12.0).reshape(6, 2), 200 + np.arange(14.0).reshape(7, 2)]
    m01 = np.array([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (7, 0)])
    m12 = np.array([(0, 0), (1, 1), (2, 2), (3, 3), (5, 6)])
    m02 = np.array([(0, 0), (1, 1), (2, 2), (3, 3)])                                  # four matches: the pair is left out
    r = tracks.reconstruct_tracks_tensors(kps, {(0, 1): m01, (2, 1): m12[:, ::-1], (0, 2): m02}, cams, root=1, pose_kw=dict(seed=5),
                                          track_kw=dict(conflict='views', min_views=3), rotation_kw=dict(iters=3), position_kw=dict(rounds=2),
                                          bundle_rounds=1, threshold=3.0)
    assert [e[0] for e in log] == ['pose', 'pose', 'tracks', 'tail']
    assert np.array_equal(log[0][1].numpy(), kps[0][m01[:, 0]]) and np.array_equal(log[0][2].numpy(), kps[1][m01[:, 1]])
    assert np.array_equal(log[1][1].numpy(), kps[2][m12[:, 1]]) and np.array_equal(log[1][2].numpy(), kps[1][m12[:, 0]])
    assert [e[3:5] for e in log[:2]] == [(500.0, 510.0), (520.0, 510.0)] and all(e[5] == dict(refine_rounds=4, seed=5) for e in log[:2])
    _, nodes, matches, keep, kw = log[2]
    assert len(nodes) == 3 and kw == dict(conflict='views', min_views=3)
    assert matches.tolist() == [[a, 8 + b] for a, b in m01] + [[14 + b, 8 + a] for a, b in m12]
    assert keep.tolist() == [True, False, True, False, True, False] + [False] * 5   # the second pair was not found: none of its matches
    tail = log[3]
    assert tuple(tail[1].shape) == (3, 4, 2) and tail[2].all() and np.array_equal(tail[3], cams) and tail[4] == [(0, 1), (2, 1)] and len(tail[5]) == 2
    assert tail[6:] == (3, 1, dict(iters=3), dict(rounds=2), 1, dict(threshold=3.0))
    assert r['poses'] == 'poses' and r['tracks']['info'] == 'track_info'


def test_zoom_engine_reconstruct_keypoints_host_logic(monkeypatch):
    calls, mutual, got = [], [], {}

    def fake(keypoints, pair_matches, Ks, **kw):
        got.update(keypoints=keypoints, pair_matches=pair_matches, Ks=Ks, kw=kw)
        return 'result'

    def fake_mutual(corrs_a_b, corrs_b_a, kp_a, kp_b):
        mutual.append((corrs_a_b, corrs_b_a, kp_a, kp_b))
        return np.array([(len(mutual), 0)])
    monkeypatch.setattr(tracks, 'reconstruct_tracks_tensors', fake)
    monkeypatch.setattr(guided, 'mutual_matches', fake_mutual)

    class Spy(ZoomEngine):
        def __init__(self):
            pass

        def cotr_corr_multiscale(self, img_a, img_b, zoom_ins=(1.0,), converge_iters=1, max_corrs=1000, queries_a=None, force=False, **kw):
            calls.append((int(img_a[0, 0, 0]), int(img_b[0, 0, 0]), force, max_corrs, len(zoom_ins), converge_iters))
            return np.concatenate([queries_a, queries_a + 10 * img_b[0, 0, 0]], axis=1)
    imgs = [np.full((48, 64, 3), v, np.uint8) for v in range(4)]
    K = np.array([[50.0, 0, 32], [0, 50, 24], [0, 0, 1]])
    kps = [np.arange(2.0 * (5 + v)).reshape(5 + v, 2) for v in range(4)]
    assert Spy().reconstruct_keypoints(imgs, K, kps, span=2, bundle_rounds=3, root=2) == 'result'
    pairs = [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]
    assert [c[:2] for c in calls] == [p for i, j in pairs for p in ((i, j), (j, i))]
    assert all(c[2] is True and c[3] == 5 + c[0] and c[4:] == (4, 1) for c in calls)
    assert list(got['pair_matches']) == pairs and [int(m[0, 0]) for m in got['pair_matches'].values()] == [1, 2, 3, 4, 5]
    assert got['Ks'] is K and got['kw'] == dict(bundle_rounds=3, root=2) and all(np.array_equal(a, b) for a, b in zip(got['keypoints'], kps))
    ab, ba, kp_a, kp_b = mutual[1]                                                    # the pair (0, 2)
    assert np.array_equal(ab, np.concatenate([kps[0], kps[0] + 20], axis=1)) and np.array_equal(ba, np.concatenate([kps[2], kps[2]], axis=1))
    assert np.array_equal(kp_a, kps[0]) and np.array_equal(kp_b, kps[2])
    del calls[:]
    Spy().reconstruct_keypoints(imgs, K, kps, pairs=[(3, 0), (1, 2)], zoom_ins=(1.0, 0.5), converge_iters=2)
    assert [c[:2] for c in calls] == [(3, 0), (0, 3), (1, 2), (2, 1)] and all(c[4:] == (2, 2) for c in calls) and list(got['pair_matches']) == [(3, 0), (1, 2)]
    for kw, msg in ((dict(span=0), 'span'), (dict(pairs=[(0, 4)]), 'pairs must'), (dict(pairs=[(1, 1)]), 'pairs must'), (dict(pairs=[]), 'pairs must'),
                    (dict(pairs=[(0, 1), (0, 1)]), 'pairs must')):
        with pytest.raises(ValueError, match=msg):
            Spy().reconstruct_keypoints(imgs, K, kps, **kw)
    with pytest.raises(ValueError, match='between 2 and 32 images'):
        Spy().reconstruct_keypoints(imgs[:1], K, kps[:1])
    with pytest.raises(ValueError, match='one set per image'):
        Spy().reconstruct_keypoints(imgs, K, kps[:3])
