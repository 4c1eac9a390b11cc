"""A numpy / Python restatement of the rules of cotr_build_tracks (include/cotr_hip.h): sequential union-find
over the live matches, then one pass over the components in ascending label.  Written from the rules, not from the kernels:
nothing here runs in parallel, and no order of the matches matters to it.  Also the graphs the tests share."""
import numpy as np


def node_views(offsets, V, K):
    """the view of nodes 0 .. K - 1: the rule's binary search over entries 1 .. V - 1 (the largest v with offsets[v] <= g for a
    table that does not decrease)"""
    offsets = np.asarray(offsets, np.int64)
    g = np.arange(K, dtype=np.int64)
    lo, hi = np.zeros(K, np.int64), np.full(K, V, np.int64)
    while ((hi - lo) > 1).any():
        go = (hi - lo) > 1
        mid = (lo + hi) >> 1
        left = go & (offsets[np.minimum(mid, V)] <= g)
        lo = np.where(left, mid, lo)
        hi = np.where(go & ~left, mid, hi)
    return lo


def build_tracks(offsets, matches, keep=None, keypoints=None, min_views=2, conflict=0, cap=None, K=None):
    """-> dict: track_of_node [K], node [V,cap], visible uint8 [V,cap], points [V,cap,2] or None, info int32 [8], label [K]
    (the component's smallest node, -1 for an untouched node).  conflict: 0 'drop', 1 'views'."""
    offsets = np.asarray(offsets, np.int64)
    V = len(offsets) - 1
    K = int(offsets[V]) if K is None else int(K)
    m = np.asarray(matches, np.int64).reshape(-1, 2)
    M = m.shape[0]
    cap = min(K // 2, M) if cap is None else int(cap)
    view = node_views(offsets, V, K)
    live = (m >= 0).all(axis=1) & (m < K).all(axis=1)
    if keep is not None:
        live &= np.asarray(keep).reshape(-1) != 0
    idx = np.nonzero(live)[0]
    live[idx] = view[m[idx, 0]] != view[m[idx, 1]]
    parent = list(range(K))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    touched = np.zeros(K, bool)
    for a, b in m[live].tolist():
        touched[a] = touched[b] = True
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    label = np.full(K, -1, np.int64)
    nodes = np.nonzero(touched)[0]
    label[nodes] = [find(int(g)) for g in nodes]
    track_of_node = np.full(K, -1, np.int32)
    node = np.full((V, cap), -1, np.int32)
    visible = np.zeros((V, cap), np.uint8)
    points = None if keypoints is None else np.full((V, cap, 2), np.nan)
    found = obs = comps = conflicted = short = longest = 0
    order = nodes[np.argsort(label[nodes], kind='stable')]
    starts = np.nonzero(np.diff(label[order], prepend=-2))[0]
    for members in np.split(order, starts[1:]) if len(order) else []:
        counts = np.bincount(view[members], minlength=V)
        seen, conf = counts > 0, counts > 1
        comps += 1
        conflicted += bool(conf.any())
        if conflict == 0 and conf.any():
            continue
        left = seen & ~conf if conflict else seen
        if left.sum() < min_views:
            short += 1
            continue
        t, found = found, found + 1
        if t >= cap:
            continue
        longest = max(longest, int(left.sum()))
        for g in members:
            v = view[g]
            if not left[v]:
                continue
            track_of_node[g], node[v, t], visible[v, t] = t, g - offsets[v], 1
            if points is not None:
                points[v, t] = keypoints[g]
            obs += 1
    info = np.array([found, min(found, cap), obs, int(live.sum()), comps, conflicted, short, longest], np.int32)
    return dict(track_of_node=track_of_node, node=node, visible=visible, points=points, info=info, label=label)


# ---- graphs ---------------------------------------------------------------------------------------------------------------
def even_offsets(V, K):
    """K nodes over V views as evenly as they go (the first K mod V views one more)"""
    sizes = np.full(V, K // V) + (np.arange(V) < K % V)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def random_graph(V, K, M, seed, empty_views=(), bad=0.05, near=0.6):
    """offsets (the views of ``empty_views`` without keypoints), matches [M,2] (a share ``near`` between keypoints of the same
    local index in two views, so that long clean tracks exist; a share ``bad`` dead in every way), keep [M], keypoints [K,2]"""
    rng = np.random.default_rng(seed)
    full = [v for v in range(V) if v not in empty_views]
    sizes = np.zeros(V, np.int64)
    sizes[full] = np.full(len(full), K // len(full)) + (np.arange(len(full)) < K % len(full))
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    m = rng.integers(0, K, size=(M, 2))
    sel = np.nonzero(rng.random(M) < near)[0]
    va, vb = rng.choice(full, len(sel)), rng.choice(full, len(sel))
    i = (rng.random(len(sel)) * np.minimum(sizes[va], sizes[vb])).astype(np.int64)
    m[sel, 0], m[sel, 1] = offsets[va] + i, offsets[vb] + i
    kinds = rng.random(M)
    m[kinds < bad / 4, 0] = -1 - rng.integers(0, 5)
    m[(kinds >= bad / 4) & (kinds < bad / 2), 1] = K + rng.integers(0, 5)
    same = (kinds >= bad / 2) & (kinds < 3 * bad / 4)
    m[same, 1] = m[same, 0]
    keep = (rng.random(M) >= 0.1).astype(np.uint8)
    return dict(offsets=offsets, matches=m.astype(np.int32), keep=keep, keypoints=rng.normal(size=(K, 2)) * 100, V=V, K=K, M=M)


def orders(matches, seed=0):
    """the same matches ascending, descending and shuffled"""
    m = np.asarray(matches)
    return dict(ascending=m, descending=m[::-1].copy(), shuffled=m[np.random.default_rng(seed).permutation(len(m))])


def chain(V):
    """one node per view, node v matched to node v + 1"""
    return np.arange(V + 1, dtype=np.int32), np.stack([np.arange(V - 1), np.arange(1, V)], axis=1).astype(np.int32)


def star(V, per_view):
    """``per_view`` nodes in each of V views; node i of view 0 matched to node i of every other view"""
    offsets = (np.arange(V + 1) * per_view).astype(np.int32)
    m = [(i, v * per_view + i) for v in range(1, V) for i in range(per_view)]
    return offsets, np.array(m, np.int32)


def zigzag(n):
    """a path of n nodes alternating between two views of n / 2 nodes each: one deep component, both views in conflict"""
    h = n // 2
    path = np.stack([np.arange(h), h + np.arange(h)], axis=1).reshape(-1)    # 0, h, 1, h + 1, ...
    return np.array([0, h, n], np.int32), np.stack([path[:-1], path[1:]], axis=1).astype(np.int32)


def joined_paths(n):
    """two paths of n nodes over 4 views (views 0-1 and 2-3 alternating), joined by one match between their far ends"""
    h = n // 2
    offsets = np.array([0, h, 2 * h, 3 * h, 4 * h], np.int32)
    pa = np.stack([np.arange(h), h + np.arange(h)], axis=1).reshape(-1)
    pb = 2 * h + pa
    m = np.concatenate([np.stack([pa[:-1], pa[1:]], axis=1), np.stack([pb[:-1], pb[1:]], axis=1), [[pa[-1], pb[-1]]]])
    return offsets, m.astype(np.int32)
