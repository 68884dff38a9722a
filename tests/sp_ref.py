"""CPU references for landmark shortest paths (the values lpa_shortest_paths returns).

GraphX lib.ShortestPaths, which GraphFrames 0.6.0 shortestPaths(landmarks) calls, restated
on dense ids: dist[l, v] = the number of edges on a shortest directed path from v to
landmarks[l] along src -> dst (GraphX sends its messages from dst to src, so distances are
TO the landmark), 0 at the landmark, -1 where there is no path.  Duplicate edges and
self-loops change nothing; an edge with an endpoint outside [0, V) is dropped.

shortest_paths()      a level-synchronous numpy BFS per landmark over the reversed,
                      deduplicated arc set
shortest_paths_csr()  independent of the first: scipy.sparse.csgraph.shortest_path
                      (unweighted) on the reversed PATTERN matrix, built from np.unique of
                      the arc keys (summing duplicates into a small integer type overflows)
summary()             the integers of lpa_sp_summary that do not depend on the schedule,
                      and `levels`, what push_levels + pull_levels must add up to
"""
import numpy as np


def arcs(V, src, dst):
    """The distinct in-range non-loop arcs as int64 (s, d), ascending by (s, d)."""
    s = np.asarray(src).astype(np.int64)
    d = np.asarray(dst).astype(np.int64)
    ok = (s >= 0) & (s < V) & (d >= 0) & (d < V) & (s != d)
    key = np.unique(s[ok] * max(V, 1) + d[ok])
    return key // max(V, 1), key % max(V, 1)


def shortest_paths(V, src, dst, landmarks):
    """int32 [len(landmarks), V]: a BFS per landmark along the reversed arcs."""
    s, d = arcs(V, src, dst)
    order = np.argsort(d, kind="stable")     # in-lists: the predecessors of every vertex
    pred = s[order]
    off = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(d, minlength=V), out=off[1:])
    lms = [int(l) for l in landmarks]
    out = np.full((len(lms), V), -1, np.int32)
    for row, l in enumerate(lms):
        assert 0 <= l < V
        dist = out[row]
        dist[l] = 0
        front = np.array([l], np.int64)
        level = 0
        while front.size:
            level += 1
            lo, hi = off[front], off[front + 1]
            n = hi - lo
            idx = np.repeat(lo - np.concatenate(([0], np.cumsum(n)[:-1])), n) + np.arange(int(n.sum()))
            cand = np.unique(pred[idx])
            front = cand[dist[cand] < 0]
            dist[front] = level
    return out


def shortest_paths_csr(V, src, dst, landmarks):
    """The same array from scipy's unweighted shortest_path on the reversed pattern matrix."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import shortest_path

    lms = np.asarray([int(l) for l in landmarks], dtype=np.int64)
    if lms.size == 0 or V == 0:
        return np.full((lms.size, V), -1, np.int32)
    s, d = arcs(V, src, dst)
    M = sp.csr_matrix((np.ones(s.size, np.float64), (d, s)), shape=(V, V))   # reversed: d -> s
    uniq, inv = np.unique(lms, return_inverse=True)
    D = np.atleast_2d(shortest_path(M, method="D", directed=True, unweighted=True, indices=uniq))
    out = np.where(np.isfinite(D), D, -1.0).astype(np.int32)
    return out[inv]


def summary(V, src, dst, dist):
    """dict of the schedule-independent fields of lpa_sp_summary, plus `levels`: the sum over
    the batches of 64 landmarks of (the batch's largest distance + 1) = push_levels + pull_levels."""
    n = dist.shape[0]
    s, _ = arcs(V, src, dst)
    levels = 0
    for b in range(0, n, 64):
        rows = dist[b:b + 64]
        if rows.size:
            levels += int(rows.max()) + 1
    return dict(arcs=int(s.size), reached=int((dist >= 0).sum()),
                max_distance=int(dist.max()) if dist.size else -1, batches=(n + 63) // 64, levels=levels)


# ---- graphs ----
def path(n):
    """i -> i + 1 on n vertices."""
    i = np.arange(n - 1, dtype=np.int32)
    return n, i, i + 1


def cycle(n):
    i = np.arange(n, dtype=np.int32)
    return n, i, ((i + 1) % n).astype(np.int32)


def evenly_spaced(V, k):
    """k landmarks V // k apart, from vertex 0."""
    return (np.arange(k) * (V // k)).astype(np.int32)


def top_in_degree(V, src, dst, k):
    """The k vertices of largest in-degree (with multiplicity), ties by the smaller id."""
    s = np.asarray(src).astype(np.int64)
    d = np.asarray(dst).astype(np.int64)
    ok = (s >= 0) & (s < V) & (d >= 0) & (d < V)
    indeg = np.bincount(d[ok], minlength=V)
    return np.lexsort((np.arange(V), -indeg))[:k].astype(np.int32)
