"""CPU references for triangle counting (the values lpa_triangle_count returns).

Counting runs on the canonical simple undirected graph of the multigraph: self-loops
dropped, direction ignored, duplicates collapsed.  count[v] = the triangles (unordered
vertex triples, pairwise adjacent) that contain v; simple_degree[v] = v's distinct
neighbours.

triangles()          scipy: A = symmetrised 0/1 adjacency without the diagonal,
                     count = rowsum((A @ A) o A) // 2  (in row blocks, to bound memory)
triangles_oriented() numpy only, independent of the first: the simple edges oriented by
                     (degree, id), np.intersect1d of the two out-lists of every edge"""
import numpy as np


def simple_edges(V, src, dst):
    """The distinct undirected non-loop edges as (a, b), a < b, in ascending (a, b) order."""
    s = np.asarray(src).astype(np.int64)
    d = np.asarray(dst).astype(np.int64)
    lo, hi = np.minimum(s, d), np.maximum(s, d)
    keep = lo != hi
    key = np.unique(lo[keep] * max(V, 1) + hi[keep])
    return key // max(V, 1), key % max(V, 1)


def triangles(V, src, dst, block_work=20_000_000, progress=None):
    """(count int64[V], simple_degree int64[V]) by sparse matrix products.  progress
    (optional) is called with (rows done, V) after every row block."""
    import scipy.sparse as sp

    a, b = simple_edges(V, src, dst)
    if V == 0 or a.size == 0:
        return np.zeros(V, np.int64), np.zeros(V, np.int64)
    one = np.ones(2 * a.size, np.int64)
    A = sp.csr_matrix((one, (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(V, V))
    deg = np.asarray(A.sum(axis=1)).ravel().astype(np.int64)
    # row blocks of about block_work multiply-adds each (row v costs sum of d over N(v))
    work = np.cumsum(np.asarray(A @ deg).ravel())
    count = np.zeros(V, np.int64)
    r0 = 0
    while r0 < V:
        r1 = int(np.searchsorted(work, (work[r0 - 1] if r0 else 0) + block_work, side="right"))
        r1 = min(max(r1, r0 + 1), V)
        blk = A[r0:r1]
        count[r0:r1] = np.asarray((blk @ A).multiply(blk).sum(axis=1)).ravel() // 2
        r0 = r1
        if progress is not None:
            progress(r0, V)
    return count, deg


def triangles_oriented(V, src, dst):
    """The same pair from oriented out-lists: every simple edge points from its endpoint of
    lower (degree, id) to the higher; for each oriented edge u -> v, every w in both
    out-lists closes one triangle {u, v, w}, met at no other edge."""
    a, b = simple_edges(V, src, dst)
    deg = np.bincount(a, minlength=V) + np.bincount(b, minlength=V)
    deg = deg.astype(np.int64)
    count = np.zeros(V, np.int64)
    fwd = (deg[a] < deg[b]) | ((deg[a] == deg[b]) & (a < b))
    frm, to = np.where(fwd, a, b), np.where(fwd, b, a)
    order = np.lexsort((to, frm))
    frm, to = frm[order], to[order]
    start = np.searchsorted(frm, np.arange(V + 1))
    for u, v in zip(frm.tolist(), to.tolist()):
        w = np.intersect1d(to[start[u]:start[u + 1]], to[start[v]:start[v + 1]], assume_unique=True)
        if w.size:
            count[u] += w.size
            count[v] += w.size
            count[w] += 1
    return count, deg


def summary(count, deg):
    """The dict of lpa_triangle_summary from numpy."""
    V = count.size
    top = int(count.max()) if V else 0
    return dict(n_triangles=int(count.sum()) // 3, simple_edges=int(deg.sum()) // 2,
                wedges=int((deg * (deg - 1) // 2).sum()), n_in_triangle=int((count > 0).sum()),
                max_count=top, max_count_id=int(np.flatnonzero(count == top)[0]) if V else -1)
