"""CPU references for static PageRank (the values lpa_pagerank returns).

Spark 2.4.5 GraphX PageRank.runWithOptions, which GraphFrames 0.6.0 pageRank(maxIter=...)
calls, restated in numpy float64 on the directed multigraph as given (duplicates are edges,
a self-loop is one edge; an edge with an endpoint outside [0, V) is dropped):

    outdeg[u] = kept edges leaving u;  w[u] = 1.0 / outdeg[u]  (0.0 for a sink, never read)
    r = 1.0 everywhere; with a source, 1.0 at the source and 0.0 elsewhere
    max_iter times, all reads of the previous r:
        c[u] = r[u] * w[u]
        s[v] = sum of c[u] over the kept edges u -> v
        r[v] = a + (1.0 - a) * s[v];  with a source (v == src ? a : 0.0) + (1.0 - a) * s[v]
    S = sum r;  r *= V / S;  with a source r /= S

pagerank()      np.bincount(dst, weights=c[src]) per superstep: the sum in edge order
pagerank_csr()  independent of the first: a scipy CSR matrix M[v, u] = the multiplicity of
                u -> v, s = M @ c (multiplicity times c instead of repeated adds)
bound()         the largest relative difference of two implementations of these semantics
"""
import numpy as np

U = 2.0 ** -53


def bound(k, D, V):
    """Every term is non-negative, so a sum of n terms in any order has a relative error of at
    most about (n - 1) u; the update is linear with non-negative coefficients and does not
    grow it.  k supersteps over in-lists of at most D entries, then the sum over V ranks."""
    return 2 * (k * (D + 2) + V + 2) * U


def kept(V, src, dst):
    """The kept edges as int64 (s, d), in input order."""
    s = np.asarray(src).astype(np.int64)
    d = np.asarray(dst).astype(np.int64)
    ok = (s >= 0) & (s < V) & (d >= 0) & (d < V)
    return s[ok], d[ok]


def degrees(V, src, dst):
    """(out_degree int64[V], in_degree int64[V]) with multiplicity."""
    s, d = kept(V, src, dst)
    return np.bincount(s, minlength=V).astype(np.int64), np.bincount(d, minlength=V).astype(np.int64)


def _weights(outdeg):
    w = np.zeros(outdeg.size, np.float64)
    np.divide(1.0, outdeg, out=w, where=outdeg > 0)
    return w


def _run(V, w, gather, max_iter, a, source):
    """(normalised rank, S) with s = gather(c)."""
    assert max_iter > 0 and 0.0 <= a <= 1.0 and (source is None or 0 <= source < V)
    if source is None:
        r = np.ones(V, np.float64)
        base = np.full(V, a, np.float64)
    else:
        r = np.zeros(V, np.float64)
        r[source] = 1.0
        base = np.zeros(V, np.float64)
        base[source] = a
    for _ in range(max_iter):
        c = r * w
        r = base + (1.0 - a) * gather(c)
    S = float(r.sum()) if V else 0.0
    if V:
        r = r / S if source is not None else r * (float(V) / S)
    return r, S


def pagerank(V, src, dst, max_iter, reset_prob=0.15, source=None):
    """(rank float64[V], out_degree, in_degree, S) -- S the rank sum before normalisation."""
    s, d = kept(V, src, dst)
    outdeg, indeg = degrees(V, src, dst)
    rank, S = _run(V, _weights(outdeg), lambda c: np.bincount(d, weights=c[s], minlength=V), max_iter,
                   float(reset_prob), source)
    return rank, outdeg, indeg, S


def pagerank_csr(V, src, dst, max_iter, reset_prob=0.15, source=None):
    """The same four values from a scipy CSR product."""
    import scipy.sparse as sp

    s, d = kept(V, src, dst)
    M = sp.csr_matrix((np.ones(s.size, np.float64), (d, s)), shape=(V, V))   # duplicates summed: multiplicities
    outdeg = np.asarray(M.sum(axis=0)).ravel().astype(np.int64)
    indeg = np.asarray(M.sum(axis=1)).ravel().astype(np.int64)
    rank, S = _run(V, _weights(outdeg), lambda c: M @ c, max_iter, float(reset_prob), source)
    return rank, outdeg, indeg, S


def summary(rank, outdeg, indeg, S):
    """The dict of lpa_pagerank_summary from numpy."""
    V = rank.size
    top = float(rank.max()) if V else 0.0
    return dict(rank_sum=float(S), max_rank=top, max_rank_id=int(np.flatnonzero(rank == top)[0]) if V else -1,
                edges=int(outdeg.sum()), sinks=int((outdeg == 0).sum()), max_in_degree=int(indeg.max()) if V else 0)
