"""CPU reference for parallel personalized PageRank (the values lpa_parallel_pagerank returns).

Column l is what pr_ref describes for source = sources[l]; here every column advances at
once, as one scipy CSR product per superstep on the (V, n) matrix of all columns:

    R[v, l] = (v == sources[l]);  max_iter times  R = base + (1.0 - a) * (M @ (R * w[:, None]))
    S = R.sum(axis=0);  R /= S

with M[v, u] = the multiplicity of u -> v (multiplicity times c instead of repeated adds, the
sum in column-index order) -- independent of pr_ref.pagerank, which takes one source at a time
and sums in edge order with np.bincount.  Two implementations of these semantics differ per
entry by a relative pr_ref.bound(k, D, V) at most.
"""
import numpy as np

import pr_ref
from pr_ref import bound  # noqa: F401 -- the bound is pr_ref's


def parallel(V, src, dst, sources, k, a=0.15):
    """(ranks float64[n][V], S float64[n]) -- S the column sums before normalisation."""
    import scipy.sparse as sp

    sources = [int(x) for x in sources]
    n = len(sources)
    assert k > 0 and 0.0 <= a <= 1.0 and all(0 <= x < V for x in sources)
    s, d = pr_ref.kept(V, src, dst)
    M = sp.csr_matrix((np.ones(s.size, np.float64), (d, s)), shape=(V, V))   # duplicates summed: multiplicities
    outdeg = np.asarray(M.sum(axis=0)).ravel().astype(np.int64)
    w = np.zeros(V, np.float64)
    np.divide(1.0, outdeg, out=w, where=outdeg > 0)
    R = np.zeros((V, n), np.float64)
    base = np.zeros((V, n), np.float64)
    R[sources, np.arange(n)] = 1.0
    base[sources, np.arange(n)] = a
    for _ in range(k):
        R = base + (1.0 - a) * (M @ (R * w[:, None]))
    S = R.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        R = R / S
    return np.ascontiguousarray(R.T), S


def tournament_sources():
    """17 sources of the 1026-vertex transitive tournament: the sink 1025 and a repeat among them."""
    return [0, 1, 7, 31, 32, 33, 63, 64, 65, 500, 1023, 1024, 1025, 7, 2, 900, 1000]


def degree_mix_sources(V, s, d):
    """17 sources of degree_mix(): the vertex of the largest out-degree, the one of the largest
    in-degree and a sink among them."""
    outdeg, indeg = pr_ref.degrees(V, s, d)
    sinks = np.flatnonzero(outdeg == 0)
    assert sinks.size
    rest = np.random.default_rng(5).choice(V, size=14, replace=False)
    return [int(np.argmax(outdeg)), int(np.argmax(indeg)), int(sinks[0])] + [int(x) for x in rest]


def reachable_pairs(V, src, dst, sources, k):
    """The (source, vertex) pairs joined by a directed walk of at most k edges, the pair
    (x, x) included: with 0 < a < 1 exactly the entries with rank > 0 (the reset keeps a > 0
    at the source in every superstep, so the support after superstep j is the source plus
    the out-neighbours of the support after superstep j - 1)."""
    import scipy.sparse as sp

    s, d = pr_ref.kept(V, src, dst)
    A = sp.csr_matrix((np.ones(s.size, np.int64), (d, s)), shape=(V, V))
    A.data[:] = 1
    total = 0
    for x in sources:
        front = np.zeros(V, bool)
        front[int(x)] = True
        seen = front.copy()
        for _ in range(k):
            front = (A @ front.astype(np.int64)) > 0
            seen |= front
        total += int(seen.sum())
    return total
