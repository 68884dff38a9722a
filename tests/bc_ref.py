"""CPU references of the betweenness centrality (lpa_betweenness), over dense ids.

Two independent ones: ``brandes`` is Brandes' algorithm written out in plain Python from the
definition in include/lpa.h (it also returns the integers of the summary and the numbers the
tests' error bound needs); ``networkx_bc`` hands the distinct non-loop arcs to networkx.  The
fixtures the tests share are here too."""
import numpy as np


def simple_arcs(V, src, dst, directed=True):
    """The distinct arcs src -> dst with src != dst and both ends in [0, V), as a sorted list of
    pairs; both orientations of every one of them when not directed."""
    arcs = set()
    for a, b in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        if a != b and 0 <= a < V and 0 <= b < V:
            arcs.add((a, b))
            if not directed:
                arcs.add((b, a))
    return sorted(arcs)


def brandes(V, src, dst, sources=None, directed=True):
    """Unscaled betweenness from ``sources`` (None: every vertex): a dict of
    raw        float64 [V]: sum over the sources s != v of delta_s(v)
    max_depth  largest level of any source (-1 without a source or a vertex)
    reached    sum over the sources of the vertices given a level, the source included
    arcs       distinct non-loop arcs walked (both orientations when not directed)
    max_list   the longest out-list or in-list
    Sums are taken in ascending neighbour order, sigma is a Python float (binary64)."""
    arcs = simple_arcs(V, src, dst, directed)
    out = [[] for _ in range(V)]
    indeg = [0] * V
    for a, b in arcs:
        out[a].append(b)
        indeg[b] += 1
    srcs = list(range(V)) if sources is None else [int(x) for x in sources]
    raw = [0.0] * V
    max_depth, reached = -1, 0
    for s in srcs:
        level = [-1] * V
        sigma = [0.0] * V
        level[s], sigma[s] = 0, 1.0
        order, frontier = [s], [s]
        while frontier:
            nxt = []
            for u in frontier:
                for w in out[u]:
                    if level[w] < 0:
                        level[w] = level[u] + 1
                        nxt.append(w)
                    if level[w] == level[u] + 1:
                        sigma[w] += sigma[u]
            order.extend(nxt)
            frontier = nxt
        reached += len(order)
        max_depth = max(max_depth, level[order[-1]])
        delta = [0.0] * V
        for v in reversed(order):
            acc = 0.0
            for w in out[v]:
                if level[w] == level[v] + 1:
                    acc += sigma[v] / sigma[w] * (1.0 + delta[w])
            delta[v] = acc
            if v != s:
                raw[v] += acc
    max_list = max([len(x) for x in out] + indeg + [0])
    return dict(raw=np.asarray(raw, dtype=np.float64), max_depth=max_depth, reached=reached, arcs=len(arcs),
                max_list=max_list)


def networkx_bc(V, src, dst, directed=True, normalized=True):
    """networkx.betweenness_centrality of the DiGraph (Graph when not directed) of the distinct
    non-loop arcs over the vertices 0 ... V - 1, as float64 [V]."""
    import networkx as nx

    G = nx.DiGraph() if directed else nx.Graph()
    G.add_nodes_from(range(V))
    G.add_edges_from(simple_arcs(V, src, dst, True))
    bc = nx.betweenness_centrality(G, normalized=normalized)
    return np.asarray([bc[v] for v in range(V)], dtype=np.float64)


def scale(raw, V, n_sources, directed=True, normalized=True):
    """The table of include/lpa.h / GraphFrame.betweennessCentrality, in binary64."""
    raw = np.asarray(raw, dtype=np.float64)
    if normalized:
        return raw * (V / n_sources) / ((V - 1) * (V - 2)) if V > 2 else np.zeros(V, np.float64)
    x = raw * (V / n_sources)
    return x if directed else x / 2


def pivots(V, k, seed):
    """The documented draw of betweennessCentrality(k=..., seed=...)."""
    return np.sort(np.random.default_rng(seed).choice(V, size=k, replace=False))


# ---- fixtures ----
def path(n):
    """0 -> 1 -> ... -> n - 1: raw[i] = i (n - 1 - i) with every vertex a source."""
    a = np.arange(n - 1, dtype=np.int32)
    return n, a, a + 1


def diamond_chain(stages):
    """`stages` triple diamonds in a row: joint j -> three middles -> joint j + 1.  4 stages + 1
    vertices, depth 2 stages and sigma = 3^stages at the last joint."""
    s, d = [], []
    for j in range(stages):
        a, b = 4 * j, 4 * j + 4
        for k in (1, 2, 3):
            s += [a, a + k]
            d += [a + k, b]
    return 4 * stages + 1, np.asarray(s, np.int32), np.asarray(d, np.int32)


def form_stars(lengths=(0, 1, 8, 9, 32, 33, 1024, 1025)):
    """For every L of `lengths` one centre with L out-arcs and one with L in-arcs, all to leaves
    of one shared pool (so the pool's vertices have short lists of several lengths too), plus
    the arcs in-centre i -> out-centre i + 1, which close a ring without touching an out-centre's
    out-list or an in-centre's in-list.  Returns V, src, dst, centres (out-centres first)."""
    pool = max(lengths) + 7
    n = len(lengths)
    centres = np.arange(2 * n, dtype=np.int32)
    leaf0 = 2 * n
    s, d = [], []
    for i, L in enumerate(lengths):
        leaves = leaf0 + (np.arange(L) + 5 * i) % pool
        s += [np.full(L, i), leaves]                # out-star i
        d += [leaves, np.full(L, n + i)]            # in-star n + i
    s.append(centres[n:])
    d.append(np.roll(centres[:n], -1))
    return 2 * n + pool, np.concatenate(s).astype(np.int32), np.concatenate(d).astype(np.int32), centres
