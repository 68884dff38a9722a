"""CPU restatements of lpa_core_numbers (include/lpa.h): the core numbers of the canonical
simple undirected graph of a multigraph (self-loops dropped, direction ignored, duplicates
collapsed, an edge with an end outside [0, V) is no edge).

core_numbers          a vectorised numpy peel, level by level and sub-level by sub-level
core_numbers_literal  an independent restatement with no peeling in it: the h-index fixpoint
                      (Lu, Zhou, Zhang, Stanley 2016): from c = the degrees, c[v] <- H of its
                      neighbours' c, until nothing changes
summary               the summary fields that are functions of the graph (not `passes`)
"""
import numpy as np

SUMMARY_KEYS = ("degeneracy", "main_core_size", "levels", "simple_edges", "max_degree", "n_core0", "passes")
PURE_KEYS = SUMMARY_KEYS[:-1]


def simple_graph(V, s, d):
    """(off, col, deg) of the canonical simple undirected graph: both directions of every simple
    edge, rows ascending; deg int32."""
    s = np.asarray(s, dtype=np.int64)
    d = np.asarray(d, dtype=np.int64)
    ok = (s >= 0) & (s < V) & (d >= 0) & (d < V) & (s != d)
    lo, hi = np.minimum(s[ok], d[ok]), np.maximum(s[ok], d[ok])
    key = np.unique(lo * max(V, 1) + hi)
    a, b = key // max(V, 1), key % max(V, 1)
    frm = np.concatenate([a, b])
    to = np.concatenate([b, a])
    order = np.lexsort((to, frm))
    col = to[order].astype(np.int64)
    deg = np.bincount(frm, minlength=V).astype(np.int64) if V else np.zeros(0, np.int64)
    off = np.zeros(V + 1, np.int64)
    np.cumsum(deg, out=off[1:])
    return off, col, deg.astype(np.int32)


def _gather(off, col, rows):
    """The concatenated neighbour lists of rows."""
    lens = off[rows + 1] - off[rows]
    total = int(lens.sum())
    if total == 0:
        return np.empty(0, np.int64)
    starts = np.repeat(off[rows] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
    return col[starts + np.arange(total)]


def _check_cap(max_k):
    if max_k is not None:
        if not isinstance(max_k, (int, np.integer)) or isinstance(max_k, (bool, np.bool_)):
            raise TypeError("max_k must be an int or None")
        if max_k < 0:
            raise ValueError("max_k must not be negative")


def core_numbers(V, s, d, max_k=None):
    """(core int32 [V], simple_degree int32 [V]); with max_k, min(core, max_k), the peeling
    stopped before level max_k."""
    _check_cap(max_k)
    off, col, deg0 = simple_graph(V, s, d)
    deg = deg0.astype(np.int64)
    core = np.zeros(V, np.int32)
    alive = np.ones(V, bool)
    left = V
    while left:
        live = np.flatnonzero(alive)
        k = int(deg[live].min())
        if max_k is not None and k >= max_k:
            core[live] = max_k
            break
        front = live[deg[live] <= k]
        while front.size:
            core[front] = k
            alive[front] = False
            left -= front.size
            nb = _gather(off, col, front)
            nb = nb[alive[nb]]
            if nb.size == 0:
                break
            cand, dec = np.unique(nb, return_counts=True)
            deg[cand] -= dec
            front = cand[deg[cand] <= k]
    return core, deg0


def _h_index(vals):
    """The largest h such that at least h of vals are >= h."""
    h = 0
    for i, x in enumerate(sorted(vals, reverse=True)):
        if x >= i + 1:
            h = i + 1
        else:
            break
    return h


def core_numbers_literal(V, s, d, max_k=None):
    """The same pair by the h-index fixpoint, vertex by vertex in plain Python."""
    _check_cap(max_k)
    off, col, deg0 = simple_graph(V, s, d)
    c = [int(x) for x in deg0]
    nbrs = [col[off[v]:off[v + 1]].tolist() for v in range(V)]
    changed = True
    while changed:
        changed = False
        for v in range(V):
            h = _h_index([c[w] for w in nbrs[v]])
            if h < c[v]:
                c[v] = h
                changed = True
    core = np.array(c, dtype=np.int32).reshape(V)
    if max_k is not None:
        core = np.minimum(core, max_k).astype(np.int32)
    return core, deg0


def summary_of(core, deg, max_k=None):
    """The pure summary fields from the UNCAPPED core numbers and the simple degrees."""
    V = int(core.size)
    if V == 0:
        return dict.fromkeys(PURE_KEYS, 0)
    capped = core if max_k is None else np.minimum(core, max_k)
    top = int(capped.max())
    if max_k is None:
        levels = int(np.unique(core).size)
    else:
        levels = int(np.unique(core[core < max_k]).size) + int((core >= max_k).any())
    return dict(degeneracy=top, main_core_size=int((capped == top).sum()), levels=levels,
                simple_edges=int(deg.astype(np.int64).sum() // 2), max_degree=int(deg.max()),
                n_core0=int((deg == 0).sum()))


def summary(V, s, d, max_k=None):
    core, deg = core_numbers(V, s, d)
    return summary_of(core, deg, max_k)


# ---- the shapes of the closed forms ----
def _i32(s, d):
    return np.asarray(s, dtype=np.int32), np.asarray(d, dtype=np.int32)


def clique(n, first=0):
    iu, ju = np.triu_indices(n, 1)
    return _i32(iu + first, ju + first)


def path(n):
    return (n,) + _i32(np.arange(n - 1), np.arange(1, n))


def complete_bipartite(a, b):
    """K_{a,b}: vertices 0 .. a - 1 against a .. a + b - 1."""
    return (a + b,) + _i32(np.repeat(np.arange(a), b), np.tile(a + np.arange(b), a))


def clique_with_leaves(n=40, leaves=100):
    """K_n, every member with `leaves` pendant leaves of its own."""
    s, d = clique(n)
    ls = np.repeat(np.arange(n), leaves)
    ld = n + np.arange(n * leaves)
    return (n + n * leaves,) + _i32(np.concatenate([s, ls]), np.concatenate([d, ld]))


def overshoot(leaves=50):
    """Vertex 0 with `leaves` leaves and one edge into the triangle {1, 2, 3}: at level 1 its count
    falls from leaves + 1 to 1 in one sub-level."""
    s = np.concatenate([[1, 2, 3, 0], np.zeros(leaves, np.int64)])
    d = np.concatenate([[2, 3, 1, 1], 4 + np.arange(leaves)])
    return (4 + leaves,) + _i32(s, d)


def clique_chain(lo=3, hi=12):
    """K_lo .. K_hi, the last vertex of each joined to the first of the next by one edge."""
    ss, dd, first, last = [], [], 0, None
    for n in range(lo, hi + 1):
        s, d = clique(n, first)
        ss.append(s)
        dd.append(d)
        if last is not None:
            ss.append(np.array([last]))
            dd.append(np.array([first]))
        last = first + n - 1
        first += n
    return (first,) + _i32(np.concatenate(ss), np.concatenate(dd))


def grid(r, c):
    idx = np.arange(r * c).reshape(r, c)
    s = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    d = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return (r * c,) + _i32(s, d)


def circulant(n, steps=(1, 2)):
    i = np.arange(n)
    return (n,) + _i32(np.concatenate([i] * len(steps)), np.concatenate([(i + t) % n for t in steps]))


def binary_tree(n):
    """Complete binary tree on n vertices: v's parent is (v - 1) // 2."""
    v = np.arange(1, n)
    return (n,) + _i32((v - 1) // 2, v)
