"""CPU references for the breadth-first search between two vertex sets (lpa_bfs, GraphFrame.bfs).

Two restatements of what GraphFrames 0.6.0 ``BFS.run`` computes:

literal()     the join loop itself, paths as tuples (v0, e0, v1, e1, ..., vL) of dense vertex ids
              and input edge indices.  It asserts that its own table never exceeds 1,000,000
              rows: a condition on the input, not a measurement -- use it on small graphs only.
levels_dag()  a level-synchronous numpy search from F, the stop at the first level that holds a
              vertex of T, and the backward sweep that keeps what lies on a shortest path: the
              values lpa_bfs returns (length, level, the marked edges, the summary fields that do
              not depend on the schedule, and the number of levels expanded).

Plus the graph builders of the cases (tests/test_bfs_host.py, tests/test_gpu_bfs.py).
"""
import numpy as np

LITERAL_CAP = 1_000_000


def _masks(V, m, F, T, keep):
    F = np.asarray(F, dtype=bool)
    T = np.asarray(T, dtype=bool)
    keep = np.ones(m, bool) if keep is None else np.asarray(keep, dtype=bool)
    assert F.shape == (V,) and T.shape == (V,) and keep.shape == (m,)
    return F, T, keep


def literal(V, src, dst, F, T, keep=None, max_len=10):
    """(length, sorted list of path tuples).  length 0: the common vertices as 1-tuples; -1: no
    path (or an empty set), an empty list."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    F, T, keep = _masks(V, src.size, F, T, keep)
    if not F.any() or not T.any():
        return -1, []
    both = np.flatnonzero(F & T)
    if both.size:
        return 0, [(int(v),) for v in both]
    out = {}
    for e in np.flatnonzero(keep & (src >= 0) & (src < V) & (dst >= 0) & (dst < V)):
        out.setdefault(int(src[e]), []).append((int(e), int(dst[e])))
    paths = [(int(f),) for f in np.flatnonzero(F)]
    for it in range(max_len):
        nxt = []
        for p in paths:
            seen = p[0::2]
            for e, b in out.get(p[-1], ()):
                if b == p[-1] and it == 0:   # step 0 drops self-loops ...
                    continue
                if b in seen:                # ... and a path never holds a vertex twice
                    continue
                nxt.append(p + (e, b))
        assert len(nxt) <= LITERAL_CAP, f"literal(): {len(nxt)} rows; use it on smaller inputs"
        paths = nxt
        hits = [p for p in paths if T[p[-1]]]
        if hits:
            return it + 1, sorted(hits)
        if not paths:
            break
    return -1, []


def levels_dag(V, src, dst, F, T, keep=None, max_len=10):
    """dict(length, level [V] int32, on_edge [m] bool, summary, levels): summary holds arcs,
    sources, targets, length, reached, path_vertices, path_edges; levels = the levels expanded
    (push_levels + pull_levels of the library)."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    m = src.size
    F, T, keep = _masks(V, m, F, T, keep)
    valid = keep & (src >= 0) & (src < V) & (dst >= 0) & (dst < V) & (src != dst)
    vs, vd = src[valid], dst[valid]
    summ = dict(arcs=int(np.unique(vs * max(V, 1) + vd).size), sources=int(F.sum()), targets=int(T.sum()),
                length=-1, reached=0, path_vertices=0, path_edges=0)
    level = np.full(V, -1, np.int32)
    on_edge = np.zeros(m, bool)
    res = dict(length=-1, level=level, on_edge=on_edge, summary=summ, levels=0)
    if not F.any() or not T.any():
        return res
    summ["reached"] = int(F.sum())
    if (F & T).any():
        level[F & T] = 0
        summ["length"] = res["length"] = 0
        summ["path_vertices"] = int((F & T).sum())
        return res
    lev = np.full(V, -1, np.int64)
    lev[F] = 0
    front = F.copy()
    found, reached, k = -1, 0, 0
    while True:
        reached += int(front.sum())
        if not front.any():
            break
        if (front & T).any():
            found = k
            break
        if k == max_len:
            break
        nxt = np.zeros(V, bool)
        nxt[vd[front[vs]]] = True
        nxt &= lev < 0
        k += 1
        res["levels"] = k
        lev[nxt] = k
        front = nxt
    summ["reached"] = reached
    if found < 0:
        return res
    on = (lev == found) & T
    for l in range(found - 1, -1, -1):
        step = (lev[vs] == l) & (lev[vd] == l + 1) & on[vd]
        on[vs[step]] = True
    level[:] = np.where(on, lev, -1)
    on_edge[:] = valid
    ok = on[src[valid]] & on[dst[valid]] & (lev[dst[valid]] == lev[src[valid]] + 1)
    on_edge[np.flatnonzero(valid)[~ok]] = False
    summ.update(length=found, path_vertices=int(on.sum()), path_edges=int(on_edge.sum()))
    res["length"] = found
    return res


def distances(V, src, dst, F, keep=None):
    """The full forward search: [V] int64, the distance from F over the kept non-loop edges, -1
    where there is no path (for choosing targets)."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    F, _, keep = _masks(V, src.size, F, np.zeros(V, bool), keep)
    valid = keep & (src != dst)
    vs, vd = src[valid], dst[valid]
    lev = np.full(V, -1, np.int64)
    lev[F] = 0
    front, k = F.copy(), 0
    while front.any():
        nxt = np.zeros(V, bool)
        nxt[vd[front[vs]]] = True
        nxt &= lev < 0
        k += 1
        lev[nxt] = k
        front = nxt
    return lev


def path_tuples(verts, edges):
    """enumerate_paths' two arrays as literal()'s tuples, in row order."""
    out = []
    for vr, er in zip(np.asarray(verts).tolist(), np.asarray(edges).tolist()):
        p = [vr[0]]
        for e, v in zip(er, vr[1:]):
            p += [e, v]
        out.append(tuple(p))
    return out


def one_hot(V, *ids):
    a = np.zeros(V, bool)
    a[list(ids)] = True
    return a


# ---- graph builders ----
def path(n):
    """0 -> 1 -> ... -> n - 1."""
    a = np.arange(n - 1, dtype=np.int32)
    return n, a, a + 1


def lattice(layers=4, width=3):
    """`layers` layers of `width` vertices, every vertex joined to every vertex of the next layer:
    width ** (layers - 1) paths of layers - 1 edges from ONE vertex of the first layer to the last
    layer (and as many from the first layer to one vertex of the last)."""
    s, d = [], []
    for l in range(layers - 1):
        for a in range(width):
            for b in range(width):
                s.append(l * width + a)
                d.append((l + 1) * width + b)
    return layers * width, np.array(s, np.int32), np.array(d, np.int32)


def fan(k, behind):
    """Source 0 with arcs to the k vertices 1 .. k; vertex 1 + behind has one arc on to the
    target k + 1: the source's out-list has k distinct arcs and the target sits two hops out,
    behind exactly one of them.  Returns V, src, dst, target."""
    s = np.concatenate([np.zeros(k, np.int32), np.array([1 + behind], np.int32)])
    d = np.concatenate([np.arange(1, k + 1, dtype=np.int32), np.array([k + 1], np.int32)])
    return k + 2, s, d, k + 1


def random_case(rng):
    """One case of the random family: a multigraph with V < 40 and m <= 4 V (self-loops and
    duplicates as they come), random F / T / filter, max_len 0 .. 6."""
    V = int(rng.integers(1, 40))
    m = int(rng.integers(0, 4 * V + 1))
    s = rng.integers(0, V, size=m).astype(np.int32)
    d = rng.integers(0, V, size=m).astype(np.int32)
    F = rng.random(V) < rng.choice([0.0, 0.05, 0.1, 0.3])
    T = rng.random(V) < rng.choice([0.0, 0.05, 0.1, 0.3])
    if rng.random() < 0.8 and V > 1:   # mostly: small disjoint sets, so that a search runs
        F[:] = False
        T[:] = False
        ids = rng.permutation(V)
        nf = int(rng.integers(1, 3))
        F[ids[:nf]] = True
        T[ids[nf:nf + int(rng.integers(1, 3))]] = True
    keep = None if rng.random() < 0.4 else rng.random(m) < rng.choice([0.5, 0.8, 0.95])
    return V, s, d, F, T, keep, int(rng.integers(0, 7))
