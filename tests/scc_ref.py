"""CPU references for strongly connected components (the values
lpa_strongly_connected_components returns).

GraphX lib.StronglyConnectedComponents.run, which GraphFrames 0.6.0
stronglyConnectedComponents(maxIter) calls, restated on dense ids.  Duplicate edges change
nothing; an edge with an endpoint outside [0, V) is dropped; a self-loop is kept as a fact
about its vertex (it is never trimmed).

scc_rounds()   the rounds themselves in numpy (write, trim to the fixpoint, and -- only if
               rounds < max_iter -- colour and mark), so that a call stopped early by
               max_iter can be compared too; returns comp and the summary dict
scc_tarjan()   independent of the first: an iterative Tarjan, the smallest member per SCC
"""
import numpy as np

CONVERGE = 2 ** 31 - 1   # what Graph.strongly_connected_components(max_iter=None) passes


def arcs_and_loops(V, src, dst):
    """The distinct in-range non-loop arcs as int64 (s, d), and loop[v] (bool)."""
    s = np.asarray(src).astype(np.int64)
    d = np.asarray(dst).astype(np.int64)
    ok = (s >= 0) & (s < V) & (d >= 0) & (d < V)
    s, d = s[ok], d[ok]
    loop = np.zeros(V, bool)
    loop[s[s == d]] = True
    ne = s != d
    key = np.unique(s[ne] * max(V, 1) + d[ne])
    return key // max(V, 1), key % max(V, 1), loop


def summary_of(comp, rounds, trimmed, unresolved):
    V = comp.size
    if V == 0:
        return dict(n_components=0, n_singletons=0, largest_size=0, largest_id=-1, rounds=int(rounds),
                    trimmed=int(trimmed), unresolved=int(unresolved))
    size = np.bincount(comp, minlength=V)
    return dict(n_components=int((size > 0).sum()), n_singletons=int((size == 1).sum()),
                largest_size=int(size.max()), largest_id=int(np.argmax(size)),   # argmax: the first maximum
                rounds=int(rounds), trimmed=int(trimmed), unresolved=int(unresolved))


def scc_rounds(V, src, dst, max_iter=CONVERGE):
    """(comp int32 [V], summary dict) after at most max_iter rounds."""
    assert max_iter > 0
    s, d, loop = arcs_and_loops(V, src, dst)
    ids = np.arange(V, dtype=np.int64)
    comp = ids.copy()
    colour = ids.copy()
    alive = np.ones(V, bool)
    marked = np.zeros(V, bool)
    rounds = trimmed = 0
    while alive.any() and rounds < max_iter:
        rounds += 1
        # 1. write
        comp[marked] = colour[marked]
        alive[marked] = False
        marked[:] = False
        # 2. trim to the fixpoint
        while True:
            live = alive[s] & alive[d]
            has_out = np.bincount(s[live], minlength=V) > 0
            has_in = np.bincount(d[live], minlength=V) > 0
            gone = alive & ~loop & ~(has_out & has_in)
            if not gone.any():
                break
            alive[gone] = False
            trimmed += int(gone.sum())
        if rounds >= max_iter:
            break
        # 3. colour: the smallest alive ancestor, by repeated minimum along the alive arcs
        live = alive[s] & alive[d]
        ls, ld = s[live], d[live]
        colour = ids.copy()
        while True:
            new = colour.copy()
            np.minimum.at(new, ld, colour[ls])
            if np.array_equal(new, colour):
                break
            colour = new
        # ... and mark: the roots, and whoever reaches one along arcs inside one colour
        marked = alive & (colour == ids)
        same = colour[ls] == colour[ld]
        bs, bd = ls[same], ld[same]
        while True:
            add = np.zeros(V, bool)
            add[bs[marked[bd]]] = True
            add &= ~marked
            if not add.any():
                break
            marked |= add
    return comp.astype(np.int32), summary_of(comp, rounds, trimmed, int(alive.sum()))


def scc_tarjan(V, src, dst):
    """int32 [V]: the smallest member of every vertex's SCC (iterative Tarjan)."""
    s, d, _ = arcs_and_loops(V, src, dst)
    off = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(s, minlength=V), out=off[1:])   # (s, d) ascending: d is the out-lists
    off, nbr = off.tolist(), d.tolist()
    index = [-1] * V
    low = [0] * V
    on = [False] * V
    comp = np.arange(V, dtype=np.int32)
    stack, n = [], 0
    for root in range(V):
        if index[root] >= 0:
            continue
        work = [(root, off[root])]
        index[root] = low[root] = n
        n += 1
        stack.append(root)
        on[root] = True
        while work:
            v, i = work.pop()
            if i < off[v + 1]:
                work.append((v, i + 1))
                w = nbr[i]
                if index[w] < 0:
                    index[w] = low[w] = n
                    n += 1
                    stack.append(w)
                    on[w] = True
                    work.append((w, off[w]))
                elif on[w]:
                    low[v] = min(low[v], index[w])
                continue
            if low[v] == index[v]:
                members = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    members.append(w)
                    if w == v:
                        break
                comp[members] = min(members)
            if work:
                p = work[-1][0]
                low[p] = min(low[p], low[v])
    return comp


# ---- graphs ----
def chain_of_2cycles(k, ascending=True):
    """k SCCs {2i, 2i+1} joined S_0 -> S_1 -> ... -> S_{k-1} by 2i+1 -> 2i+2.  ascending=False
    relabels x as 2k - 1 - x: the ids fall along the chain."""
    i = np.arange(k, dtype=np.int64)
    s = np.concatenate([2 * i, 2 * i + 1, 2 * i[:-1] + 1])
    d = np.concatenate([2 * i + 1, 2 * i, 2 * i[:-1] + 2])
    if not ascending:
        s, d = 2 * k - 1 - s, 2 * k - 1 - d
    return 2 * k, s.astype(np.int32), d.astype(np.int32)


def wheel(k):
    """Hub 0 <-> each of the leaves 1..k, both directions: one SCC."""
    leaf = np.arange(1, k + 1, dtype=np.int32)
    hub = np.zeros(k, np.int32)
    return k + 1, np.concatenate([hub, leaf]), np.concatenate([leaf, hub])


def path(n):
    """i -> i + 1 on n vertices."""
    i = np.arange(n - 1, dtype=np.int32)
    return n, i, i + 1


def cycle(n, rotate=0):
    """One directed cycle over n vertices, the edge list starting rotate ids on."""
    i = (np.arange(n, dtype=np.int64) + rotate) % n
    return n, i.astype(np.int32), ((i + 1) % n).astype(np.int32)
