"""numpy-only reference for connected components (no scipy): min-label hooking plus
pointer jumping, iterated until nothing changes.

comp[v] = the smallest vertex id of v's component in the undirected view of the
multigraph (direction, duplicates and self-loops make no difference; an edgeless vertex is
its own component) -- the value lpa_components returns."""
import numpy as np


def components(V, src, dst):
    """comp (int64[V]) of the graph on vertices [0, V) with edges (src[i], dst[i])."""
    comp = np.arange(V, dtype=np.int64)
    s = np.asarray(src).astype(np.int64)
    d = np.asarray(dst).astype(np.int64)
    keep = s != d
    s, d = s[keep], d[keep]
    while True:
        prev = comp.copy()
        # hooking: the root of either endpoint's tree takes the smaller of the two labels
        cs, cd = comp[s], comp[d]
        lo = np.minimum(cs, cd)
        np.minimum.at(comp, cs, lo)
        np.minimum.at(comp, cd, lo)
        # pointer jumping until every vertex points at a root
        while True:
            nxt = comp[comp]
            if np.array_equal(nxt, comp):
                break
            comp = nxt
        if np.array_equal(comp, prev):
            return comp


def summary(comp):
    """sizes (int64[V]: members at each component id, 0 elsewhere) and the summary dict of
    lpa_components_summary, from np.bincount."""
    V = comp.size
    sizes = np.bincount(comp, minlength=V).astype(np.int64)
    ids = np.flatnonzero(sizes)
    largest = int(sizes.max()) if V else 0
    return sizes, dict(n_components=int(ids.size), n_singletons=int((sizes == 1).sum()),
                       largest_size=largest,
                       largest_id=int(np.flatnonzero(sizes == largest)[0]) if V else -1)
