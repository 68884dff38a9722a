"""CPU restatement of lpa_scan (include/lpa.h), written from the definition with Python sets: no
orientation, no union-find, clusters grown breadth-first from the smallest unlabelled core.  It
shares no code and no approach with csrc/lpa_scan.hip.  The one floating-point decision, whether
an edge is similar, is the header's binary64 expression evaluated by numpy scalars: each product
rounded once, no fused multiply-add.

prepare(V, s, d)      the canonical simple undirected graph (self-loops dropped, direction ignored,
                      duplicates collapsed, ids outside [0, V) dropped): neighbour sets, degrees,
                      common neighbours per edge and per input row -- all independent of eps, mu
scan(prep, eps, mu)   label, role, nsim (numpy arrays) and the summary dict
"""
from collections import deque

import numpy as np

ROLES = ("outlier", "hub", "border", "core")
OUTLIER, HUB, BORDER, CORE = range(4)
SUMMARY_KEYS = ("simple_edges", "triangles", "similar_edges", "n_clusters", "n_cores", "n_borders", "n_hubs",
                "n_outliers", "largest_cluster", "largest_cluster_label")


class Prepared:
    def __init__(self, V, adj, common, common_rows):
        self.V = V
        self.adj = adj                    # list of neighbour sets
        self.deg = [len(a) for a in adj]
        self.common = common              # {(min, max): common neighbours}
        self.common_rows = common_rows    # int32 per input row, -1: no edge of the simple graph


def prepare(V, s, d) -> Prepared:
    s = [int(x) for x in np.asarray(s).ravel()]
    d = [int(x) for x in np.asarray(d).ravel()]
    adj = [set() for _ in range(V)]
    for a, b in zip(s, d):
        if a != b and 0 <= a < V and 0 <= b < V:
            adj[a].add(b)
            adj[b].add(a)
    common = {}
    for a in range(V):
        for b in adj[a]:
            if a < b:
                common[(a, b)] = len(adj[a] & adj[b])
    rows = np.full(len(s), -1, np.int32)
    for i, (a, b) in enumerate(zip(s, d)):
        if a != b and 0 <= a < V and 0 <= b < V:
            rows[i] = common[(min(a, b), max(a, b))]
    return Prepared(V, adj, common, rows)


def similar(c, du, dv, eps) -> bool:
    """The header's test, in binary64, every product rounded once."""
    eps = np.float64(eps)
    a = np.float64(c + 2)
    return bool(a * a >= (eps * eps) * (np.float64(du + 1) * np.float64(dv + 1)))


def scan(p: Prepared, eps, mu):
    V, adj, deg = p.V, p.adj, p.deg
    sim = [set() for _ in range(V)]       # similar neighbours
    n_similar = 0
    for (a, b), c in p.common.items():
        if similar(c, deg[a], deg[b], eps):
            sim[a].add(b)
            sim[b].add(a)
            n_similar += 1
    nsim = np.array([len(x) for x in sim], np.int32).reshape(V)
    core = [len(sim[v]) + 1 >= mu for v in range(V)]
    label = [None] * V
    # clusters of cores: breadth-first from the smallest unlabelled core, over similar core-core edges
    for v in range(V):
        if core[v] and label[v] is None:
            label[v] = v
            queue = deque([v])
            while queue:
                x = queue.popleft()
                for y in sim[x]:
                    if core[y] and label[y] is None:
                        label[y] = v
                        queue.append(y)
    role = np.zeros(V, np.uint8)
    out = np.arange(V, dtype=np.int32)
    for v in range(V):
        if core[v]:
            role[v], out[v] = CORE, label[v]
        else:
            around = [label[y] for y in sim[v] if core[y]]
            if around:
                role[v], out[v] = BORDER, min(around)
    member = role >= BORDER
    for v in range(V):
        if not member[v]:
            seen = {int(out[y]) for y in adj[v] if member[y]}
            role[v] = HUB if len(seen) >= 2 else OUTLIER
    sizes = {}
    for v in range(V):
        if member[v]:
            sizes[int(out[v])] = sizes.get(int(out[v]), 0) + 1
    big = max(sizes.values()) if sizes else 0
    summary = dict(
        simple_edges=len(p.common),
        triangles=sum(p.common.values()) // 3,
        similar_edges=n_similar,
        n_clusters=len(sizes),
        n_cores=int((role == CORE).sum()),
        n_borders=int((role == BORDER).sum()),
        n_hubs=int((role == HUB).sum()),
        n_outliers=int((role == OUTLIER).sum()),
        largest_cluster=big,
        largest_cluster_label=min(l for l, n in sizes.items() if n == big) if sizes else -1)
    return out, role, nsim, summary
