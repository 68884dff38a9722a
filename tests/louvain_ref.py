"""CPU restatements of lpa_louvain (include/lpa.h "lpa_louvain" states the rules): the
synchronous, deterministic Louvain in exact integers.  Two independent forms that return
``(comm, levels, summary)``:

  louvain          vectorised: one scipy CSR product per round, int64 numpy
  louvain_literal  dicts and Python ints, vertex by vertex

``comm`` is int32 [V]; ``levels`` a list of dicts with the fields of lpa_louvain_level;
``summary`` a dict with the fields of lpa_louvain_summary.
"""
import numpy as np
import scipy.sparse as sp

A_MAX = 3_037_000_499
LEVEL_KEYS = ("vertices", "communities", "rounds", "damped_rounds", "moves", "numerator")
SUMMARY_KEYS = ("n_communities", "n_singletons", "largest_size", "largest_id", "levels", "rounds",
                "damped_rounds", "moves", "arcs", "intra_arcs", "numerator", "modularity")


# ---- small generators of the closed-form cases ----
def path(n):
    a = np.arange(n - 1, dtype=np.int32)
    return n, a, a + 1


def cycle(n):
    a = np.arange(n, dtype=np.int32)
    return n, a, ((a + 1) % n).astype(np.int32)


def ring_of_cliques(n_cliques=30, k=5):
    s, d = [], []
    for q in range(n_cliques):
        b = q * k
        for i in range(k):
            for j in range(i + 1, k):
                s.append(b + i)
                d.append(b + j)
        s.append(b + k - 1)
        d.append(((q + 1) % n_cliques) * k)
    return n_cliques * k, np.array(s, np.int32), np.array(d, np.int32)


def planted(V=2000, blocks=20, m=30000, p_in=0.8, seed=11):
    """V vertices in `blocks` random blocks; a fraction p_in of the m edges has its destination
    drawn inside the source's block.  Returns (V, src, dst, block)."""
    rng = np.random.default_rng(seed)
    block = rng.integers(0, blocks, V)
    members = [np.flatnonzero(block == b) for b in range(blocks)]
    src = rng.integers(0, V, m)
    dst = rng.integers(0, V, m)
    inside = rng.random(m) < p_in
    pick = rng.random(m)
    for i in np.flatnonzero(inside):
        mem = members[block[src[i]]]
        dst[i] = mem[int(pick[i] * mem.size)]
    return V, src.astype(np.int32), dst.astype(np.int32), block


def modularity_np(V, src, dst, labels):
    """(numerator, intra_arcs, arcs, n_communities) of a labelling, plain numpy int64."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    labels = np.asarray(labels, np.int64)
    ok = (src >= 0) & (src < V) & (dst >= 0) & (dst < V)
    src, dst = src[ok], dst[ok]
    arcs = 2 * int(src.size)
    deg = np.bincount(src, minlength=V) + np.bincount(dst, minlength=V)
    intra = 2 * int((labels[src] == labels[dst]).sum())
    D = np.zeros(V, np.int64)
    np.add.at(D, labels, deg)
    return arcs * intra - int((D * D).sum()), intra, arcs, int(np.unique(labels).size)


def _kept(V, src, dst):
    src = np.asarray(src, np.int64).reshape(-1)
    dst = np.asarray(dst, np.int64).reshape(-1)
    ok = (src >= 0) & (src < V) & (dst >= 0) & (dst < V)
    return src[ok], dst[ok]


def _finish(V, member_comm, levels, A, intra, numer):
    """comm (smallest original member), then the summary."""
    comm = np.arange(V, dtype=np.int64)
    if V:
        low = np.full(int(member_comm.max()) + 1, V, np.int64)
        np.minimum.at(low, member_comm, np.arange(V))
        comm = low[member_comm]
    sizes = np.bincount(comm, minlength=V) if V else np.zeros(0, np.int64)
    big = int(sizes.max()) if V else 0
    summ = dict(n_communities=int((sizes > 0).sum()), n_singletons=int((sizes == 1).sum()), largest_size=big,
                largest_id=int(np.flatnonzero(sizes == big)[0]) if V else -1, levels=len(levels),
                rounds=sum(r["rounds"] for r in levels), damped_rounds=sum(r["damped_rounds"] for r in levels),
                moves=sum(r["moves"] for r in levels), arcs=int(A), intra_arcs=int(intra), numerator=int(numer),
                modularity=float(numer) / (float(A) * float(A)) if A else 0.0)
    return comm.astype(np.int32), levels, summ


def _check_args(max_levels, max_rounds):
    if max_levels <= 0 or max_rounds <= 0:
        raise ValueError("max_levels and max_rounds must be greater than 0")


# ---------------------------------------------------------------------------------------
# vectorised
# ---------------------------------------------------------------------------------------
def _numerator(A, W, s, k, c):
    coo = W.tocoo()
    intra = int(s.sum()) + int(coo.data[c[coo.row] == c[coo.col]].sum())
    D = np.zeros(k.size, np.int64)
    np.add.at(D, c, k)
    return A * intra - int((D * D).sum()), intra, D


def _proposals(A, W, k, c, D, size):
    """prop[u] = the community u proposes to move to, or -1."""
    n = k.size
    onehot = sp.csr_matrix((np.ones(n, np.int64), (np.arange(n), c)), shape=(n, n))
    K = (W @ onehot).tocoo()
    u, x, kv = K.row.astype(np.int64), K.col.astype(np.int64), K.data.astype(np.int64)
    pos = kv > 0
    u, x, kv = u[pos], x[pos], kv[pos]
    own = x == c[u]
    kown = np.zeros(n, np.int64)
    kown[u[own]] = kv[own]
    score_a = A * kown - k * (D[c] - k)
    u, x, kv = u[~own], x[~own], kv[~own]
    score = A * kv - k[u] * D[x]
    order = np.lexsort((x, -score, u))       # by row, then score descending, then x ascending
    u, x, score = u[order], x[order], score[order]
    first = np.ones(u.size, bool)
    first[1:] = u[1:] != u[:-1]
    u, b, score = u[first], x[first], score[first]
    a = c[u]
    go = (score > score_a[u]) & ~((size[a] == 1) & (size[b] == 1) & (b > a))
    prop = np.full(n, -1, np.int64)
    prop[u[go]] = b[go]
    return prop


def louvain(V, src, dst, max_levels=64, max_rounds=1000, trace=None):
    """trace (a list): the result as it stands after every counted level is appended to it, i.e.
    what max_levels = 1, 2, ... return (tests/test_louvain_host.py checks that they do)."""
    _check_args(max_levels, max_rounds)
    V = int(V)
    src, dst = _kept(V, src, dst)
    A = 2 * int(src.size)
    if A > A_MAX:
        raise ValueError(f"{A} arcs exceed {A_MAX}")
    member = np.arange(V, dtype=np.int64)
    if V == 0 or A == 0:
        return _finish(V, member, [], 0, 0, 0)
    loop = src == dst
    s = 2 * np.bincount(src[loop], minlength=V).astype(np.int64)
    a, b = src[~loop], dst[~loop]
    W = sp.csr_matrix((np.ones(2 * a.size, np.int64), (np.concatenate([a, b]), np.concatenate([b, a]))),
                      shape=(V, V))
    W.sum_duplicates()
    levels = []
    while True:
        n = s.size
        k = s + np.asarray(W.sum(axis=1)).reshape(-1).astype(np.int64)
        c = np.arange(n, dtype=np.int64)
        N, intra, D = _numerator(A, W, s, k, c)
        size = np.ones(n, np.int64)
        rounds = damped = moves = 0
        while rounds < max_rounds:
            prop = _proposals(A, W, k, c, D, size)
            want = prop >= 0
            if not want.any():
                break
            rounds += 1
            accepted = False
            for sub, is_damped in ((want, False), (want & (prop < c), True)):
                if not sub.any():
                    continue
                c2 = np.where(sub, prop, c)
                N2, intra2, D2 = _numerator(A, W, s, k, c2)
                if N2 > N:
                    c, N, intra, D = c2, N2, intra2, D2
                    size = np.bincount(c, minlength=n)
                    moves += int(sub.sum())
                    damped += int(is_damped)
                    accepted = True
                    break
            if not accepted:
                break
        if moves == 0:
            break
        alive = np.flatnonzero(size > 0)
        newid = np.full(n, -1, np.int64)
        newid[alive] = np.arange(alive.size)
        nc = newid[c]
        member = nc[member]
        P = sp.csr_matrix((np.ones(n, np.int64), (np.arange(n), nc)), shape=(n, alive.size))
        W2 = (P.T @ W @ P).tocsr()
        s2 = np.zeros(alive.size, np.int64)
        np.add.at(s2, nc, s)
        s = s2 + W2.diagonal().astype(np.int64)
        W2.setdiag(0)
        W2.eliminate_zeros()
        W = W2
        levels.append(dict(vertices=n, communities=int(alive.size), rounds=rounds, damped_rounds=damped,
                           moves=moves, numerator=int(N)))
        if trace is not None:
            trace.append(_finish(V, member, list(levels), A, intra, N))
        if len(levels) == max_levels:
            break
    return _finish(V, member, levels, A, intra, N)


# ---------------------------------------------------------------------------------------
# literal
# ---------------------------------------------------------------------------------------
def louvain_literal(V, src, dst, max_levels=64, max_rounds=1000):
    _check_args(max_levels, max_rounds)
    V = int(V)
    src, dst = _kept(V, src, dst)
    A = 2 * len(src)
    member = list(range(V))
    if V == 0 or A == 0:
        return _finish(V, np.arange(V, dtype=np.int64), [], 0, 0, 0)
    s = [0] * V
    w = [dict() for _ in range(V)]
    for u, v in zip(src.tolist(), dst.tolist()):
        if u == v:
            s[u] += 2
        else:
            w[u][v] = w[u].get(v, 0) + 1
            w[v][u] = w[v].get(u, 0) + 1

    def numerator(c):
        intra = sum(s)
        D = {}
        for u in range(len(s)):
            D[c[u]] = D.get(c[u], 0) + k[u]
            for v, x in w[u].items():
                if c[v] == c[u]:
                    intra += x
        return A * intra - sum(d * d for d in D.values()), intra

    levels = []
    while True:
        n = len(s)
        k = [s[u] + sum(w[u].values()) for u in range(n)]
        c = list(range(n))
        N, intra = numerator(c)
        rounds = damped = moves = 0
        while rounds < max_rounds:
            D, size = [0] * n, [0] * n
            for u in range(n):
                D[c[u]] += k[u]
                size[c[u]] += 1
            prop = {}
            for u in range(n):
                a = c[u]
                K = {}
                for v, x in w[u].items():
                    K[c[v]] = K.get(c[v], 0) + x
                best = None
                for x in sorted(K):
                    if x == a:
                        continue
                    sc = A * K[x] - k[u] * D[x]
                    if best is None or sc > best[0]:
                        best = (sc, x)
                if best is None:
                    continue
                sc_a = A * K.get(a, 0) - k[u] * (D[a] - k[u])
                b = best[1]
                if best[0] > sc_a and not (size[a] == 1 and size[b] == 1 and b > a):
                    prop[u] = b
            if not prop:
                break
            rounds += 1
            full = list(c)
            for u, b in prop.items():
                full[u] = b
            Nf, If = numerator(full)
            if Nf > N:
                c, N, intra = full, Nf, If
                moves += len(prop)
                continue
            down = {u: b for u, b in prop.items() if b < c[u]}
            if down:
                part = list(c)
                for u, b in down.items():
                    part[u] = b
                Np, Ip = numerator(part)
                if Np > N:
                    c, N, intra = part, Np, Ip
                    moves += len(down)
                    damped += 1
                    continue
            break
        if moves == 0:
            break
        alive = sorted(set(c))
        newid = {x: i for i, x in enumerate(alive)}
        s2 = [0] * len(alive)
        w2 = [dict() for _ in alive]
        for u in range(n):
            i = newid[c[u]]
            s2[i] += s[u]
            for v, x in w[u].items():
                j = newid[c[v]]
                if i == j:
                    s2[i] += x
                else:
                    w2[i][j] = w2[i].get(j, 0) + x
        member = [newid[c[i]] for i in member]
        s, w = s2, w2
        levels.append(dict(vertices=n, communities=len(alive), rounds=rounds, damped_rounds=damped, moves=moves,
                           numerator=N))
        if len(levels) == max_levels:
            break
    return _finish(V, np.asarray(member, np.int64), levels, A, intra, N)
