"""Seeded test graphs covering every degree bin and the edge cases of the path."""
import numpy as np


def two_cliques(n=5):
    """Upstream LabelPropagationSuite shape (Spark graphx + GraphFrames): clique1 =
    all (u, v) for u, v in [0, n) (self-loops included), clique2 = all (u+n, v+n)
    for u, v in [0, n], plus the bridge (0, n)."""
    e = [(u, v) for u in range(n) for v in range(n)]
    e += [(u + n, v + n) for u in range(n + 1) for v in range(n + 1)]
    e.append((0, n))
    a = np.array(e, dtype=np.int32)
    return 2 * n + 1, a[:, 0].copy(), a[:, 1].copy()


def star(k):
    """Hub 0 with leaves 1..k: period-2 oscillation under synchronous LPA."""
    s = np.zeros(k, dtype=np.int32)
    d = np.arange(1, k + 1, dtype=np.int32)
    return k + 1, s, d


def degree_mix(seed=0, hubs=(600, 2100, 4500, 9000), n_low=3000, extra=20000):
    """Random multigraph whose symmetrised degrees span every bin: a few hubs
    (single- and multi-segment), a wave band, and the g1..g16 bands; duplicates,
    self-loops and isolated vertices included."""
    rng = np.random.default_rng(seed)
    V = n_low + len(hubs) + 50
    src, dst = [], []
    for h, deg in enumerate(hubs):
        nb = rng.integers(len(hubs), V, size=deg)
        # few distinct neighbours for some hubs -> repeated labels, many for others
        if h % 2:
            nb = nb % 97 + len(hubs)
        src.append(np.full(deg, h))
        dst.append(nb)
    s = rng.integers(len(hubs), V - 50, size=extra)
    d = rng.integers(len(hubs), V - 50, size=extra)
    # skew: square-law endpoints make a wave band of medium degrees
    d = (len(hubs) + ((d - len(hubs)) ** 2) // (V - 50 - len(hubs))).astype(np.int64)
    src.append(s)
    dst.append(d)
    src.append(np.array([len(hubs) + 7, len(hubs) + 9]))   # self-loops
    dst.append(np.array([len(hubs) + 7, len(hubs) + 9]))
    s = np.concatenate(src).astype(np.int32)
    d = np.concatenate(dst).astype(np.int32)
    perm = rng.permutation(V).astype(np.int32)   # scramble ids
    return V, perm[s], perm[d]


def stale_units(leaves=10_000, leaf_loops=200):
    """A hub of > 8192 arcs (above the block tiers: tallied by 512-arc units) whose
    superstep-1 changes touch < 0.5 % of the arcs (leaves held by self-loops), so that
    superstep 2 runs on the exact frontier right after the column-run superstep 1.
    The hub row is dirty in superstep 2 only through x (a late unit); b sits in the
    hub row's first unit, keeps its label in superstep 1 and changes in superstep 2
    (to its cluster's label), so a unit word staged by an earlier run differs from the
    superstep-2 truth.  (the column-run path staged no unit words.)"""
    hub, b, c0, y = 0, 1, 2, 3
    nclu = 350
    clu = np.arange(4, 4 + nclu)
    lv = np.arange(4 + nclu, 4 + nclu + leaves)
    x = 4 + nclu + leaves
    V = x + 1
    e = []
    e.append(np.stack([np.full(leaves, hub), lv]))                      # hub - leaves
    e.append(np.stack([np.repeat(lv, leaf_loops), np.repeat(lv, leaf_loops)]))  # leaf self-loops
    e.append(np.stack([np.full(3, hub), np.full(3, b)]))                # b: 3 votes at the hub
    e.append(np.stack([np.full(300, b), np.full(300, b)]))              # b: 600 own votes
    e.append(np.stack([np.repeat(np.full(nclu, b), 2), np.repeat(clu, 2)]))  # b: 700 cluster votes
    e.append(np.stack([np.repeat(clu, 3), np.full(3 * nclu, c0)]))      # cluster -> c0 in superstep 1
    e.append(np.stack([np.full(200, x), np.full(200, y)]))              # x -> y in superstep 1
    e.append(np.stack([np.array([x]), np.array([hub])]))                # x dirties the hub row
    a = np.concatenate(e, axis=1).astype(np.int32)
    return V, a[0].copy(), a[1].copy()


def random_multigraph(V, m, seed):
    rng = np.random.default_rng(seed)
    return V, rng.integers(0, V, size=m).astype(np.int32), rng.integers(0, V, size=m).astype(np.int32)


def comb_bucket(labels, lg):
    """k_hub_combine's label-hash bucket (lpa_hub.hip comb_bucket)."""
    x = (labels.astype(np.uint64) * np.uint64(0x85EBCA77)) & np.uint64(0xFFFFFFFF)
    return (x >> np.uint64(32 - lg)).astype(np.int64) if lg else np.zeros(labels.shape, np.int64)


def giant_hub(seed=0, n_plain=200000, n_skew=20000, lg=7):
    """Hub 0 with n_plain + n_skew distinct neighbours (iteration 1: every staged
    word distinct -> 2^lg combine buckets), n_skew of which hash into ONE bucket
    (-> that bucket needs sub-bucket passes).  One skewed neighbour carries three
    parallel edges, so the hub's mode is decided inside the overloaded bucket; two
    plain neighbours carry two, testing the cross-bucket maximum."""
    rng = np.random.default_rng(seed)
    V = 4 * (n_plain + n_skew) + 1
    ids = np.arange(1, V, dtype=np.int64)
    b = comb_bucket(ids, lg)
    skew = rng.permutation(ids[b == 3])[:n_skew]
    rest = rng.permutation(ids[b != 3])[:n_plain]
    nb = np.concatenate([skew, rest, [skew[5]] * 2, [rest[7], rest[9]]])
    s = np.zeros(nb.size, np.int64)
    # a sparse random background so the leaves are not all degree 1
    bs = rng.integers(1, V, size=V // 2)
    bd = rng.integers(1, V, size=V // 2)
    return V, np.concatenate([s, bs]).astype(np.int32), np.concatenate([nb, bd]).astype(np.int32)


def comb_sub(labels, lg):
    """k_hub_bucket's sub-bucket hash (lpa_hub.hip comb_sub)."""
    x = (labels.astype(np.uint64) * np.uint64(0xC2B2AE3D)) & np.uint64(0xFFFFFFFF)
    return (x >> np.uint64(32 - lg)).astype(np.int64) if lg else np.zeros(labels.shape, np.int64)


def adversarial_hub(n_nb=20000, seed=0):
    """Hub 0 whose n_nb distinct neighbours ALL share one combine bucket (4 hash bits)
    and one sub-bucket (3 bits): in superstep 1 (labels = ids) its bucket pass meets
    n_nb > 8192 distinct labels, more than the LDS table holds (the case the spill
    guard must handle without dropping votes).  One neighbour carries a triple edge,
    so the hub's mode is decided inside that pass; a sparse background among the
    neighbours keeps later supersteps non-trivial."""
    rng = np.random.default_rng(seed)
    ids = np.arange(1, 200 * n_nb, dtype=np.int64)
    sel = ids[(comb_bucket(ids, 4) == 5) & (comb_sub(ids, 3) == 2)][:n_nb]
    assert sel.size == n_nb
    V = int(sel.max()) + 1
    nb = np.concatenate([rng.permutation(sel), [sel[17]] * 2])
    s = np.zeros(nb.size, np.int64)
    bs = rng.choice(sel, size=n_nb)
    bd = rng.choice(sel, size=n_nb)
    return V, np.concatenate([s, bs]).astype(np.int32), np.concatenate([nb, bd]).astype(np.int32)


def settled_hubs(seed=0, V=20000, n_hub=30, n_mover=40):
    """Nearly every vertex keeps its L0 label in superstep 1 (a self-loop = 2 votes
    for itself against single votes from distinct neighbours), so only the few
    `movers` (no self-loop) change and superstep 2 already runs on a frontier list
    -- with hub rows of 1024 < deg <= 4096, the rows the label-dense supersteps tally
    with one block each (k_lpa_block in list mode)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(V)
    hubs, movers = perm[:n_hub], perm[n_hub:n_hub + n_mover]
    src, dst = [], []
    for h in hubs:
        nb = rng.choice(V, size=int(rng.integers(1100, 3000)), replace=False)
        nb = nb[nb != h]
        src.append(np.full(nb.size, h)), dst.append(nb)
    bg = rng.integers(0, V, size=(2 * V, 2))
    src.append(bg[:, 0]), dst.append(bg[:, 1])
    keep = np.setdiff1d(np.arange(V), movers)
    src.append(keep), dst.append(keep)                      # one self-loop each
    src.append(np.repeat(hubs, 2)), dst.append(np.repeat(hubs, 2))   # hubs: 3 in all
    for m in movers:                                        # 4 distinct hubs each
        hs = rng.choice(hubs, size=4, replace=False)
        src.append(np.full(4, m)), dst.append(hs)
    return V, np.concatenate(src).astype(np.int32), np.concatenate(dst).astype(np.int32)


def _mul32(x, k):
    return (np.asarray(x).astype(np.uint64) * np.uint64(k)) & np.uint64(0xFFFFFFFF)


def hash_slot(labels, shift):
    """lpa_device.h hash_slot: shift 26 = the 64 buckets of giant_count (wave bins, block
    rows, units), shift 28 = the 16 buckets of the row bins' giant test."""
    return (_mul32(labels, 0x9E3779B1) >> np.uint64(shift)).astype(np.int64)


def giant_code2(labels):
    """lpa_codes.h giant_code2 of a label that is not G: 1 + a 3-way label hash."""
    return (1 + (((_mul32(labels, 0x9E3779B1) >> np.uint64(24)) * np.uint64(3)) >> np.uint64(8))).astype(np.int64)


TIE_DEGREES = (16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 4096, 4097, 8192, 8193,
               10240, 10241, 33281)


def tie_anchor_ids(region=256):
    """The anchor ids of tie_rows, found by restating the library's hashes: G, rivals
    A < B < G < C < D and E with
    - A, B in one bucket of every hash (hash_slot 26 / 28, giant_code2), C, D likewise;
    - A, C, E in three different buckets of every hash (and of comb_bucket, 4 bits);
    - no rival in a bucket of another pair."""
    ids = np.arange(region)
    h26, code, cb = hash_slot(ids, 26), giant_code2(ids), comb_bucket(ids, 4)
    same = lambda x, y: h26[x] == h26[y] and code[x] == code[y]
    for G in range(region // 4, region):
        lo = [(a, b) for a in range(G) for b in range(a + 1, G) if same(a, b)]
        hi = [(c, d) for c in range(G + 1, region) for d in range(c + 1, region) if same(c, d)]
        for a, b in lo:
            for c, d in hi:
                if code[a] == code[c] or h26[a] >> 2 == h26[c] >> 2 or cb[a] == cb[c]:
                    continue
                for e in range(region):
                    if e in (a, b, G, c, d) or code[e] in (code[a], code[c]):
                        continue
                    if len({int(h26[x]) >> 2 for x in (a, c, e)}) == 3 and len({int(cb[x]) for x in (a, c, e)}) == 3:
                        return dict(G=G, A=a, B=b, C=c, D=d, E=e)
    raise AssertionError("no anchor ids in the region")


def _tie_tables(d, an):
    """The vote tables of one row of degree d (ISSUE tables (a)-(h)): n = d - 2 engineered
    votes (two arcs go to the row's blinker pair, whose labels share E's code bucket and
    no rival's hash bucket).  name -> {label: count}."""
    G, A, B, C, D, E = (an[k] for k in "GABCDE")
    n = d - 2
    c = (n - 1) // 2
    t = {
        "a_tie_lo": {G: n // 2, A: n - n // 2},           # even n: tie, A < G wins; odd: A by one
        "b_tie_hi": {G: n - n // 2, C: n // 2},           # even n: tie, G < C wins; odd: G by one
        "c_g_plus1_lo": {G: c + 1, A: c, E: n - 2 * c - 1},
        "c_g_minus1_lo": {G: c, A: c + 1, E: n - 2 * c - 1},
        "c_g_plus1_hi": {G: c + 1, C: c, E: n - 2 * c - 1},
        "c_g_minus1_hi": {G: c, C: c + 1, E: n - 2 * c - 1},
    }
    # (d) G = g; two rivals of ONE bucket, each below g, together >= g
    g = n // 2
    t["d_pair_lo"] = {G: g, A: (n - g + 1) // 2, B: (n - g) // 2}
    t["d_pair_hi"] = {G: g, C: (n - g + 1) // 2, D: (n - g) // 2}
    # (e) G = g; rivals in three code buckets at g - 1 (E's bucket: g - 3 + the two blinkers)
    g = -(-(n + 5) // 4)
    t["e_three"] = {G: g, A: g - 1, C: g - 1, E: n - 3 * g + 2}
    t["f_no_g"] = {A: n - 2 * (n // 3), C: n // 3, E: n // 3}
    # (h) two non-G labels tied (A < C wins), G a minority
    g = (n - n // 8) // 2
    t["h_rivals_tie"] = {A: g, C: g, G: n - 2 * g}
    if d > 8192:   # (g) a rival run of > 1023 consecutive arcs: whole 512-arc units of one bucket
        t["g_full_unit"] = {G: n // 2 - 256, C: n - n // 2 + 256}
    return {k: {l: v for l, v in tab.items() if v > 0} for k, tab in t.items()}


def tie_mode(table):
    """Mode of a vote table, the smallest label on a tie."""
    top = max(table.values())
    return min(l for l, v in table.items() if v == top)


def tie_rows(degrees=TIE_DEGREES, g_mass=90_000, pad_to=0, mult_g=(200, 160, 130), mult_x=(120, 80, 40),
             cap_g=28, cap_x=36, loops=200):
    """Layered-anchor fixture with engineered ties and bin-edge degrees at the giant-label
    decision sites; no random input, every row's mode known analytically.

    Anchors (`loops` self-loops each) keep their ids for ever: G and the rivals of
    tie_anchor_ids.  Below every anchor hang three layers of pool vertices, vertex i of
    layer k joined to vertex i of layer k - 1 by mult[k - 1] parallel edges (falling with
    depth, the fall above the cap of row attachments per pool vertex), so a layer-k vertex
    takes its anchor's label in superstep k and keeps it.  g_mass vertices on two parallel
    edges to G put G on more than half of the slots from superstep 1 on.  A test row is a
    vertex that is only ever a source: its arcs go to the layer-`depth` pools with a chosen
    count per label (consecutive pool vertices, the cursor moving round the pool), plus one
    arc to each vertex of its blinker pair -- two vertices joined by three parallel edges,
    which swap labels every superstep and keep the row dirty.  From superstep depth + 1 on
    the row's neighbourhood histogram is exactly its table plus two singletons.  (One row per
    degree and depth has no blinker pair: G on exactly half of ALL its arcs.)
    G's pools sit in higher degree bins than the rivals' (mult_g vs mult_x), so in a row of
    G and one rival the rival's arcs are contiguous in the column-sorted row.

    The largest row (> 64 units) carries only tables a, b, g.  pad_to: isolated vertices
    up to that many ids (the compact graph is a prefix: labels of the first V ids agree).

    Returns V, src, dst, rows [(row id, depth, {label: votes})], G."""
    an = tie_anchor_ids()
    G = an["G"]
    rivals = [an[k] for k in "ABCDE"]
    region = 256
    specs = []
    for d in degrees:
        for name, tab in _tie_tables(d, an).items():
            if d > 32768 and name[0] not in "abg":
                continue
            for depth in (1, 2, 3):
                specs.append((d, depth, name, tab))
        if d <= 32768:
            # no blinker pair: G on exactly half of the row's arcs, the smaller rival on the other
            # half (odd d: the rival one more) -- the strict-majority settles' 2 c > deg at equality
            for depth in (1, 2, 3):
                specs.append((d, depth, "z_half_pure", {G: d // 2, an["A"]: d - d // 2}))
    need = {}
    for d, depth, name, tab in specs:
        for l, v in tab.items():
            need[(l, depth)] = need.get((l, depth), 0) + v
    psize = {l: max(-(-need.get((l, k), 0) // (cap_g if l == G else cap_x)) for k in (1, 2, 3)) for l in [G] + rivals}
    psize = {l: max(p, 1) for l, p in psize.items()}
    nxt = region
    mass = np.arange(nxt, nxt + g_mass)
    nxt += g_mass
    fill_mult = (1, 6, 12, 24, 48)     # G-mass vertices of degrees in g1, g8, g16, g32, g64
    fill = np.arange(nxt, nxt + 8 * len(fill_mult)).reshape(len(fill_mult), 8)
    nxt += fill.size
    pools = {}
    for l in [G] + rivals:
        for k in (1, 2, 3):
            pools[(l, k)] = np.arange(nxt, nxt + psize[l])
            nxt += psize[l]
    row_ids = np.arange(nxt, nxt + len(specs))
    nxt += len(specs)
    # blinker ids: the largest ids; code bucket of E, hash buckets of no rival
    cand = np.arange(nxt, nxt + 40 * len(specs))
    bad28 = {int(hash_slot(np.array([x]), 28)[0]) for x in rivals}
    ok = (giant_code2(cand) == giant_code2(np.array([an["E"]]))[0]) & ~np.isin(hash_slot(cand, 28), list(bad28))
    blink = cand[ok][: 2 * len(specs)].reshape(-1, 2)
    assert blink.shape[0] == len(specs)
    V = int(blink.max()) + 1
    es, ed = [], []

    def add(s, d, m=1):
        es.append(np.repeat(np.asarray(s, dtype=np.int64), m))
        ed.append(np.repeat(np.broadcast_to(np.asarray(d, dtype=np.int64), np.shape(s)), m))

    for l in [G] + rivals:
        add(np.array([l]), l, loops)
        mult = mult_g if l == G else mult_x
        for k in (1, 2, 3):
            add(pools[(l, k)], pools[(l, k - 1)] if k > 1 else l, mult[k - 1])
    add(mass, G, 2)
    for i, m in enumerate(fill_mult):
        add(fill[i], G, m)
    cursor = {key: 0 for key in pools}
    rows = []
    for i, (d, depth, name, tab) in enumerate(specs):
        r = int(row_ids[i])
        for l, v in tab.items():
            p = pools[(l, depth)]
            add(np.full(v, r), p[(cursor[(l, depth)] + np.arange(v)) % p.size])
            cursor[(l, depth)] = (cursor[(l, depth)] + v) % p.size
        if name != "z_half_pure":
            u, w = blink[i]
            add(np.full(3, u), w)
            add(np.array([r, r]), np.array([u, w]))
        rows.append((r, depth, dict(tab)))
    V = max(V, int(pad_to))
    return V, np.concatenate(es).astype(np.int32), np.concatenate(ed).astype(np.int32), rows, G


def code_mix(src, dst, V0):
    """R-MAT edges (V0 vertices) plus structures whose superstep-2 mode is NOT the giant
    label, so that the giant-code settle of superstep 2 (lpa_codes.h "Giant codes")
    leaves rows to its exact fallback paths: five 200-cliques (wave-bin rows, 199 arcs,
    their own block's label), a 1,100-clique (block-tier hub rows, glist) and a leader
    l < hub h pair sharing 9,000 two-arc members (rows of 9,000 arcs above the block
    tiers, ulist2: every member's superstep-1 label is l).  Returns V, src, dst."""
    es, ed = [src.astype(np.int64)], [dst.astype(np.int64)]
    nxt = V0

    def clique(n):
        nonlocal nxt
        ids = np.arange(nxt, nxt + n, dtype=np.int64)
        nxt += n
        iu, ju = np.triu_indices(n, 1)
        es.append(ids[iu])
        ed.append(ids[ju])

    for _ in range(5):
        clique(200)
    clique(1100)
    lead, hub = nxt, nxt + 1
    mem = np.arange(nxt + 2, nxt + 2 + 9000, dtype=np.int64)
    nxt += 9002
    es += [np.full(mem.size, hub), np.full(mem.size, lead)]
    ed += [mem, mem]
    return nxt, np.concatenate(es).astype(np.int32), np.concatenate(ed).astype(np.int32)


# ---- the outlier stage's engineered fixture (tests/test_gpu_outlier_edges.py) ----
# per-community multisets of sub-group sizes: 1 = a vertex that stays alone (edgeless, or
# one of a label-swapping pair), n >= 3 = a clique of n vertices
OUTLIER_CATALOGUE = (
    ("n1", [5]),
    ("n1_single", [1]),
    ("n2_equal", [3, 3]),
    ("n9_distinct", [1, 3, 4, 5, 6, 9, 10, 17, 18]),            # k = 0: thr = 18, 8 groups flagged
    ("n9_equal", [4] * 9),
    ("n10_unique_min", [1, 3, 3, 4, 5, 6, 7, 8, 9, 33]),        # k = 1: thr = the minimum, nothing below it
    ("n10_min_tied", [1, 1, 3, 4, 5, 6, 7, 8, 9, 34]),
    ("n10_equal", [5] * 10),
    ("n11", [1, 3, 3, 3, 4, 4, 5, 5, 6, 6, 65]),
    ("n19", [1, 1, 1] + [3] * 8 + [4] * 7 + [66]),
    ("n20_min_lt_2nd", [1, 3] + [4] * 17 + [129]),              # k = 2: thr = 3, one group flagged
    ("n20_min_eq_2nd", [1, 1, 3] + [4] * 16 + [130]),           # thr = 1, none
    ("n20_2nd_eq_3rd", [1, 3, 3] + [4] * 16 + [257]),           # thr = 3, one
    ("n20_equal", [3] * 20),
    ("n21", [1, 3, 3] + [5] * 17 + [258]),                      # k = 2: thr = 3, one
    ("n29", [1, 3] + [4] * 26 + [513]),                         # k = 2: thr = 3, one
    ("n30", [1, 1, 3] + [4] * 26 + [514]),                      # k = 3: thr = 3, two
    ("n31", [1, 3, 4] + [5] * 27 + [1100]),                     # k = 3: thr = 4, two
    ("n100_run_straddles_k", [1] * 7 + [3] * 6 + [4] * 87),     # k = 10: positions 8..13 tied, 7 flagged
    ("n100_run_ends_at_k", [1] * 5 + [3] * 5 + [4] * 89 + [2100]),   # positions 6..10 tied, 5 flagged
    ("n100_run_starts_after_k", [1] * 10 + [3] * 6 + [4] * 84),      # positions 11..16 tied, thr = 1, none
    ("n100_one_below_k", [1] * 9 + [3] * 91),                   # position 10 opens the run, 9 flagged
)


def threshold_of(sizes):
    """App. B threshold of a multiset of group sizes: the k-th smallest (k = n // 10), the
    largest when k == 0 (an independent restatement: numpy sort, ascending)."""
    a = np.sort(np.asarray(sizes, dtype=np.int64))
    k = a.size // 10
    return int(a[k - 1] if k > 0 else a[-1])


class OutlierGroups:
    """outlier_groups' result: V, src, dst, labels (the community labelling, an input),
    comm (community index per vertex), names, sizes (the catalogue, by community index),
    atom_size (size of each vertex's sub-group), clique_min (the clique's smallest id, own
    id outside cliques), partner (the pair partner, own id elsewhere), order (vertex ids in
    construction order: communities, and inside them cliques, are consecutive stretches),
    atom_start (positions in `order` where an atom begins)."""

    def sub_labels(self, sub_iter):
        """Closed form of the second LPA's labels after sub_iter >= 2 supersteps."""
        assert sub_iter >= 2
        return (self.partner if sub_iter % 2 else self.clique_min).astype(np.int32)

    def closed_form(self):
        """flags, summary of mode L2 (any sub_iter >= 2) from the catalogue alone."""
        thr = np.array([threshold_of(sz) for sz in self.sizes])
        flags = self.atom_size < thr[self.comm]
        summ = dict(n_communities=len(self.sizes), n_subgroups=sum(len(sz) for sz in self.sizes),
                    n_flagged=int(flags.sum()), n_communities_flagged=int(np.unique(self.comm[flags]).size))
        return flags, summ


def outlier_groups(big=True, pad_pow2=True, seed=5, n_cross=4000, n_dup=3000):
    """Communities chosen directly as an input labelling, each a disjoint union of cliques
    of prescribed sizes plus vertices that stay alone, so every community's multiset of
    sub-group sizes -- and with it its threshold and its flagged groups -- is known.

    A clique of n >= 3 has every pair joined one-directionally (random orientation) or every
    pair reciprocally (two directed edges), never mixed: after superstep 1 of the second LPA
    its smallest vertex holds the second-smallest id and every other the smallest, from
    superstep 2 on all hold the smallest.  Two self-loops (on the second-smallest and the
    largest member) in every third clique of n >= 8 change superstep 1 only.  A pair swaps
    labels every superstep (two groups of size 1), an edgeless vertex keeps its id.
    Duplicated edges (deduplicated by the stage) and n_cross edges between communities (E'
    drops them, `incident` counts them) are added, the ids scrambled, the edges shuffled.
    Community label values are member ids: the smallest for even communities, the largest
    for odd ones and for the community of vertex V - 1.

    big: the cliques of 1,100 (one-directional: 1,099 arcs per row) and 2,100 (reciprocal:
    4,198) members; otherwise every clique above 300 shrinks 20-fold (CPU-sized).
    pad_pow2: one more community of edgeless vertices brings V to a power of two."""
    rng = np.random.default_rng(seed)
    cat = [(name, [s if big or s <= 300 else s // 20 for s in sizes]) for name, sizes in OUTLIER_CATALOGUE]
    n0 = sum(sum(sz) for _, sz in cat)
    if pad_pow2:
        V = 1 << int(n0 - 1).bit_length()
        if V - n0 > 0:
            cat.append(("pad_singles", [1] * (V - n0)))
    V = sum(sum(sz) for _, sz in cat)
    perm = rng.permutation(V).astype(np.int64)
    comm = np.empty(V, np.int64)
    atom_size = np.empty(V, np.int64)
    clique_min = np.arange(V, dtype=np.int64)
    partner = np.arange(V, dtype=np.int64)
    atom_start = []
    es, ed = [], []
    nxt = 0
    n_clique = 0
    for c, (name, sizes) in enumerate(cat):
        singles = []
        for s in sizes:
            ids = perm[nxt:nxt + s]
            comm[ids] = c
            atom_size[ids] = s
            atom_start.append(nxt)
            nxt += s
            if s == 1:
                singles.append(int(ids[0]))
                continue
            assert s >= 3
            iu, ju = np.triu_indices(s, 1)
            a, b = ids[iu], ids[ju]
            reciprocal = s == 2100 or (s != 1100 and n_clique % 2 == 1)
            if reciprocal:
                es += [a, b]
                ed += [b, a]
            else:
                flip = rng.random(a.size) < 0.5
                es.append(np.where(flip, b, a))
                ed.append(np.where(flip, a, b))
            srt = np.sort(ids)
            clique_min[ids] = srt[0]
            partner[ids] = srt[0]
            if s >= 8 and n_clique % 3 == 0:
                loops = np.array([srt[1], srt[-1]])
                es.append(loops)
                ed.append(loops)
            n_clique += 1
        # half of an even community's lone vertices (a quarter of an odd one's) pair up
        n_pairs = 0 if name == "pad_singles" else len(singles) // (4 if c % 2 else 2)
        for i in range(n_pairs):
            u, w = singles[2 * i], singles[2 * i + 1]
            es.append(np.array([u]))
            ed.append(np.array([w]))
            partner[u], partner[w] = w, u
    assert nxt == V
    s = np.concatenate(es)
    d = np.concatenate(ed)
    dup = rng.integers(0, s.size, size=n_dup)
    cs = rng.integers(0, V, size=4 * n_cross)
    cd = rng.integers(0, V, size=4 * n_cross)
    keep = np.flatnonzero(comm[cs] != comm[cd])[:n_cross]
    assert keep.size == n_cross
    cs, cd = cs[keep], cd[keep]
    s = np.concatenate([s, s[dup], cs, cd[:n_cross // 8], cs[:n_cross // 8]])
    d = np.concatenate([d, d[dup], cd, cs[:n_cross // 8], cd[:n_cross // 8]])
    sh = rng.permutation(s.size)
    f = OutlierGroups()
    f.V, f.src, f.dst = V, s[sh].astype(np.int32), d[sh].astype(np.int32)
    lo = np.full(len(cat), V, np.int64)
    hi = np.full(len(cat), -1, np.int64)
    np.minimum.at(lo, comm, np.arange(V))
    np.maximum.at(hi, comm, np.arange(V))
    use_max = (np.arange(len(cat)) % 2 == 1) | (np.arange(len(cat)) == comm[V - 1])
    f.labels = np.where(use_max, hi, lo)[comm].astype(np.int32)
    f.comm, f.atom_size, f.clique_min, f.partner = comm, atom_size, clique_min, partner
    f.names = [name for name, _ in cat]
    f.sizes = [list(sz) for _, sz in cat]
    f.order = perm
    f.atom_start = np.array(atom_start, dtype=np.int64)
    return f


def sub_edges(src, dst, labels, V):
    """E' of mode L2, restated in numpy: the distinct directed (s, d) with equal labels."""
    lab = np.asarray(labels)
    key = np.unique(src.astype(np.int64) * V + dst.astype(np.int64))
    ks, kd = key // V, key % V
    m = lab[ks] == lab[kd]
    return ks[m].astype(np.int32), kd[m].astype(np.int32)


def outlier_l1_np(V, src, dst, labels, key=None):
    """Mode L1 restated in numpy: np.bincount for the sizes, np.unique over int64 s * V + d
    keys for the distinct edges (key: those keys, if the caller kept them).
    Returns size, incident, flags, summary."""
    lab = np.asarray(labels).astype(np.int64)
    size = np.bincount(lab, minlength=V)
    if key is None:
        key = np.unique(np.asarray(src).astype(np.int64) * V + np.asarray(dst).astype(np.int64))
    ls, ld = lab[key // V], lab[key % V]
    inc = np.bincount(ls, minlength=V) + np.bincount(ld[ld != ls], minlength=V)
    groups = size[size > 0]
    thr = threshold_of(groups)
    flags = size[lab] < thr
    return size, inc, flags, dict(n_groups=int(groups.size), k=int(groups.size // 10), thr=thr,
                                  n_flagged=int(flags.sum()))


def coarse_labels(f, sizes):
    """A labelling of f's V vertices with the given group sizes (they sum to V): consecutive
    stretches of the construction order, i.e. the fixture's cliques and communities merged
    (a stretch may end inside a clique).  Label value: the stretch's smallest member id for
    even groups, its largest for odd ones."""
    assert sum(sizes) == f.V
    lab = np.empty(f.V, np.int32)
    at = 0
    for i, n in enumerate(sizes):
        ids = f.order[at:at + n]
        lab[ids] = ids.max() if i % 2 else ids.min()
        at += n
    return lab


def coarse_family(V):
    """Group-size lists for coarse_labels with the threshold rule's decision on an edge:
    n groups on both sides of every multiple of 10 in reach, the sizes around position
    k = n // 10 of the ascending order tied or one apart.  Every list is an engineered
    prefix, groups of 6, and one last group with the rest of the V vertices.
    Returns [(name, sizes, dict(n_groups, k, thr, n_flagged))], the dict written down from
    the rule (k-th smallest, strict <), not computed by code under test."""
    out = []

    def case(name, n, prefix, thr, n_flagged):
        mid = [6] * (n - len(prefix) - 1)
        rest = V - sum(prefix) - sum(mid)
        assert rest > 16 and len(prefix) + len(mid) + 1 == n
        out.append((f"n{n}_{name}", prefix + mid + [rest],
                    dict(n_groups=n, k=n // 10, thr=rest if thr is None else thr, n_flagged=n_flagged)))

    case("all_one", 1, [], None, 0)
    # k = 0: the largest size is the threshold, every other group is flagged
    case("distinct", 9, [2, 3, 4, 5, 7, 8, 9, 10], None, 48)
    case("flat", 9, [6] * 8, None, 48)
    for n in (10, 11, 19, 20, 21, 99, 100, 101):
        k = n // 10
        case("kth_unique", n, [2] * (k - 1) + [3, 4], 3, 2 * (k - 1))      # position k alone at 3
        case("tie_k_k1", n, [2] * (k - 1) + [3, 3], 3, 2 * (k - 1))        # positions k, k + 1 tied
        case("tie_km1_k", n, [2] * k + [3], 2, 0)                          # positions k - 1 (if any), k tied
        case("flat", n, [], 6, 0)                                          # every size but the last equal
        if k >= 2:
            case("run_straddles", n, [2] * (k - 2) + [3] * 4, 3, 2 * (k - 2))   # positions k - 1 .. k + 2
    return out


def bh_home_slot(labels):
    """BlockHist's home slot (lpa_device.h lds_add): the top 12 bits of label * 0x9E3779B1."""
    return (_mul32(labels, 0x9E3779B1) >> np.uint64(20)).astype(np.int64)


BH_PROBES = 8   # lpa_device.h kBhProbes


def bh_saturating_labels(V=65536, block=37, heavy_blocks=6, seed=3):
    """V labels (position i is element i of the kernel's input) that overflow one block's
    BlockHist for certain.  The home slot shared by the most label values of [0, V) is
    found; all but one of its labels (>= 12, asserted) stand, twice each, at the start of
    the 256-element stretch of `block` -- more distinct keys than the BH_PROBES slots a key
    of that home slot may probe, so at least 4 of them fail every probe whatever the thread
    order, set `sat` and go to the device histogram directly; the stretch's other elements
    (random labels, and the heavy one) then probe their home slot only.  The last label of
    the slot, the heavy one, fills the rest of the stretch's first half and the following
    heavy_blocks stretches; every other position holds a random label.
    Returns labels, the colliding labels, the heavy label."""
    rng = np.random.default_rng(seed)
    slot = bh_home_slot(np.arange(V))
    best = int(np.argmax(np.bincount(slot, minlength=4096)))
    same = np.flatnonzero(slot == best)
    assert same.size >= 13, same.size
    rng.shuffle(same)
    heavy, coll = int(same[0]), same[1:]
    assert coll.size >= 12 > BH_PROBES
    lab = rng.integers(0, V, size=V)
    at = 256 * block
    assert at + 256 * (heavy_blocks + 1) <= V and 2 * coll.size <= 128
    lab[at:at + 2 * coll.size] = np.repeat(coll, 2)
    lab[at + 2 * coll.size:at + 128] = heavy
    lab[at + 256:at + 256 * (heavy_blocks + 1)] = heavy
    return lab.astype(np.int32), coll.astype(np.int32), heavy


# ---- the label exchange's gadgets (tests/exchange_ref.py, tests/test_gpu_exchange_edges.py) ----
class Gadgets:
    """Disjoint union of small gadgets on consecutive ids, each with a label history known in
    closed form (input edges are undirected votes, parallel edges count): they put chosen
    numbers of changed labels at chosen supersteps.  Every method files the ids it makes under
    `groups[name]`.  The first gadget of every fixture is the core clique on ids 0..c-1, so
    that label 0 is the giant label."""

    def __init__(self):
        self.n = 0
        self.s, self.d = [], []
        self.groups = {}

    def ids(self, k, name):
        a = np.arange(self.n, self.n + k, dtype=np.int64)
        self.n += k
        self.groups[name] = np.concatenate([self.groups[name], a]) if name in self.groups else a
        return a

    def edges(self, a, b, mult=1):
        self.s.append(np.repeat(np.asarray(a, dtype=np.int64).ravel(), mult))
        self.d.append(np.repeat(np.asarray(b, dtype=np.int64).ravel(), mult))

    def clique(self, c, mult=1, name="still"):
        """c >= 3 vertices, every pair joined: superstep 1 gives (second smallest id, smallest,
        smallest, ...), from superstep 2 on every vertex holds the smallest id for ever."""
        v = self.ids(c, name)
        iu, ju = np.triu_indices(c, 1)
        self.edges(v[iu], v[ju], mult)
        return v

    def blinkers(self, pairs, mult=1, name="blink"):
        """Two vertices and `mult` parallel edges: they swap labels in every superstep for
        ever (2 changes per pair per superstep, both labels distinct from every other)."""
        v = self.ids(2 * pairs, name).reshape(pairs, 2)
        self.edges(v[:, 0], v[:, 1], mult)
        return v

    def paths3(self, k, mult=1, name="blink"):
        """Paths a - b - c (ids ascending): (b, a, b), (a, b, a), ... -- three changes per path
        per superstep for ever; the middle vertex has twice the ends' degree."""
        v = self.ids(3 * k, name).reshape(k, 3)
        self.edges(v[:, 0], v[:, 1], mult)
        self.edges(v[:, 1], v[:, 2], mult)
        return v

    def isolated(self, k, name="iso"):
        return self.ids(k, name)

    def still(self, k, mult=1, name="still"):
        """k vertices (k = 3, 4 or >= 6) in cliques of 4 (k % 3 of them) and 3: each settled on
        its smallest id from superstep 2 on."""
        assert k in (0, 3, 4) or k >= 6, k
        n4 = k % 3
        for c, n in ((4, n4), (3, (k - 4 * n4) // 3)):
            v = self.ids(c * n, name).reshape(n, c)
            iu, ju = np.triu_indices(c, 1)
            self.edges(v[:, iu], v[:, ju], mult)

    def build(self, pad_to=0):
        if pad_to > self.n:
            self.isolated(pad_to - self.n)
        s = np.concatenate(self.s) if self.s else np.zeros(0, np.int64)
        d = np.concatenate(self.d) if self.d else np.zeros(0, np.int64)
        return self.n, s.astype(np.int32), d.astype(np.int32), self.groups


def blinker_field(V, pairs=0, paths=0, core=4, core_mult=1):
    """Core clique (ids 0..core-1, all label 0 from superstep 2 on; core_mult parallel edges per
    pair: with enough of them the blinkers dirty <= 0.5 % of a rank's arcs and the converged
    tallies walk their frontier lists), `pairs` blinker pairs, `paths` three-vertex blinker
    paths, isolated vertices up to V ids: from superstep 3 on exactly 2 pairs + 3 paths labels
    change per superstep, none of them to label 0."""
    g = Gadgets()
    g.clique(core, mult=core_mult, name="core")
    if pairs:
        g.blinkers(pairs)
    if paths:
        g.paths3(paths)
    assert g.n <= V, (g.n, V)
    return g.build(pad_to=V)


def fuse_broom(n, D, c=16, share=1, blink=0, pad_to=0, tri_mult=2, ballast=0):
    """A timed burst of n changes.  Core clique on ids 0..c-1; ceil(n / share) triangles with
    every edge tri_mult-fold (each settles on its smallest id T_i; 2 tri_mult > share, so the
    leaves never outvote it); n leaves, each with one edge to a triangle's first vertex (`share`
    leaves per triangle) and one to the hub; `blink` blinker pairs; isolated ids up to pad_to;
    then, on the largest ids, a fuse: a path of D vertices from core vertex 0 to the hub, every
    hop n + 1 parallel edges.  The hub repeats the fuse's end one superstep late and the leaves
    follow the hub when its label is below their T_i: they are still from superstep 4 through
    D + 1 and all n change in every superstep from D + 2 on (to label 0 at D + 2, D + 4, ...).
    The fuse, the hub and core vertex 0 (n + 1 fuse votes against its c - 1 core votes) blink
    throughout.  ballast: a settled 4-clique of that many parallel edges per pair, whose arcs
    keep the dirty ones below 0.5 % of a rank's, so that the converged tallies walk their lists."""
    assert 2 * tri_mult > share >= 1 and D >= 1
    g = Gadgets()
    core = g.clique(c, name="core")
    if ballast:
        g.clique(4, mult=ballast, name="ballast")
    ntri = -(-n // share)
    tri = g.ids(3 * ntri, "tri").reshape(ntri, 3)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        g.edges(tri[:, a], tri[:, b], tri_mult)
    leaves = g.ids(n, "leaves")
    g.edges(leaves, tri[np.arange(n) // share, 0])
    if blink:
        g.blinkers(blink)
    if pad_to > g.n + D + 1:
        g.isolated(pad_to - (g.n + D + 1))
    fuse = g.ids(D, "fuse")
    hub = g.ids(1, "hub")
    g.edges(leaves, np.full(n, hub[0]))
    chain = np.concatenate([core[:1], fuse, hub])
    g.edges(chain[:-1], chain[1:], n + 1)
    return g.build()


def odd_slice_field(P, slice_):
    """V = P * slice_ vertices, none isolated, for the tight slices (P = 3, or LPA_POW2_SLICES=0):
    in the plain order (degree descending, id ascending; degree rank k at slot k // P of rank
    k % P) the blinking vertices hold slots 0, 63, 64 and slice_ - 1 of every rank and the
    vertices between them are settled cliques, the core among them (ids 0..7)."""
    assert slice_ % 64 == 0 and slice_ >= 192 and P in (2, 3, 4)
    g = Gadgets()
    g.clique(8, mult=4, name="core")                        # degree 28
    if P == 3:
        g.paths3(1, mult=100, name="top")                   # degrees 100, 200, 100: ranks 0..2
    else:
        g.blinkers(P // 2, mult=100, name="top")            # degree 100: ranks 0..P-1
    g.still(63 * P - P - 8, mult=10, name="still_a")        # degrees 20 / 30: up to rank 63 P
    g.blinkers(P, mult=10, name="mid")                      # ranks 63 P .. 65 P - 1: slots 63, 64
    tail = 5 if P == 3 else P                               # P = 3: a path (middle: degree 2) + a pair
    g.still(P * slice_ - 65 * P - tail, mult=2, name="still_b")   # degrees 4 / 6
    if P == 3:
        g.paths3(1, name="tail")
        g.blinkers(1, name="tail")
    else:
        g.blinkers(P // 2, name="tail")
    assert g.n == P * slice_
    return g.build()
