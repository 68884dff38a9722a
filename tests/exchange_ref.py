"""Host restatement of the multi-rank label exchange's decisions (csrc/lpa_exchange.hip), in
plain numpy: from the oracle's label history and the slot map, what every rank compacts in
every superstep, the gathered capacities, the form `exchange_collective` must take and the
next posted capacity.  No GPU, nothing imported from the library.

Where every constant comes from (csrc/, at the commit that added this file):
  lpa_build.hip:779-793      slice = ceil(V / P) rounded up to 64, at least 64; a power of two
                             when P is one (and LPA_POW2_SLICES is not 0); vpad = P * slice
  lpa_build.hip:73-78,135-143  the plain order: key (maxdeg - deg) << 32 | id ascending, degree
                             rank k at slot (k % P) * slice + k / P
  lpa_build.hip:369-377      L0: a slot holds its vertex id, a padding slot 0
  lpa_refresh.hip:502-538    k_giant_pick: kPickK = 1024 top degree ranks, best word
                             (count << 32 | ~label): most frequent label, the smaller on a tie
  lpa_exchange.hip:98-100    kCompactWords = 8, kTriple = 3, kNoGiantForm = 2^62
  lpa_exchange.hip:119-120   converged and the tally walked its lists: no giant form
  lpa_exchange.hip:308-309   dcap = max(1, slice / 4)
  lpa_exchange.hip:373-390   kPostMin = 1024, kPostMax = 2^17, posted_cap, agreed_post_cap
  lpa_exchange.hip:402,426-485  superstep 1 full; the posted delta; delta_b <= giant_b and
                             delta_b < full_b; giant_b < full_b; else full
  lpa_schedule.h:112, lpa_internal.h:35  converged_now: superstep kDenseSupersteps + 3 = 5 on
  lpa_internal.h:69, lpa_refresh.hip:373-374,1806  a rank's next tally walks its lists unless
                             more than (int64)(kFrontierFrac * arcs) of its arcs are dirty
                             (kFrontierFrac = 0.005; dirty: the arcs of the rank's rows whose
                             column changed, k_delta_finish / k_diff counters[1])
  lpa_refresh.hip:1745, lpa_build.hip:462  a rank without arcs refreshes nothing: its
                             "tally every row" flag stays 1 from L0 on
"""
import functools

import numpy as np

import graphs as _g

K_PICK = 1024
K_POST_MIN, K_POST_MAX = 1024, 1 << 17
K_FRONTIER_FRAC = 0.005
CONVERGED_FROM = 5          # first converged superstep
FORMS = ("full", "delta", "giant", "posted", "post_missed")   # lpa_graph_info.exchanges_*


def slice_of(V, P, pow2=True):
    s = (V + P - 1) // P
    s = (s + 63) // 64 * 64
    if s == 0:
        s = 64
    if P > 1 and P & (P - 1) == 0 and pow2:
        n = 64
        while n < s:
            n *= 2
        if n * P <= 1 << 30:
            s = n
    return s


def plain_order(V, src, dst):
    """Vertex ids by degree descending, id ascending (the symmetrised degree: both ends of
    every input edge, a self-loop twice)."""
    deg = np.bincount(src, minlength=V) + np.bincount(dst, minlength=V)
    return np.lexsort((np.arange(V), -deg)), deg


class SlotMap:
    """slice, vpad, slot_of[v] (global slot), old_of[slot] (-1: padding), order."""

    def __init__(self, V, P, slice_, order):
        self.V, self.P, self.slice, self.vpad = V, P, slice_, P * slice_
        self.order = np.asarray(order, dtype=np.int64)
        k = np.arange(V, dtype=np.int64)
        self.slot_of = np.empty(V, np.int64)
        self.slot_of[self.order] = (k % P) * slice_ + k // P
        self.old_of = np.full(self.vpad, -1, np.int64)
        self.old_of[self.slot_of] = np.arange(V)
        self.rank_of = self.slot_of // slice_
        self.local = self.slot_of % slice_

    def l0_slices(self):
        """What exchange_get() returns on every rank right after reset(): (P, slice)."""
        return np.where(self.old_of >= 0, self.old_of, 0).reshape(self.P, self.slice).astype(np.int32)


def restated_map(V, src, dst, P, pow2=True):
    order, _ = plain_order(V, src, dst)
    return SlotMap(V, P, slice_of(V, P, pow2), order)


def map_from_l0(V, P, l0_slices, zero_slot):
    """The slot map read back from the library: row r of l0_slices is rank r's exchange_get()
    after reset().  A slot holds its vertex id and a padding slot 0 (init_labels), so vertex 0
    cannot be told from padding: its slot is given (the restated one) and must hold 0.
    Asserts that every real vertex occurs exactly once over the ranks."""
    l0 = np.asarray(l0_slices)
    slice_ = l0.shape[1]
    flat = l0.reshape(-1).astype(np.int64)
    assert flat[zero_slot] == 0
    assert flat.min() >= 0 and flat.max() < V
    cnt = np.bincount(flat, minlength=V)
    assert np.all(cnt[1:] == 1), "a vertex id occurs twice or never over the ranks"
    assert cnt[0] == flat.size - (V - 1), "padding slots hold 0"
    slot_of = np.empty(V, np.int64)
    nz = np.flatnonzero(flat)
    slot_of[flat[nz]] = nz
    slot_of[0] = zero_slot
    k = (slot_of % slice_) * P + slot_of // slice_       # degree rank of every vertex
    order = np.argsort(k)
    assert np.array_equal(np.sort(k), np.arange(V)), "real vertices do not fill the first ranks"
    return SlotMap(V, P, slice_, order)


def giant_pick(L, order):
    """k_giant_pick of the label vector L: (G, unambiguous) -- unambiguous when G holds
    strictly more of the top min(V, 1024) degree ranks than any other label."""
    top = np.asarray(L)[order[:K_PICK]]
    if top.size == 0:
        return 0, True
    lab, cnt = np.unique(top, return_counts=True)
    best = cnt.max()
    return int(lab[cnt == best].min()), int((cnt == best).sum()) == 1


def posted_cap(capd, dcap):
    c = K_POST_MIN
    while c < 2 * capd:
        c *= 2
    return c if c <= K_POST_MAX and c <= dcap else 0


def agreed_post_cap(capd, dcap, requests):
    return min(posted_cap(capd, dcap) if q < 0 else min(q, dcap) for q in requests)


def choose(capd, capg, slice_, dcap):
    """The form of fewest bytes among those that fit (exchange_collective)."""
    inf = float("inf")
    full_b = 4 * slice_
    delta_b = 8 * capd if capd <= dcap else inf
    giant_b = 8 * (slice_ // 64) + 8 * capg if capg <= dcap else inf
    if delta_b <= giant_b and delta_b < full_b:
        return "delta"
    if giant_b < full_b:
        return "giant"
    return "full"


class Step:
    """One superstep of the restatement: G, changed[r] = (local slots, labels) sorted by slot,
    nd[r] / ng[r] (the ranks' delta / non-G counts), capd, capg, giant_offered, post (the
    capacity posted before the counts were read, 0: none), counters (the differences of
    exchanges_full / _delta / _giant / _posted / _post_missed), form, post_cap_next."""

    def entries(self, r):
        """Rank r's delta entries as k_delta_compact packs them, sorted."""
        sl, lab = self.changed[r]
        return np.sort((sl.astype(np.uint64) << np.uint64(32)) | lab.astype(np.uint32).astype(np.uint64))

    @property
    def letter(self):
        f = {"full": "F", "delta": "D", "giant": "G"}[self.form]
        if self.counters[3]:
            return "P"
        return f.lower() if self.counters[4] else f


def restate(V, src, dst, hist, smap, requests=None):
    """hist: the oracle's (T, V) label history.  requests: every rank's lpa_set_posted value
    (-1 adaptive, the default).  Returns a list of T Steps."""
    P, S = smap.P, smap.slice
    dcap = max(1, S // 4)
    requests = [-1] * P if requests is None else list(requests)
    assert len(requests) == P
    # arcs of rank r's rows whose column is u: the input edges (u, v) with v owned by r
    s64, d64 = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    cnt = (np.bincount(smap.rank_of[d64] * V + s64, minlength=P * V) +
           np.bincount(smap.rank_of[s64] * V + d64, minlength=P * V)).reshape(P, V)
    arcs = cnt.sum(axis=1)
    fr_thr = (K_FRONTIER_FRAC * arcs.astype(np.float64)).astype(np.int64)
    prev = np.arange(V, dtype=np.int64)
    prev_delta_ok, post_cap = False, 0
    fr_all = np.ones(P, bool)
    steps = []
    for t in range(1, hist.shape[0] + 1):
        new = np.asarray(hist[t - 1], np.int64)
        st = Step()
        st.t = t
        st.G, st.g_unambiguous = giant_pick(prev, smap.order)
        chg = np.flatnonzero(new != prev)
        st.changed, st.nd, st.ng = [], [], []
        for r in range(P):
            mine = chg[smap.rank_of[chg] == r]
            mine = mine[np.argsort(smap.local[mine])]
            st.changed.append((smap.local[mine], new[mine].astype(np.int32)))
            st.nd.append(int(mine.size))
            st.ng.append(int((new[mine] != st.G).sum()))
        st.capd = max(st.nd)
        st.walked = [bool(t >= CONVERGED_FROM and not fr_all[r]) for r in range(P)]
        st.giant_offered = not any(st.walked)
        st.capg = max(st.ng) if st.giant_offered else 1 << 62
        c = [0, 0, 0, 0, 0]
        st.post = 0
        if t == 1:
            st.form = "full"
        else:
            st.post = post_cap if prev_delta_ok else 0
            if st.post > 0 and st.capd <= st.post:
                st.form = "delta"
                c[3] = 1
            else:
                c[4] = 1 if st.post > 0 else 0
                st.form = choose(st.capd, st.capg, S, dcap)
        c[FORMS.index(st.form)] += 1
        if st.form == "delta":
            post_cap = agreed_post_cap(st.capd, dcap, requests)
            prev_delta_ok = True
        else:
            prev_delta_ok = False
        st.counters = tuple(c)
        st.post_cap_next = post_cap
        # the refresh: which ranks tally every row next
        dirty = cnt[:, chg].sum(axis=1)
        fr_all = (dirty > fr_thr) | (arcs == 0)
        steps.append(st)
        prev = new
    return steps


def letters(steps):
    return "".join(s.letter for s in steps)


# ---- the fixtures of tests/test_exchange_fixtures_host.py and tests/test_gpu_exchange_edges.py ----
# One entry per GPU case: name -> (builder of (V, src, dst, groups), P, pow2 slices, every rank's
# lpa_set_posted request or None).  EXPECT holds what each was built for, written down from the
# rule and the gadgets' closed forms: the forms of supersteps 1..10 (F full, D delta, G giant, P a
# posted delta that was taken, a lower-case letter the form that followed a posted delta that
# missed), then capd and capg of supersteps 2..10 (capg -1: no giant form, the converged
# compaction walked a frontier list).  The host test asserts them against the oracle's history;
# the GPU test asserts them again with the slot map read back, then the library's counters.
def _bf(V, **kw):
    return functools.partial(_g.blinker_field, V, **kw)


def _fb(n, D, **kw):
    return functools.partial(_g.fuse_broom, n, D, **kw)


CASES = {}
for _P in (2, 4):
    for _k in (-1, 0, 1):
        # largest per-rank count dcap - 1, dcap, dcap + 1 (dcap = 16 and 1024)
        CASES[f"dcap_s64_P{_P}_{_k:+d}"] = (_bf(64 * _P, pairs=(16 + _k) * _P // 2), _P, True, None)
        CASES[f"dcap_s4096_P{_P}_{_k:+d}"] = (_bf(4096 * _P, pairs=(1024 + _k) * _P // 2), _P, True, None)
# the same at slice 64 with a core heavy enough that the converged tallies walk their lists
CASES["dcap_lists_s64_+0"] = (_bf(128, pairs=16, core=16, core_mult=40), 2, True, None)
CASES["dcap_lists_s64_+1"] = (_bf(128, pairs=17, core=16, core_mult=40), 2, True, None)
# uneven ranks: counts of 0 beside counts of 1, ranks without a real vertex
CASES["uneven_P4_V70_pair"] = (_bf(70, pairs=1), 4, True, None)
CASES["uneven_P8_V70_path"] = (_bf(70, paths=1), 8, True, None)
CASES["uneven_P8_V5_pair"] = (_bf(5, pairs=1, core=3), 8, True, None)
CASES["uneven_P4_V7_path"] = (_bf(7, paths=1), 4, True, None)
# delta_b <= giant_b: capd == capg + slice / 64 (delta) and one more (giant); posting off, or the
# posted delta of superstep 3 would pre-empt the choice
CASES["tie_D1_n127"] = (_fb(127, 1, pad_to=4200), 2, True, [0, 0])
CASES["tie_D1_n128"] = (_fb(128, 1, pad_to=4200), 2, True, [0, 0])
CASES["tie_D2_n128"] = (_fb(128, 2, pad_to=4200), 2, True, [0, 0])
CASES["tie_D2_n129"] = (_fb(129, 2, pad_to=4200), 2, True, [0, 0])
# capg == dcap fits the giant form, dcap + 1 does not (capd is above dcap in both)
CASES["capg_dcap"] = (_fb(128, 1, blink=1023, pad_to=4200), 2, True, [0, 0])
CASES["capg_dcap+1"] = (_fb(128, 1, blink=1024, pad_to=4200), 2, True, [0, 0])
# a burst in the converged supersteps: above dcap per rank (lists walked: full; slice walked:
# giant and full in turn), and just below it (delta throughout)
CASES["rise_lists_D4"] = (_fb(36, 4, c=8, share=3, ballast=10000), 2, True, None)
CASES["rise_lists_D6"] = (_fb(36, 6, c=8, share=3, ballast=10000), 2, True, None)
CASES["rise_lists_below_D4"] = (_fb(24, 4, c=8, share=3, ballast=10000), 2, True, None)
CASES["rise_lists_below_D6"] = (_fb(24, 6, c=8, share=3, ballast=10000), 2, True, None)
CASES["rise_slice_D4"] = (_fb(28, 4, c=8, share=3), 2, True, None)
CASES["rise_slice_D6"] = (_fb(28, 6, c=8, share=3), 2, True, None)
# a pulse: a core above n + 1 vertices keeps core vertex 0 settled, so the fuse carries one wave
# (0, 1, 0) and settles; the leaves change in supersteps D + 2 .. D + 4 only -- delta, full (giant
# and full where the slice was walked), delta again, and then deltas of no entry at all
CASES["pulse_lists_D4"] = (_fb(36, 4, c=40, share=3, ballast=10000), 2, True, None)
CASES["pulse_lists_D5"] = (_fb(36, 5, c=40, share=3, ballast=10000), 2, True, None)
CASES["pulse_slice_D4"] = (_fb(36, 4, c=40, share=3), 2, True, None)
# posted capacity c: taken at a largest count of c, missed at c + 1
CASES["posted_16_+0"] = (_bf(8192, pairs=16), 2, True, [16, 16])
CASES["posted_16_+1"] = (_bf(8192, pairs=17), 2, True, [16, 16])
CASES["posted_1024_+0"] = (_bf(16384, pairs=1024), 2, True, [1024, 1024])
CASES["posted_1024_+1"] = (_bf(16384, pairs=1025), 2, True, [1024, 1024])
# one rank alone requests the smaller capacity: the smallest request wins on every rank
CASES["posted_one_rank_P2"] = (_bf(8192, pairs=17), 2, True, [-1, 16])
CASES["posted_one_rank_P4"] = (_bf(16384, pairs=34), 4, True, [-1, -1, 16, -1])
# what follows a miss: a delta where the burst fits dcap, a full exchange where it does not
CASES["posted_miss_delta"] = (_fb(36, 6, c=8, share=3, ballast=10000, pad_to=4200), 2, True, [16, 16])
CASES["posted_miss_full"] = (_fb(36, 6, c=8, share=3, ballast=10000), 2, True, [8, 8])
# adaptive: the capacity falls to 1,024 while 4 labels change, the burst doubles past it
CASES["posted_adaptive_burst"] = (_fb(2100, 6, share=3, pad_to=17000), 2, True, None)
# tight slices: P = 3, and LPA_POW2_SLICES=0 at P = 2; no multiple of 512 slots, V = P * slice
CASES["odd_P3_s192"] = (functools.partial(_g.odd_slice_field, 3, 192), 3, False, None)
CASES["odd_P2_s576"] = (functools.partial(_g.odd_slice_field, 2, 576), 2, False, None)
CASES["odd_P2_s4160"] = (functools.partial(_g.odd_slice_field, 2, 4160), 2, False, None)

# k_delta_compact directly, on caller-driven ranks: (fixture, P, pow2 slices, the per-rank change counts of every superstep from 3 on)
COMPACT = {
    "one_and_none": (lambda: _g.blinker_field(200, pairs=1), 4, True, [1, 1, 0, 0]),
    "255": (lambda: _g.blinker_field(4096, pairs=255), 2, True, [255, 255]),
    "256": (lambda: _g.blinker_field(4096, pairs=256), 2, True, [256, 256]),
    "257": (lambda: _g.blinker_field(4096, pairs=257), 2, True, [257, 257]),
    # 4,096 blocks of 256 slots take 2^20 slots a trip: the last 64 slots are the second trip's,
    # and the tail blinkers sit in the last slot of every rank
    "second_trip": (lambda: _g.odd_slice_field(2, (1 << 20) + 64), 2, False, [4, 4]),
}

N_STEPS = 10

EXPECT = {
    "dcap_s64_P2_-1": ("FDDDDDDDDD", (16, 15, 15, 15, 15, 15, 15, 15, 15),
        (15, 15, 15, 15, 15, 15, 15, 15, 15)),
    "dcap_s4096_P2_-1": ("FDDDDDDDDD", (1024, 1023, 1023, 1023, 1023, 1023, 1023, 1023, 1023),
        (1023, 1023, 1023, 1023, 1023, 1023, 1023, 1023, 1023)),
    "dcap_s64_P2_+0": ("FGDDDDDDDD", (17, 16, 16, 16, 16, 16, 16, 16, 16),
        (16, 16, 16, 16, 16, 16, 16, 16, 16)),
    "dcap_s4096_P2_+0": ("FGDDDDDDDD", (1025, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024),
        (1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024)),
    "dcap_s64_P2_+1": ("FFFFFFFFFF", (18, 17, 17, 17, 17, 17, 17, 17, 17),
        (17, 17, 17, 17, 17, 17, 17, 17, 17)),
    "dcap_s4096_P2_+1": ("FFFFFFFFFF", (1026, 1025, 1025, 1025, 1025, 1025, 1025, 1025, 1025),
        (1025, 1025, 1025, 1025, 1025, 1025, 1025, 1025, 1025)),
    "dcap_s64_P4_-1": ("FDDDDDDDDD", (16, 15, 15, 15, 15, 15, 15, 15, 15),
        (15, 15, 15, 15, 15, 15, 15, 15, 15)),
    "dcap_s4096_P4_-1": ("FDDDDDDDDD", (1024, 1023, 1023, 1023, 1023, 1023, 1023, 1023, 1023),
        (1023, 1023, 1023, 1023, 1023, 1023, 1023, 1023, 1023)),
    "dcap_s64_P4_+0": ("FGDDDDDDDD", (17, 16, 16, 16, 16, 16, 16, 16, 16),
        (16, 16, 16, 16, 16, 16, 16, 16, 16)),
    "dcap_s4096_P4_+0": ("FGDDDDDDDD", (1025, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024),
        (1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024)),
    "dcap_s64_P4_+1": ("FFFFFFFFFF", (18, 17, 17, 17, 17, 17, 17, 17, 17),
        (17, 17, 17, 17, 17, 17, 17, 17, 17)),
    "dcap_s4096_P4_+1": ("FFFFFFFFFF", (1026, 1025, 1025, 1025, 1025, 1025, 1025, 1025, 1025),
        (1025, 1025, 1025, 1025, 1025, 1025, 1025, 1025, 1025)),
    "dcap_lists_s64_+0": ("FGDDDDDDDD", (17, 16, 16, 16, 16, 16, 16, 16, 16),
        (16, 16, 16, -1, -1, -1, -1, -1, -1)),
    "dcap_lists_s64_+1": ("FFFFFFFFFF", (18, 17, 17, 17, 17, 17, 17, 17, 17),
        (17, 17, 17, -1, -1, -1, -1, -1, -1)),
    "uneven_P4_V70_pair": ("FDDDDDDDDD", (2, 1, 1, 1, 1, 1, 1, 1, 1),
        (1, 1, 1, -1, -1, -1, -1, -1, -1)),
    "uneven_P8_V70_path": ("FDDDDDDDDD", (1, 1, 1, 1, 1, 1, 1, 1, 1),
        (1, 1, 1, -1, -1, -1, -1, -1, -1)),
    "uneven_P8_V5_pair": ("FDDDDDDDDD", (1, 1, 1, 1, 1, 1, 1, 1, 1),
        (1, 1, 1, -1, -1, -1, -1, -1, -1)),
    "uneven_P4_V7_path": ("FDDDDDDDDD", (2, 1, 1, 1, 1, 1, 1, 1, 1),
        (1, 1, 1, -1, -1, -1, -1, -1, -1)),
    "tie_D1_n127": ("FDDDDDDDDD", (129, 65, 65, 65, 65, 65, 65, 65, 65),
        (128, 1, 64, 1, 64, 1, 64, 1, 64)),
    "tie_D1_n128": ("FDGDGDGDGD", (130, 66, 66, 66, 66, 66, 66, 66, 66),
        (129, 1, 65, 1, 65, 1, 65, 1, 65)),
    "tie_D2_n128": ("FDDDDDDDDD", (130, 66, 66, 66, 66, 66, 66, 66, 66),
        (130, 66, 2, 66, 2, 66, 2, 66, 2)),
    "tie_D2_n129": ("FDDGDGDGDG", (131, 67, 67, 67, 67, 67, 67, 67, 67),
        (131, 66, 2, 66, 2, 66, 2, 66, 2)),
    "capg_dcap": ("FFGFGFGFGF", (1153, 1089, 1089, 1089, 1089, 1089, 1089, 1089, 1089),
        (1152, 1024, 1088, 1024, 1088, 1024, 1088, 1024, 1088)),
    "capg_dcap+1": ("FFFFFFFFFF", (1154, 1090, 1090, 1090, 1090, 1090, 1090, 1090, 1090),
        (1153, 1025, 1089, 1025, 1089, 1025, 1089, 1025, 1089)),
    "rise_lists_D4": ("FFFDDFFFFF", (28, 21, 3, 3, 21, 21, 21, 21, 21),
        (28, 21, 3, -1, -1, -1, -1, -1, -1)),
    "rise_lists_D6": ("FFFDDDDFFF", (29, 22, 4, 4, 4, 4, 22, 22, 22),
        (29, 22, 4, -1, -1, -1, -1, -1, -1)),
    "rise_lists_below_D4": ("FFDDDDDDDD", (20, 15, 3, 3, 15, 15, 15, 15, 15),
        (20, 15, 3, -1, -1, -1, -1, -1, -1)),
    "rise_lists_below_D6": ("FFDDDDDDDD", (21, 16, 4, 4, 4, 4, 16, 16, 16),
        (21, 16, 4, -1, -1, -1, -1, -1, -1)),
    "rise_slice_D4": ("FFFDDGFGFG", (22, 17, 3, 3, 17, 17, 17, 17, 17),
        (22, 17, 3, 3, 3, 17, 3, 17, 3)),
    "rise_slice_D6": ("FFFDDDDGFG", (23, 18, 4, 4, 4, 4, 18, 18, 18),
        (23, 18, 4, 4, 4, 4, 4, 18, 4)),
    "pulse_lists_D4": ("FFFDDFFFDD", (28, 21, 2, 2, 19, 19, 18, 0, 0),
        (27, 20, 2, -1, -1, -1, -1, -1, -1)),
    "pulse_lists_D5": ("FFFDDDFFFD", (29, 21, 3, 2, 2, 19, 19, 18, 0),
        (27, 21, 2, -1, -1, -1, -1, -1, -1)),
    "pulse_slice_D4": ("FFFDDGFGDD", (27, 21, 2, 2, 19, 19, 18, 0, 0),
        (27, 20, 2, 1, 1, 18, 0, 0, -1)),
    "posted_16_+0": ("FDPPPPPPPP", (17, 16, 16, 16, 16, 16, 16, 16, 16),
        (16, 16, 16, 16, 16, 16, 16, 16, 16)),
    "posted_16_+1": ("FDdddddddd", (18, 17, 17, 17, 17, 17, 17, 17, 17),
        (17, 17, 17, 17, 17, 17, 17, 17, 17)),
    "posted_1024_+0": ("FDPPPPPPPP", (1025, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024),
        (1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024)),
    "posted_1024_+1": ("FDdddddddd", (1026, 1025, 1025, 1025, 1025, 1025, 1025, 1025, 1025),
        (1025, 1025, 1025, 1025, 1025, 1025, 1025, 1025, 1025)),
    "posted_one_rank_P2": ("FDdddddddd", (18, 17, 17, 17, 17, 17, 17, 17, 17),
        (17, 17, 17, 17, 17, 17, 17, 17, 17)),
    "posted_one_rank_P4": ("FDdddddddd", (18, 17, 17, 17, 17, 17, 17, 17, 17),
        (17, 17, 17, 17, 17, 17, 17, 17, 17)),
    "posted_miss_delta": ("FDdPPPPddd", (29, 22, 4, 4, 4, 4, 22, 22, 22),
        (29, 22, 4, -1, -1, -1, -1, -1, -1)),
    "posted_miss_full": ("FFFDPPPfFF", (29, 22, 4, 4, 4, 4, 22, 22, 22),
        (29, 22, 4, -1, -1, -1, -1, -1, -1)),
    "posted_adaptive_burst": ("FDPPPPPgDP", (1404, 1054, 4, 4, 4, 4, 1054, 1054, 1054),
        (1404, 1054, 4, 4, 4, 4, 4, 1054, 4)),
    "odd_P3_s192": ("FFDDDDDDDD", (130, 5, 5, 5, 5, 5, 5, 5, 5),
        (129, 5, 5, 5, 5, 5, 5, 5, 5)),
    "odd_P2_s576": ("FFDDDDDDDD", (195, 4, 4, 4, 4, 4, 4, 4, 4),
        (194, 4, 4, 4, 4, 4, 4, 4, 4)),
    "odd_P2_s4160": ("FFDPPPPPPP", (1390, 4, 4, 4, 4, 4, 4, 4, 4),
        (1389, 4, 4, 4, 4, 4, 4, 4, 4)),
}


@functools.lru_cache(maxsize=None)
def case_history(name):
    """(V, src, dst, groups, hist) of a case: built and run through the oracle once."""
    from oracle import oracle

    build, _, _, _ = CASES[name]
    V, s, d, groups = build()
    _, hist, _ = oracle.lpa(V, s, d, N_STEPS, per_iter=True)
    hist.setflags(write=False)
    return V, s, d, groups, hist


def check_precondition(name, steps, smap):
    """What a case was built for holds for these restated steps (a failure, never a skip)."""
    forms, capd, capg = EXPECT[name]
    assert smap.slice == slice_of(smap.V, smap.P, CASES[name][2])
    for st in steps[1:]:
        assert st.G == 0 and st.g_unambiguous, f"{name} superstep {st.t}: G is {st.G}, ambiguous or not the core's"
    got_d = tuple(st.capd for st in steps[1:])
    got_g = tuple(st.capg if st.giant_offered else -1 for st in steps[1:])
    assert got_d == capd, f"{name}: capd of supersteps 2.. {got_d}, built for {capd}"
    assert got_g == capg, f"{name}: capg of supersteps 2.. {got_g}, built for {capg}"
    assert letters(steps) == forms, f"{name}: forms {letters(steps)}, built for {forms}"
