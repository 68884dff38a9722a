"""The label exchange's forms at their thresholds, with built graphs (csrc/lpa_exchange.hip).

Every case of tests/exchange_ref.py CASES runs as a loopback group in one process: all ranks
step one superstep at a time for 10 supersteps, and after each superstep every rank's whole
replica equals the oracle's vector and the differences of its exchanges_full / _delta / _giant
/ _posted / _post_missed counters equal the form that the host restatement derives from the
oracle's history and the slot map read back from the library (exchange_get() after reset()).
Then reset() and run(10) give the same final vector.  tests/test_exchange_fixtures_host.py
asserts the same preconditions without a GPU.

k_delta_compact is compared with the restated entry set directly, on caller-driven ranks, at
0, 1, 255, 256 and 257 changes in one rank and in the second, partial trip of its grid-stride
loop (slice 2^20 + 64).

Not covered: the second trip of k_exch_compact's own grid (slices above 8 M slots: no
few-second test), and the RCCL and gloo transports, which have their jobs."""
import numpy as np
import pytest

import exchange_ref as X

pytestmark = pytest.mark.gpu

COUNTERS = tuple("exchanges_" + f for f in X.FORMS)


@pytest.fixture(scope="module")
def gfa():
    import graphframes_amd

    return graphframes_amd


def _plain_env(monkeypatch, pow2):
    monkeypatch.setenv("LPA_LOCALITY", "0")      # the plain order: degree descending, id ascending
    if not pow2:
        monkeypatch.setenv("LPA_POW2_SLICES", "0")


def _read_map(V, s, d, P, pow2, ranks):
    """The slot map read back after reset(), asserted equal to the restated one."""
    rm = X.restated_map(V, s, d, P, pow2)
    for g in ranks:
        g.reset()
    assert all(g.info()["slice"] == rm.slice for g in ranks)
    smap = X.map_from_l0(V, P, np.stack([g.exchange_get() for g in ranks]), rm.slot_of[0])
    assert np.array_equal(smap.slot_of, rm.slot_of), "the library's order is not the restated plain order"
    return smap


@pytest.mark.parametrize("name", list(X.CASES))
def test_exchange_case(gfa, oracle, monkeypatch, name):
    _, P, pow2, req = X.CASES[name]
    _plain_env(monkeypatch, pow2)
    V, s, d, _, hist = X.case_history(name)
    lb = gfa.Loopback(P)
    ranks = [gfa.Graph(s, d, V, rank=r, loopback=lb) for r in range(P)]
    try:
        if req is not None:
            for g, q in zip(ranks, req):
                g.set_posted(q)
        smap = _read_map(V, s, d, P, pow2, ranks)
        steps = X.restate(V, s, d, hist, smap, req)
        X.check_precondition(name, steps, smap)

        def work(r, g):
            out, last = [], g.info()
            for _ in range(X.N_STEPS):
                g.step(1)
                now = g.info()
                out.append((g.labels(), tuple(now[c] - last[c] for c in COUNTERS)))
                last = now
            return out

        got = gfa.run_ranks(ranks, work)
        for t, st in enumerate(steps):
            for r in range(P):
                lab, cnt = got[r][t]
                bad = int((lab != hist[t]).sum())
                assert bad == 0, f"{name} rank {r} superstep {t + 1} ({st.form}): {bad} labels differ"
                assert cnt == st.counters, (f"{name} rank {r} superstep {t + 1}: counters {dict(zip(X.FORMS, cnt))}, "
                                            f"restated {st.form} {dict(zip(X.FORMS, st.counters))} "
                                            f"(capd {st.capd}, capg {st.capg}, posted {st.post})")

        def rerun(r, g):
            g.reset()
            return g.run(X.N_STEPS)

        for r, lab in enumerate(gfa.run_ranks(ranks, rerun)):
            assert np.array_equal(lab, hist[-1]), f"{name} rank {r}: reset() + run({X.N_STEPS})"
    finally:
        for g in ranks:
            g.close()
        lb.close()


@pytest.mark.parametrize("name", list(X.COMPACT))
def test_delta_compact_entries(gfa, oracle, monkeypatch, name):
    """k_delta_compact against a reference of its own output: on caller-driven ranks,
    exchange_get_delta() as a set equals the restated (slot << 32 | label) set in every
    superstep; the exchange then goes by exchange_put_delta / exchange_put as the restated
    rule says (superstep 1 full, then a delta while the largest count fits dcap), bit-exact for 8 supersteps."""
    build, P, pow2, counts = X.COMPACT[name]
    _plain_env(monkeypatch, pow2)
    V, s, d, _ = build()
    n = 8
    _, hist, _ = oracle.lpa(V, s, d, n, per_iter=True)
    ranks = [gfa.Graph(s, d, V, rank=r, nranks=P) for r in range(P)]
    try:
        smap = _read_map(V, s, d, P, pow2, ranks)
        steps = X.restate(V, s, d, hist, smap)
        dcap = max(1, smap.slice // 4)
        assert all(sorted(st.nd) == sorted(counts) for st in steps[2:]), [st.nd for st in steps]
        if name == "second_trip":
            assert smap.slice == (1 << 20) + 64
            assert all(st.changed[r][0].max() == smap.slice - 1 for st in steps[2:] for r in range(P))
        forms = []
        for t, st in enumerate(steps):
            for g in ranks:
                g.step(1)
            deltas = [g.exchange_get_delta() for g in ranks]
            for r, e in enumerate(deltas):
                assert e.size == st.nd[r], f"{name} rank {r} superstep {t + 1}: {e.size} entries, restated {st.nd[r]}"
                assert np.array_equal(np.sort(e), st.entries(r)), f"{name} rank {r} superstep {t + 1}: entry set"
            if t > 0 and st.capd <= dcap:       # superstep 1 is full, as in the library
                for g in ranks:
                    g.exchange_put_delta(deltas)
                forms.append("delta")
            else:
                full = np.concatenate([g.exchange_get() for g in ranks])
                for g in ranks:
                    g.exchange_put(full)
                forms.append("full")
            for r, g in enumerate(ranks):
                assert np.array_equal(g.labels(), hist[t]), f"{name} rank {r} superstep {t + 1} ({forms[-1]})"
        assert forms[0] == "full" and forms[-2:] == ["delta", "delta"], forms
    finally:
        for g in ranks:
            g.close()
