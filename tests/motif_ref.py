"""Two independent CPU references for motif finding (GraphFrame.find) over dense ids.

A pattern comes in as a *spec*: ``(n_vars, terms, columns)`` with ``terms`` the edge terms in
PATTERN order as ``(src_var, dst_var, negated)`` and ``columns`` the named elements in order of
first appearance as ``("v", var)`` or ``("e", term index)``; ``spec(parsed)`` makes one from what
``parse_motif`` returns.  Both references return the sorted list of row tuples over ``columns``
(dense vertex ids and input edge rows).  Edges with an end outside [0, V) are no edges.

``literal``      brute force: every assignment of edge rows to the positive terms
                 (``itertools.product``), kept when the vertex variables are consistent and no
                 negated term has an edge.  For m <= 40 with <= 3 positive terms, m <= 24 with 4.
``merge_chain``  successive ``pandas.merge`` calls on the edge table in pattern order (a cross
                 join where a term shares nothing with the ones before it), the anti-joins last.
"""
import itertools

import numpy as np
import pandas as pd

TOOL_PATTERNS = [
    "(a)-[e]->(b)",
    "(a)-[e]->(b); (b)-[e2]->(a)",
    "(a)-[]->(b); (a)-[]->(c)",
    "(a)-[]->(b); (b)-[]->(c); (c)-[]->(a)",
    "(a)-[]->(b); !(b)-[]->(a)",
]
EXTRA_PATTERNS = [
    "(a)-[e]->(a)",
    "(a)-[]->()",
    "(a)-[e1]->(b); (a)-[e2]->(b)",
]
PATTERNS = TOOL_PATTERNS + EXTRA_PATTERNS


def spec(parsed):
    """The references' view of a ParsedMotif."""
    terms = [(t.src_var, t.dst_var, bool(t.negated)) for t in parsed.terms]
    var_of = {nm: i for i, nm in enumerate(parsed.var_names) if nm is not None}
    term_of = {t.edge: i for i, t in enumerate(parsed.terms) if t.edge is not None}
    columns = [("v", var_of[nm]) if k == "v" else ("e", term_of[nm]) for nm, k in parsed.names]
    return parsed.n_vars, terms, columns


def _valid(V, s, d):
    s = np.asarray(s, dtype=np.int64)
    d = np.asarray(d, dtype=np.int64)
    ok = (s >= 0) & (s < V) & (d >= 0) & (d < V)
    return s, d, np.flatnonzero(ok)


def literal(V, s, d, n_vars, terms, columns):
    s, d, rows = _valid(V, s, d)
    pos = [i for i, t in enumerate(terms) if not t[2]]
    neg = [i for i, t in enumerate(terms) if t[2]]
    assert (len(pos) <= 3 and rows.size <= 40) or (len(pos) <= 4 and rows.size <= 24), "too large for the brute force"
    pairs = {(int(s[e]), int(d[e])) for e in rows}
    out = []
    for pick in itertools.product([int(e) for e in rows], repeat=len(pos)):
        val = [None] * n_vars
        ok = True
        for i, e in zip(pos, pick):
            for var, x in ((terms[i][0], int(s[e])), (terms[i][1], int(d[e]))):
                if val[var] is None:
                    val[var] = x
                elif val[var] != x:
                    ok = False
            if not ok:
                break
        if not ok or any((val[terms[i][0]], val[terms[i][1]]) in pairs for i in neg):
            continue
        edge = dict(zip(pos, pick))
        out.append(tuple(val[c] if k == "v" else edge[c] for k, c in columns))
    return sorted(out)


def merge_chain(V, s, d, n_vars, terms, columns):
    s, d, rows = _valid(V, s, d)
    E = pd.DataFrame({"s": s[rows], "d": d[rows], "e": rows})
    tab = None
    for i, (a, b, negated) in enumerate(terms):
        if negated:
            continue
        if a == b:
            part = E[E["s"] == E["d"]].rename(columns={"s": f"v{a}", "e": f"e{i}"}).drop(columns="d")
        else:
            part = E.rename(columns={"s": f"v{a}", "d": f"v{b}", "e": f"e{i}"})
        if tab is None:
            tab = part
            continue
        on = [c for c in part.columns if c.startswith("v") and c in tab.columns]
        tab = tab.merge(part, on=on, how="inner") if on else tab.merge(part, how="cross")
    arcs = E[["s", "d"]].drop_duplicates()
    for a, b, negated in terms:
        if not negated:
            continue
        if a == b:
            hit = arcs[arcs["s"] == arcs["d"]].rename(columns={"s": f"v{a}"}).drop(columns="d")
        else:
            hit = arcs.rename(columns={"s": f"v{a}", "d": f"v{b}"})
        tab = tab.merge(hit, on=list(hit.columns), how="left", indicator=True)
        tab = tab[tab["_merge"] == "left_only"].drop(columns="_merge")
    cols = [f"{k}{c}" for k, c in columns]
    return sorted(map(tuple, tab[cols].to_numpy(dtype=np.int64).tolist()))


def rows_of(vcols, ecols, columns, term_at=None):
    """The sorted row tuples of a Graph.motif result over ``columns``; ``term_at[i]`` is the
    position at which pattern term i ran (the key of its edge column)."""
    arrs = [vcols[c] if k == "v" else ecols[c if term_at is None else term_at[c]] for k, c in columns]
    return sorted(zip(*(a.tolist() for a in arrs)))
