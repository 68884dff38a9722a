"""CPU references for Pregel (the columns lpa_pregel returns).

Both walk the expression TREES (graphframes_amd.MessageExpr), never the compiled programs:

run()       numpy, vectorised over edges and vertices, a null mask beside every value; messages
            through am_ref.evaluate
run_loop()  a literal Python loop over iterations, vertices and edges with None for null, for
            the small cases

Semantics restated (graphframes.lib.Pregel.run of GraphFrames 0.8): Pregel column j starts as its
initial expression over the static columns.  One iteration, max_iter times, every read of the
state before it: every edge row with both ends in [0, V) evaluates each to_dst expression for its
dst and each to_src expression for its src, over the columns (static or Pregel) of its ends and
its edge columns; a null message is not delivered; a vertex aggregates what it received with sum,
min (-0.0 below +0.0), max, avg (sum / count) or count into msg, which is null where nothing
arrived, for count too; every Pregel column becomes its update expression over the vertex's own
old columns and msg, all columns at once.  A null initial or updated value is an error
(NullUpdate).  Null rules as in am_ref, plus coalesce(a, b) = a where a is not null, else b, and
isnull(a) = 1.0 / 0.0, never null.  The sums here are math.fsum: the exact sum rounded once.
"""
import math

import numpy as np

import am_ref


class NullUpdate(ValueError):
    def __init__(self, iteration, column, vertex):
        super().__init__(f"null value of column {column!r} in iteration {iteration} at vertex {vertex}")
        self.iteration, self.column, self.vertex = iteration, column, vertex


_ARITH = {"add": np.add, "sub": np.subtract, "mul": np.multiply}
_CMP = {"eq": np.equal, "ne": np.not_equal, "lt": np.less, "le": np.less_equal, "gt": np.greater,
        "ge": np.greater_equal}


def evaluate_vertex(expr, cols, msg, msg_ok):
    """(values float64[V], valid bool[V]) of a vertex expression; cols: name -> [V]."""
    V = msg.size
    op = expr.op
    if op == "const":
        return np.full(V, expr.value, np.float64), np.ones(V, bool)
    if op == "col":
        return cols[expr.value].astype(np.float64), np.ones(V, bool)
    if op == "msg":
        return msg.copy(), msg_ok.copy()
    args = [evaluate_vertex(a, cols, msg, msg_ok) for a in expr.args]
    with np.errstate(all="ignore"):
        if op == "neg":
            return -args[0][0], args[0][1]
        if op == "abs":
            return np.abs(args[0][0]), args[0][1]
        if op == "not":
            return (args[0][0] == 0.0).astype(np.float64), args[0][1]
        if op == "isnull":
            return (~args[0][1]).astype(np.float64), np.ones(V, bool)
        if op == "coalesce":
            (a, av), (b, bv) = args
            return np.where(av, a, b), av | bv
        if op == "when":
            c, cv = args[0]
            take = cv & (c != 0.0)
            x, xv = args[1]
            if len(args) == 3:
                o, ov = args[2]
                return np.where(take, x, o), np.where(take, xv, ov)
            return x, take & xv
        (a, av), (b, bv) = args
        ok = av & bv
        if op in _ARITH:
            return _ARITH[op](a, b), ok
        if op == "div":
            ok = ok & (b != 0.0)
            return np.divide(a, np.where(b != 0.0, b, 1.0)), ok
        if op in _CMP:
            return _CMP[op](a, b).astype(np.float64), ok
        if op == "and":
            return ((a != 0.0) & (b != 0.0)).astype(np.float64), ok
        if op == "or":
            return ((a != 0.0) | (b != 0.0)).astype(np.float64), ok
    raise AssertionError(op)


def _reduce(V, recv, val):
    """count, min, max, fsum, abs_sum per receiving vertex of the delivered messages."""
    count = np.bincount(recv, minlength=V).astype(np.int64)
    mn, mx = np.full(V, np.inf), np.full(V, -np.inf)
    np.minimum.at(mn, recv, val)
    np.maximum.at(mx, recv, val)
    zero = val == 0.0
    neg0 = np.bincount(recv[zero & np.signbit(val)], minlength=V) > 0
    pos0 = np.bincount(recv[zero & ~np.signbit(val)], minlength=V) > 0
    mn = np.where(mn == 0.0, np.where(neg0, -0.0, 0.0), mn)
    mx = np.where(mx == 0.0, np.where(pos0, 0.0, -0.0), mx)
    order = np.argsort(recv, kind="stable")
    cuts = np.concatenate([[0], np.cumsum(count)])
    sv = val[order]
    fs = np.array([math.fsum(sv[cuts[v]:cuts[v + 1]]) for v in range(V)], np.float64).reshape(V)
    abs_sum = np.bincount(recv, weights=np.abs(val), minlength=V)
    return count, mn, mx, fs, abs_sum


def _multiple(x, q):
    with np.errstate(all="ignore"):
        r = np.asarray(x, np.float64) / q
    return bool(np.all(np.isfinite(r)) and np.all(r == np.rint(r)))


def run(V, src, dst, max_iter, agg, to_src, to_dst, columns, vcols=None, ecols=None, q=None, free=()):
    """columns: [(name, initial expression, update expression)]; to_src / to_dst: lists of message
    expressions; vcols: the static columns, name -> [V].  Returns one dict per iteration (index 0:
    the start) with cols (name -> [V], the Pregel columns after it) and, from iteration 1 on,
    count, fsum, abs_sum of the messages per vertex; and a dict of the counters: edges,
    messages_to_src, messages_to_dst, nulls (summed over the iterations), rows (the message-list
    length in rows), iterations.
    q: assert that every message and every state (but the columns named in free, which nothing
    reads) is an integer multiple of q and that every vertex's sum of magnitudes is below 2^53 q:
    every summation order then gives the same bits."""
    vcols, ecols = dict(vcols or {}), ecols or {}
    s, d, e = am_ref.kept(V, src, dst)
    none = np.zeros(V)
    state = {}
    for j, (name, init, _) in enumerate(columns):
        x, ok = evaluate_vertex(init, vcols, none, np.zeros(V, bool))
        if not ok.all():
            raise NullUpdate(0, name, int(np.flatnonzero(~ok)[0]))
        state[name] = x
    rows = np.zeros(V, np.int64)
    if to_dst:
        rows += np.bincount(d, minlength=V)
    if to_src:
        rows += np.bincount(s, minlength=V)
    trace = [dict(cols=dict(state))]
    tot = dict(edges=int(s.size), messages_to_src=0, messages_to_dst=0, nulls=0, rows=rows, iterations=max_iter)
    for it in range(1, max_iter + 1):
        allc = {**vcols, **state}
        if q is not None:
            assert all(_multiple(x, q) for n, x in state.items() if n not in free), (it, "state")
        recv, val = [], []
        for exprs, to, key in ((to_dst, d, "messages_to_dst"), (to_src, s, "messages_to_src")):
            for expr in exprs:
                x, ok = am_ref.evaluate(expr, s, d, e, allc, ecols)
                recv.append(to[ok]), val.append(x[ok])
                tot[key] += int(ok.sum())
                tot["nulls"] += int((~ok).sum())
        recv, val = np.concatenate(recv), np.concatenate(val)
        count, mn, mx, fs, abs_sum = _reduce(V, recv, val)
        if q is not None:
            assert _multiple(val, q) and (abs_sum < 2.0 ** 53 * q).all(), (it, "messages")
        with np.errstate(all="ignore"):
            msg = {"sum": fs, "min": mn, "max": mx, "avg": fs / np.maximum(count, 1),
                   "count": count.astype(np.float64)}[agg]
        msg_ok = count > 0
        new = {}
        for name, _, upd in columns:
            x, ok = evaluate_vertex(upd, allc, np.where(msg_ok, msg, 0.0), msg_ok)
            if not ok.all():
                raise NullUpdate(it, name, int(np.flatnonzero(~ok)[0]))
            new[name] = x
        state = new
        trace.append(dict(cols=dict(state), count=count, fsum=fs, abs_sum=abs_sum))
    if q is not None:
        assert all(_multiple(x, q) for n, x in state.items() if n not in free), "final state"
    return trace, tot


def eval_vertex_one(expr, cols, v, msg):
    """A vertex expression at one vertex: a Python float, or None for null."""
    op = expr.op
    if op == "const":
        return float(expr.value)
    if op == "col":
        return float(cols[expr.value][v])
    if op == "msg":
        return msg
    a = [eval_vertex_one(x, cols, v, msg) for x in expr.args]
    if op == "when":
        if a[0] is not None and a[0] != 0.0:
            return a[1]
        return a[2] if len(a) == 3 else None
    if op == "coalesce":
        return a[0] if a[0] is not None else a[1]
    if op == "isnull":
        return 1.0 if a[0] is None else 0.0
    if any(x is None for x in a):
        return None
    if op == "neg":
        return -a[0]
    if op == "abs":
        return abs(a[0])
    if op == "not":
        return 1.0 if a[0] == 0.0 else 0.0
    x, y = a
    if op == "add":
        return x + y
    if op == "sub":
        return x - y
    if op == "mul":
        return x * y
    if op == "div":
        return None if y == 0.0 else x / y
    if op == "and":
        return 1.0 if x != 0.0 and y != 0.0 else 0.0
    if op == "or":
        return 1.0 if x != 0.0 or y != 0.0 else 0.0
    return 1.0 if {"eq": x == y, "ne": x != y, "lt": x < y, "le": x <= y, "gt": x > y, "ge": x >= y}[op] else 0.0


def run_loop(V, src, dst, max_iter, agg, to_src, to_dst, columns, vcols=None, ecols=None):
    """The final columns (name -> [V]) by literal loops: for every iteration, for every vertex,
    for every edge, for every message expression."""
    vcols, ecols = dict(vcols or {}), ecols or {}
    key = lambda x: (x, 0 if math.copysign(1.0, x) < 0 else 1)   # -0.0 below +0.0
    state = {}
    for name, init, _ in columns:
        state[name] = np.zeros(V)
        for v in range(V):
            x = eval_vertex_one(init, vcols, v, None)
            if x is None:
                raise NullUpdate(0, name, v)
            state[name][v] = x
    for it in range(1, max_iter + 1):
        allc = {**vcols, **state}
        new = {name: np.zeros(V) for name, _, _ in columns}
        for v in range(V):
            got = []
            for i in range(len(src)):
                s, d = int(src[i]), int(dst[i])
                if not (0 <= s < V and 0 <= d < V):
                    continue
                if d == v:
                    got += [am_ref.eval_one(x, s, d, i, allc, ecols) for x in to_dst]
                if s == v:
                    got += [am_ref.eval_one(x, s, d, i, allc, ecols) for x in to_src]
            got = [x for x in got if x is not None]
            msg = None
            if got:
                msg = {"sum": lambda: math.fsum(got), "min": lambda: min(got, key=key),
                       "max": lambda: max(got, key=key), "avg": lambda: math.fsum(got) / len(got),
                       "count": lambda: float(len(got))}[agg]()
            for name, _, upd in columns:
                x = eval_vertex_one(upd, allc, v, msg)
                if x is None:
                    raise NullUpdate(it, name, v)
                new[name][v] = x
        state = new
    return state
