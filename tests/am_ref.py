"""CPU references for message aggregation (the values lpa_aggregate_messages returns).

Both walk the expression TREE (graphframes_amd.MessageExpr), never the compiled program:

aggregate()       numpy, vectorised over the edges, a null mask beside every value
aggregate_loop()  a literal Python double loop over vertices and edges with None for null, for
                  the small cases

Semantics restated: every edge row with both ends in [0, V) sends to_dst's value to its dst and
to_src's to its src; IEEE binary64; a comparison is 1.0 or 0.0; an operator with a null operand
gives null (& and | too); x / 0 is null; when(c, x) is x where c is true, else (c false or null)
the otherwise value, or null without one; a null message is not delivered.  Per receiving vertex:
count, min (-0.0 below +0.0), max (+0.0 above -0.0), math.fsum of the messages, and the sum of
their magnitudes; NaN for min / max and 0.0 for the sums where nothing arrived.
"""
import math

import numpy as np

U = 2.0 ** -53


def gamma(n):
    """gamma(n) = n u / (1 - n u).  A sum of n terms in ANY order has |computed - exact| <=
    gamma(n - 1) * sum |x_i| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2);
    fsum is the exact sum rounded once, within u * sum |x_i| of it; gamma(n - 1) + u <= gamma(n).
    So |computed - fsum| <= gamma(L) * sum |x_i| for a list of L >= n entries."""
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


_ARITH = {"add": np.add, "sub": np.subtract, "mul": np.multiply}
_CMP = {"eq": np.equal, "ne": np.not_equal, "lt": np.less, "le": np.less_equal, "gt": np.greater,
        "ge": np.greater_equal}


def evaluate(expr, s, d, e, vcols, ecols):
    """(values float64[n], valid bool[n]) of the expression over the edge rows e from s to d."""
    n = s.size
    op = expr.op
    if op == "const":
        return np.full(n, expr.value, np.float64), np.ones(n, bool)
    if op == "src":
        return vcols[expr.value][s].astype(np.float64), np.ones(n, bool)
    if op == "dst":
        return vcols[expr.value][d].astype(np.float64), np.ones(n, bool)
    if op == "edge":
        return ecols[expr.value][e].astype(np.float64), np.ones(n, bool)
    args = [evaluate(a, s, d, e, vcols, ecols) for a in expr.args]
    with np.errstate(all="ignore"):
        if op == "neg":
            return -args[0][0], args[0][1]
        if op == "abs":
            return np.abs(args[0][0]), args[0][1]
        if op == "not":
            return (args[0][0] == 0.0).astype(np.float64), args[0][1]
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


def kept(V, src, dst):
    """(s, d, edge row) of the rows with both ends in [0, V), int64, in input order."""
    s = np.asarray(src).astype(np.int64)
    d = np.asarray(dst).astype(np.int64)
    ok = (s >= 0) & (s < V) & (d >= 0) & (d < V)
    return s[ok], d[ok], np.flatnonzero(ok)


def aggregate(V, src, dst, to_src, to_dst, vcols=None, ecols=None):
    """dict of [V] arrays: count, min, max, fsum, abs_sum, rows (the message-list length), and the
    scalars messages_to_src, messages_to_dst, nulls."""
    vcols, ecols = vcols or {}, ecols or {}
    s, d, e = kept(V, src, dst)
    recv, val, ok = [], [], []
    rows = np.zeros(V, np.int64)
    n_msg = {}
    for expr, to in ((to_dst, d), (to_src, s)):
        n_msg[id(to)] = 0
        if expr is None:
            continue
        x, v = evaluate(expr, s, d, e, vcols, ecols)
        recv.append(to), val.append(x), ok.append(v)
        rows += np.bincount(to, minlength=V)
        n_msg[id(to)] = int(v.sum())
    recv, val, ok = np.concatenate(recv), np.concatenate(val), np.concatenate(ok)
    nulls = int((~ok).sum())
    recv, val = recv[ok], val[ok]
    count = np.bincount(recv, minlength=V).astype(np.int64)
    mn, mx = np.full(V, np.inf), np.full(V, -np.inf)
    np.minimum.at(mn, recv, val)
    np.maximum.at(mx, recv, val)
    # the zero's sign: min is -0.0 if any -0.0 arrived, max +0.0 if any +0.0 did
    zero = val == 0.0
    neg0 = np.bincount(recv[zero & np.signbit(val)], minlength=V) > 0
    pos0 = np.bincount(recv[zero & ~np.signbit(val)], minlength=V) > 0
    mn = np.where(mn == 0.0, np.where(neg0, -0.0, 0.0), mn)
    mx = np.where(mx == 0.0, np.where(pos0, 0.0, -0.0), mx)
    mn[count == 0] = np.nan
    mx[count == 0] = np.nan
    order = np.argsort(recv, kind="stable")
    cuts = np.concatenate([[0], np.cumsum(count)])
    sv = val[order]
    fs = np.array([math.fsum(sv[cuts[v]:cuts[v + 1]]) for v in range(V)], np.float64).reshape(V)
    with np.errstate(all="ignore"):
        abs_sum = np.bincount(recv, weights=np.abs(val), minlength=V)
    return dict(count=count, min=mn, max=mx, fsum=fs, abs_sum=abs_sum, rows=rows, messages_to_src=n_msg[id(s)],
                messages_to_dst=n_msg[id(d)], nulls=nulls, edges=int(s.size))


def eval_one(expr, s, d, e, vcols, ecols):
    """The expression over one edge row: a Python float, or None for null."""
    op = expr.op
    if op == "const":
        return float(expr.value)
    if op == "src":
        return float(vcols[expr.value][s])
    if op == "dst":
        return float(vcols[expr.value][d])
    if op == "edge":
        return float(ecols[expr.value][e])
    a = [eval_one(x, s, d, e, vcols, ecols) for x in expr.args]
    if op == "when":
        if a[0] is not None and a[0] != 0.0:
            return a[1]
        return a[2] if len(a) == 3 else None
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


def aggregate_loop(V, src, dst, to_src, to_dst, vcols=None, ecols=None):
    """count, min, max, fsum per vertex by a double loop: for every vertex, for every edge."""
    vcols, ecols = vcols or {}, ecols or {}
    count = np.zeros(V, np.int64)
    mn, mx, fs = np.full(V, np.nan), np.full(V, np.nan), np.zeros(V)
    for v in range(V):
        got = []
        for i in range(len(src)):
            s, d = int(src[i]), int(dst[i])
            if not (0 <= s < V and 0 <= d < V):
                continue
            if to_dst is not None and d == v:
                got.append(eval_one(to_dst, s, d, i, vcols, ecols))
            if to_src is not None and s == v:
                got.append(eval_one(to_src, s, d, i, vcols, ecols))
        got = [x for x in got if x is not None]
        count[v] = len(got)
        if got:
            # the key orders -0.0 below +0.0
            mn[v] = min(got, key=lambda x: (x, 0 if math.copysign(1.0, x) < 0 else 1))
            mx[v] = max(got, key=lambda x: (x, 0 if math.copysign(1.0, x) < 0 else 1))
            fs[v] = math.fsum(got)
    return dict(count=count, min=mn, max=mx, fsum=fs)


def same_bits(a, b):
    """Two float64 arrays are bit-equal, every NaN counted as one value."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))
