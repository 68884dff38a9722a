"""Drop-in for the reference's community-detection call surface.

The reference drives GraphFrames 0.6.0 from PySpark:

    Graphs = GraphFrame(Graph_Vertices, Graph_Edges)          # Graphframes.py:78
    Community_Graphs = Graphs.labelPropagation(maxIter=5)     # Graphframes.py:81

and then runs the outlier stage of Graphframes.py:92-137 over the result.
Here the same calls take pandas DataFrames (pyspark is not part of this
stack) and return a pandas DataFrame with every vertex column plus
``label`` (int64), computed by liblpa_hip.so on the GPU.

Id handling follows GraphFrames' ``indexedVertices`` / ``indexedEdges``
(SURVEY.md §8(a) a2, §8(b)):

* edges whose ``src`` or ``dst`` is not a vertex id are dropped (inner join);
* integral ids: ``label`` is the original id of the label vertex, so results are
  bit-comparable with GraphFrames on tie-free graphs;
* other ids (the reference's 8-hex-char SHA-1 strings): ``label`` is the dense
  index of the label vertex in ascending unique-id order (GraphFrames' own
  value, ``monotonically_increasing_id``, is partition-dependent and not
  reproducible; compare partitions, not values).

Ties are broken by the smallest label.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field

import numpy as np
import pandas as pd

from . import _lib
from .graph import SCAN_ROLES, Graph, PregelNullError, _check_scan

ID, SRC, DST, LABEL = "id", "src", "dst", "label"
COMPONENT = "component"
COUNT = "count"
CORE = "core"
ROLE, COMMON, SIMILARITY = "role", "common", "similarity"
BETWEENNESS = "betweenness"
PAGERANK = "pagerank"
PAGERANKS = "pageranks"
WEIGHT = "weight"
DISTANCES = "distances"
CC_ALGORITHMS = ("graphframes", "graphx")


def _check_max_iter(maxIter):
    if not isinstance(maxIter, (int, np.integer)) or isinstance(maxIter, bool):
        raise TypeError(f"maxIter must be an int, got {type(maxIter).__name__}")
    if maxIter <= 0:
        # GraphX LabelPropagation.run: require(maxSteps > 0, ...)
        raise ValueError(f"requirement failed: Maximum of steps must be greater than 0, but got {maxIter}")


def _check_page_rank(resetProbability, maxIter, tol):
    """The argument checks of GraphFrame.pageRank, before any device work."""
    if (maxIter is None) == (tol is None):
        # graphframes.GraphFrame.pageRank (0.6.0)
        raise ValueError("Exactly one of maxIter or tol should be set.")
    if tol is not None:
        raise NotImplementedError(
            "pageRank(tol=...) (GraphX runUntilConvergence) is not implemented; use maxIter for the static form")
    if not isinstance(maxIter, (int, np.integer)) or isinstance(maxIter, bool):
        raise TypeError(f"maxIter must be an int, got {type(maxIter).__name__}")
    if maxIter <= 0:
        # GraphX PageRank.runWithOptions: require(numIter > 0, ...)
        raise ValueError(f"requirement failed: Number of iterations must be greater than 0, but got {maxIter}")
    if not 0 <= resetProbability <= 1:   # NaN fails both
        raise ValueError(
            f"requirement failed: Random reset probability must belong to [0, 1], but got {resetProbability}")


def _check_parallel_page_rank(resetProbability, sourceIds, maxIter):
    """The argument checks of GraphFrame.parallelPersonalizedPageRank that need no vertex
    table, before any device work."""
    if sourceIds is None or (isinstance(sourceIds, (list, tuple, np.ndarray)) and len(sourceIds) == 0):
        # graphframes.GraphFrame.parallelPersonalizedPageRank (0.6.0)
        raise ValueError("Source vertices Ids sourceIds must be provided")
    if maxIter is None:
        raise ValueError("Max number of iterations maxIter must be provided")
    if isinstance(sourceIds, (str, bytes)) or not isinstance(sourceIds, (list, tuple, np.ndarray)):
        raise TypeError(f"sourceIds must be a list, tuple or array of vertex ids, got {type(sourceIds).__name__}")
    if isinstance(sourceIds, np.ndarray) and sourceIds.ndim != 1:
        raise TypeError(f"sourceIds must be one-dimensional, got {sourceIds.ndim} dimensions")
    _check_page_rank(resetProbability, maxIter, None)


def _check_scc_max_iter(maxIter):
    """The argument check of GraphFrame.stronglyConnectedComponents, before any device work."""
    if not isinstance(maxIter, (int, np.integer)) or isinstance(maxIter, (bool, np.bool_)):
        raise TypeError(f"maxIter must be an int, got {type(maxIter).__name__}")
    if maxIter <= 0:
        # GraphX StronglyConnectedComponents.run: require(numIter > 0, ...)
        raise ValueError(f"requirement failed: Number of iterations must be greater than 0, but got {maxIter}")


def _check_louvain(maxLevels, maxRounds):
    """The argument checks of GraphFrame.louvain, before any device work."""
    for name, x in (("maxLevels", maxLevels), ("maxRounds", maxRounds)):
        if not isinstance(x, (int, np.integer)) or isinstance(x, (bool, np.bool_)):
            raise TypeError(f"{name} must be an int, got {type(x).__name__}")
        if x <= 0:
            raise ValueError(f"{name} must be greater than 0, but got {x}")


def _check_core_k(k, name="k"):
    """The argument check of GraphFrame.kCore (and of a core-number cap), before any device work."""
    if not isinstance(k, (int, np.integer)) or isinstance(k, (bool, np.bool_)):
        raise TypeError(f"{name} must be an int, got {type(k).__name__}")
    if k < 0:
        raise ValueError(f"{name} must not be negative, but got {k}")


def _check_bfs(maxPathLength, maxPaths):
    """The argument checks of GraphFrame.bfs that need no table, before any device work."""
    if not isinstance(maxPathLength, (int, np.integer)) or isinstance(maxPathLength, (bool, np.bool_)):
        raise TypeError(f"maxPathLength must be an int, got {type(maxPathLength).__name__}")
    if maxPathLength < 0:
        # graphframes.lib.BFS.run: require(maxPathLength >= 0, ...)
        raise ValueError(f"requirement failed: BFS maxPathLength must be >= 0, but was set to {maxPathLength}")
    if maxPaths is not None:
        if not isinstance(maxPaths, (int, np.integer)) or isinstance(maxPaths, (bool, np.bool_)):
            raise TypeError(f"maxPaths must be an int or None, got {type(maxPaths).__name__}")
        if maxPaths < 0:
            raise ValueError(f"maxPaths must not be negative, got {maxPaths}")


def _bfs_mask(frame: pd.DataFrame, expr, name: str) -> np.ndarray:
    """``expr`` over ``frame`` as a boolean array of its length: a str goes through
    ``DataFrame.eval``, a callable is called with the frame, a boolean Series or array is taken
    positionally."""
    if isinstance(expr, str):
        try:
            val = frame.eval(expr)
        except Exception as e:  # noqa: BLE001 -- pandas raises many types for a bad expression
            raise ValueError(f"{name}: cannot evaluate {expr!r}: {e}") from e
    elif callable(expr):
        val = expr(frame)
    elif isinstance(expr, (pd.Series, np.ndarray)):
        val = expr
    else:
        raise TypeError(f"{name} must be a str, a callable or a boolean Series or array, got {type(expr).__name__}")
    if not isinstance(val, (pd.Series, np.ndarray)):
        raise TypeError(f"{name} must yield a boolean column, got {type(val).__name__}")
    a = np.asarray(val)
    if a.dtype != np.bool_:
        raise TypeError(f"{name} must yield a boolean column, got dtype {a.dtype}")
    if a.ndim != 1:
        raise TypeError(f"{name} must yield one column, got {a.ndim} dimensions")
    if a.size != len(frame):
        raise ValueError(f"{name} must yield {len(frame)} entries, got {a.size}")
    return a


def _path_dag(level, src, dst, edge_index):
    """The marked edges grouped by source, ascending edge index inside a group: (sorted edge
    indices, their targets, start of each vertex's group [V + 1])."""
    level = np.asarray(level)
    eidx = np.asarray(edge_index, dtype=np.int64)
    es = np.asarray(src)[eidx].astype(np.int64)
    order = np.lexsort((eidx, es))
    off = np.zeros(level.size + 1, dtype=np.int64)
    np.cumsum(np.bincount(es, minlength=level.size), out=off[1:])
    return eidx[order], np.asarray(dst)[eidx[order]].astype(np.int64), off


def count_paths(level, src, dst, edge_index, length) -> int:
    """The number of rows ``enumerate_paths`` would return, counted over the DAG level by level
    (exact below 2^53, float64 above)."""
    if length <= 0:
        return 0
    level = np.asarray(level)
    eidx = np.asarray(edge_index, dtype=np.int64)
    es, ed = np.asarray(src)[eidx].astype(np.int64), np.asarray(dst)[eidx].astype(np.int64)
    n = (level == length).astype(np.float64)      # paths from the vertex to a target
    le = level[es]
    for l in range(int(length) - 1, -1, -1):
        at = le == l
        np.add.at(n, es[at], n[ed[at]])
    return int(n[level == 0].sum())


def enumerate_paths(level, src, dst, edge_index, length):
    """Every path of ``length`` edges of a ``Graph.bfs`` result: ``level`` [V], the edge list
    ``src`` / ``dst`` it was built on, the marked ``edge_index``.  Returns ``(verts [n, L + 1]
    int32, edges [n, L] int64)``: row i is one path, its vertices (dense ids) and the indices of
    its edges; the rows are sorted by the tuple of edge indices.  One level is one join: every
    path is repeated by the out-count of its last vertex (``np.repeat``).  A pure host
    function."""
    L = int(length)
    if L <= 0:
        return np.empty((0, max(L, 0) + 1), np.int32), np.empty((0, 0), np.int64)
    level = np.asarray(level)
    se, sd, off = _path_dag(level, src, dst, edge_index)
    eidx = np.asarray(edge_index, dtype=np.int64)
    es = np.asarray(src)[eidx].astype(np.int64)
    first = np.sort(eidx[level[es] == 0])
    verts = [np.asarray(src)[first].astype(np.int64), np.asarray(dst)[first].astype(np.int64)]
    edges = [first]
    for _ in range(1, L):
        end = verts[-1]
        cnt = off[end + 1] - off[end]
        rep = np.repeat(np.arange(end.size), cnt)
        start = np.cumsum(cnt) - cnt
        pos = off[end][rep] + (np.arange(rep.size) - start[rep])
        verts = [c[rep] for c in verts] + [sd[pos]]
        edges = [c[rep] for c in edges] + [se[pos]]
    return np.stack(verts, axis=1).astype(np.int32), np.stack(edges, axis=1)


MOTIF_MAX_TERMS = 8   # positive terms, and negated terms, of one pattern

_MOTIF_EDGE = re.compile(r"^(!?)\(([A-Za-z0-9_]*)\)-\[([A-Za-z0-9_]*)\]->\(([A-Za-z0-9_]*)\)$")
_MOTIF_VERTEX = re.compile(r"^\(([A-Za-z0-9_]+)\)$")


@dataclass(frozen=True)
class MotifTerm:
    """One edge term of a motif: ``src`` / ``dst`` / ``edge`` are the names (``None``:
    anonymous), ``src_var`` / ``dst_var`` the vertex variables (an anonymous vertex is a fresh
    one).  ``str(term)`` is the term as GraphFrames writes it."""
    src: str | None
    dst: str | None
    edge: str | None
    negated: bool
    src_var: int
    dst_var: int

    def __str__(self):
        return "{}({})-[{}]->({})".format("!" if self.negated else "", self.src or "", self.edge or "",
                                          self.dst or "")


@dataclass(frozen=True)
class ParsedMotif:
    """A parsed pattern: its edge ``terms`` in pattern order, the ``lone`` vertex terms' names,
    ``names`` = the named elements as ``(name, "v" | "e")`` in order of first appearance,
    ``var_names[var]`` the name of a vertex variable (``None``: anonymous)."""
    terms: tuple
    lone: tuple
    names: tuple
    var_names: tuple

    @property
    def n_vars(self) -> int:
        return len(self.var_names)


def parse_motif(pattern) -> ParsedMotif:
    """Parse a GraphFrames motif: terms separated by ``;``, whitespace free; a term is
    ``(a)-[e]->(b)``, with ``!`` in front when negated, or a lone vertex ``(a)``; ``()`` and
    ``[]`` are anonymous.  Every named vertex is one variable wherever it appears, every ``()``
    a fresh one, every positive term has its own edge variable.  A pure host function: raises
    ``ValueError`` naming the offending term for every pattern this implementation refuses
    (see ``GraphFrame.find``)."""
    if not isinstance(pattern, str):
        raise TypeError(f"pattern must be a str, got {type(pattern).__name__}")
    text = "".join(pattern.split())
    if not text:
        raise ValueError("find: the pattern is empty")
    terms, lone, var_names = [], [], []
    kind, var_of, edge_term = {}, {}, {}

    def name_of(name, k, term):
        if kind.setdefault(name, k) != k:
            raise ValueError(f"find: term '{term}': the name '{name}' is used both for a vertex and for an edge")

    def vertex(name, term):
        if not name:
            var_names.append(None)
            return len(var_names) - 1
        name_of(name, "v", term)
        if name not in var_of:
            var_of[name] = len(var_names)
            var_names.append(name)
        return var_of[name]

    for raw in text.split(";"):
        mv = _MOTIF_VERTEX.match(raw)
        if mv:
            name_of(mv.group(1), "v", raw)
            lone.append(mv.group(1))
            continue
        me = _MOTIF_EDGE.match(raw)
        if not me:
            raise ValueError(f"find: the term '{raw}' does not parse; a term is (a)-[e]->(b), !(a)-[]->(b) or (a)")
        neg, a, e, b = me.group(1) == "!", me.group(2), me.group(3), me.group(4)
        if neg and e:
            raise ValueError(f"find: term '{raw}': a negated term cannot name its edge")
        if neg and (not a or not b):
            raise ValueError(f"find: term '{raw}': a negated term cannot have an anonymous vertex")
        if e:
            name_of(e, "e", raw)
            if e in edge_term:
                raise ValueError(f"find: term '{raw}': the edge name '{e}' is already used by '{edge_term[e]}'")
            edge_term[e] = raw
        if neg:   # a negated term binds nothing: its variables are looked up once every term is read
            terms.append((a, b, None, True, raw))
        else:
            terms.append(MotifTerm(a or None, b or None, e or None, False, vertex(a, raw), vertex(b, raw)))
    for i, t in enumerate(terms):
        if isinstance(t, tuple):
            a, b, _, _, raw = t
            for nm in (a, b):
                name_of(nm, "v", raw)
                if nm not in var_of:
                    raise ValueError(f"find: term '{raw}': no positive term binds the vertex '{nm}'")
            terms[i] = MotifTerm(a, b, None, True, var_of[a], var_of[b])
    # the named elements in order of first appearance in the pattern
    order = []
    for raw in text.split(";"):
        for nm in re.findall(r"[A-Za-z0-9_]+", raw):
            if (nm, kind[nm]) not in order:
                order.append((nm, kind[nm]))
    pos = [t for t in terms if not t.negated]
    n_neg = len(terms) - len(pos)
    if len(pos) > MOTIF_MAX_TERMS or n_neg > MOTIF_MAX_TERMS:
        raise ValueError(f"find: the pattern '{text}' has {len(pos)} positive and {n_neg} negated terms, "
                         f"more than {MOTIF_MAX_TERMS} of a kind")
    for nm in lone:
        if nm not in var_of and not (len(lone) == 1 and not terms):
            raise ValueError(f"find: the lone term '({nm})' occurs in no edge term; a cross-join is not supported")
    if not order:
        raise ValueError(f"find: the pattern '{text}' names nothing")
    # the positive terms form one connected pattern
    if pos:
        seen, todo = {pos[0].src_var, pos[0].dst_var}, list(pos[1:])
        while todo:
            nxt = [t for t in todo if t.src_var not in seen and t.dst_var not in seen]
            if len(nxt) == len(todo):
                raise ValueError(f"find: term '{todo[0]}' is not connected to '{pos[0]}'; "
                                 "a cross-join of disconnected patterns is not supported")
            for t in todo:
                if t not in nxt:
                    seen.update((t.src_var, t.dst_var))
            todo = nxt
    return ParsedMotif(tuple(terms), tuple(lone), tuple(order), tuple(var_names))


def plan_motif(parsed: ParsedMotif) -> list:
    """The execution order of a parsed pattern's edge terms, as indices into ``parsed.terms``.
    The first positive term is the one that binds the most named variables; then always a term
    with both ends bound (a close: it can only keep or drop rows per parallel edge, and never
    needs a new column) before an extend; ties go to pattern order.  A negated term runs right
    after the positive term that binds the last of its variables, so it prunes the table
    before the next extension multiplies it."""
    terms = parsed.terms
    pos = [i for i, t in enumerate(terms) if not t.negated]
    neg = [i for i, t in enumerate(terms) if t.negated]
    if not pos:
        return []

    def named(i):
        t = terms[i]
        return len({v for v in (t.src_var, t.dst_var) if parsed.var_names[v] is not None})

    first = max(pos, key=lambda i: (named(i), -i))
    plan, bound, left = [], set(), [i for i in pos if i != first]

    def run(i):
        plan.append(i)
        bound.update((terms[i].src_var, terms[i].dst_var))
        for j in list(neg):
            if terms[j].src_var in bound and terms[j].dst_var in bound:
                plan.append(j)
                neg.remove(j)

    run(first)
    while left:
        close = [i for i in left if terms[i].src_var in bound and terms[i].dst_var in bound]
        ext = [i for i in left if terms[i].src_var in bound or terms[i].dst_var in bound]
        nxt = (close or ext)[0]   # parse_motif has checked that the pattern is connected
        left.remove(nxt)
        run(nxt)
    return plan


def _check_max_rows(maxRows):
    if maxRows is None:
        return
    if not isinstance(maxRows, (int, np.integer)) or isinstance(maxRows, (bool, np.bool_)):
        raise TypeError(f"maxRows must be an int or None, got {type(maxRows).__name__}")
    if maxRows <= 0:
        raise ValueError(f"maxRows must be greater than 0, got {maxRows}")


# ---- message aggregation: the expression layer (pure host) ----
AM_MAX_OPS = _lib.LPA_AM_MAX_OPS                  # ops of one compiled message
AM_MAX_STACK = _lib.LPA_AM_MAX_STACK              # operand stack depth of its evaluation
AM_MAX_CONSTS = _lib.LPA_AM_MAX_CONSTS            # distinct constants of one message
AM_MAX_VERTEX_COLUMNS = _lib.LPA_AM_MAX_COLUMNS   # vertex columns of one call, both directions together
AM_MAX_EDGE_COLUMNS = _lib.LPA_AM_MAX_COLUMNS     # edge columns of one call, both directions together
AM_MSG_NAME = "MSG"
AM_EXACT_INT = 2 ** 53                            # integers up to this magnitude are exact in binary64
_AM_OPCODE = {name: i for i, name in enumerate(_lib.AM_OPCODES)}
_AM_BINARY = {"add": "+", "sub": "-", "mul": "*", "div": "/", "eq": "==", "ne": "!=", "lt": "<", "le": "<=",
              "gt": ">", "ge": ">=", "and": "&", "or": "|"}
_AM_UNARY = {"neg": "-", "not": "~"}
_AM_BOOL_OPS = ("eq", "ne", "lt", "le", "gt", "ge", "and", "or", "not")
_AM_COLUMN_KINDS = {"src": "vertex", "dst": "vertex", "edge": "edge"}
AM_AGGREGATES = ("sum", "min", "max", "avg", "count")
_VP_OPCODE = {name: i for i, name in enumerate(_lib.VP_OPCODES)}
_VP_ONLY_OPS = ("col", "coalesce", "isnull")      # nodes of a vertex expression that no message holds
PREGEL_MAX_COLUMNS = _lib.LPA_PG_MAX_COLUMNS      # Pregel columns of one run
PREGEL_MAX_MESSAGES = _lib.LPA_PG_MAX_MESSAGES    # sendMsgToSrc, and sendMsgToDst, of one run


class MessageExpr:
    """A node of a message expression: ``AM.src["x"] * 2 + AM.edge["w"]``.  Built by the
    operators and by ``AggregateMessages``; never evaluated on the host."""
    __slots__ = ("op", "args", "value", "is_bool")

    def __init__(self, op, args=(), value=None, is_bool=False):
        self.op, self.args, self.value, self.is_bool = op, tuple(args), value, bool(is_bool)

    @staticmethod
    def of(x):
        """An operand: an expression, or a plain Python / numpy number or bool as a constant."""
        if isinstance(x, MessageExpr):
            return x
        if isinstance(x, MessageAggregate):
            raise ValueError(f"{x} is an aggregate: it is aggCol, not an operand of an expression")
        if isinstance(x, (bool, np.bool_)):
            return MessageExpr("const", value=1.0 if x else 0.0, is_bool=True)
        if isinstance(x, (int, np.integer)):
            if abs(int(x)) > AM_EXACT_INT:
                raise ValueError(f"the constant {x} is beyond +-2^53 and not exact in binary64")
            return MessageExpr("const", value=float(int(x)))
        if isinstance(x, (float, np.floating)):
            if not np.isfinite(x):
                raise ValueError(f"the constant {x} is not finite")
            return MessageExpr("const", value=float(x))
        raise TypeError(f"a message operand is an expression or a number, got {type(x).__name__}")

    def _binary(self, op, other, swap=False):
        a, b = self, MessageExpr.of(other)
        if swap:
            a, b = b, a
        if op in ("and", "or"):
            for x in (a, b):
                x._need_bool(_AM_BINARY[op])
        return MessageExpr(op, (a, b), is_bool=op in _AM_BOOL_OPS)

    def _need_bool(self, what):
        if not self.is_bool:
            raise ValueError(f"{what} takes comparison results, got {self}; compare a column first, as in "
                             f"({self} != 0)")

    def __add__(self, o): return self._binary("add", o)
    def __radd__(self, o): return self._binary("add", o, True)
    def __sub__(self, o): return self._binary("sub", o)
    def __rsub__(self, o): return self._binary("sub", o, True)
    def __mul__(self, o): return self._binary("mul", o)
    def __rmul__(self, o): return self._binary("mul", o, True)
    def __truediv__(self, o): return self._binary("div", o)
    def __rtruediv__(self, o): return self._binary("div", o, True)
    def __eq__(self, o): return self._binary("eq", o)
    def __ne__(self, o): return self._binary("ne", o)
    def __lt__(self, o): return self._binary("lt", o)
    def __le__(self, o): return self._binary("le", o)
    def __gt__(self, o): return self._binary("gt", o)
    def __ge__(self, o): return self._binary("ge", o)
    def __and__(self, o): return self._binary("and", o)
    def __rand__(self, o): return self._binary("and", o, True)
    def __or__(self, o): return self._binary("or", o)
    def __ror__(self, o): return self._binary("or", o, True)
    def __neg__(self): return MessageExpr("neg", (self,))
    def __abs__(self): return MessageExpr("abs", (self,))

    def __invert__(self):
        self._need_bool("~")
        return MessageExpr("not", (self,), is_bool=True)

    __hash__ = None   # == builds an expression

    def __bool__(self):
        raise TypeError("a message expression has no truth value: combine conditions with & | ~, not and / or / not")

    def otherwise(self, value):
        """The value of a ``when`` whose condition is false or null."""
        if self.op != "when" or len(self.args) != 2:
            raise ValueError("otherwise() follows when(condition, value), once")
        v = MessageExpr.of(value)
        return MessageExpr("when", self.args + (v,), is_bool=self.is_bool and v.is_bool)

    def same(self, other) -> bool:
        """Structural equality (``==`` builds a comparison)."""
        return (isinstance(other, MessageExpr) and self.op == other.op and self.value == other.value
                and len(self.args) == len(other.args) and all(a.same(b) for a, b in zip(self.args, other.args)))

    def walk(self):
        """Every node, operands before their operator."""
        for a in self.args:
            yield from a.walk()
        yield self

    def __str__(self):
        if self.op == "const":
            return repr(self.value)
        if self.op in _AM_COLUMN_KINDS:
            return f"{self.op}[{self.value!r}]"
        if self.op == "msg":
            return AM_MSG_NAME
        if self.op in _AM_BINARY:
            return f"({self.args[0]} {_AM_BINARY[self.op]} {self.args[1]})"
        if self.op in _AM_UNARY:
            return f"({_AM_UNARY[self.op]}{self.args[0]})"
        if self.op == "abs":
            return f"abs({self.args[0]})"
        if self.op == "col":
            return f"col[{self.value!r}]"
        if self.op in ("coalesce", "isnull"):
            return f"{self.op}({', '.join(map(str, self.args))})"
        s = f"when({self.args[0]}, {self.args[1]})"
        return s + (f".otherwise({self.args[2]})" if len(self.args) == 3 else "")

    __repr__ = __str__


class MessageAggregate:
    """``AM.sum(AM.msg)`` and its kin: what ``aggCol`` is.  ``alias(name)`` names the column."""

    def __init__(self, kind, expr, name=None):
        self.kind, self.expr, self._name = kind, expr, name

    def alias(self, name):
        return MessageAggregate(self.kind, self.expr, str(name))

    @property
    def name(self) -> str:
        """The result column: the alias, or Spark's default ``sum(MSG)``."""
        return self._name if self._name is not None else f"{self.kind}({AM_MSG_NAME})"

    def __str__(self):
        return f"{self.kind}({self.expr})"

    __repr__ = __str__


class _MessageColumns:
    def __init__(self, kind):
        self._kind = kind

    def __getitem__(self, name):
        if not isinstance(name, str):
            raise TypeError(f"AM.{self._kind}[...] takes a column name, got {type(name).__name__}")
        return MessageExpr(self._kind, value=name)


class AggregateMessages:
    """The vocabulary of ``GraphFrame.aggregateMessages``, used as ``AM`` the way
    ``graphframes.lib.AggregateMessages`` is::

        from graphframes_amd import AggregateMessages as AM
        g.aggregateMessages(AM.sum(AM.msg).alias("crossing"),
                            sendToSrc=AM.when(AM.src["label"] != AM.dst["label"], 1.0),
                            sendToDst=AM.when(AM.src["label"] != AM.dst["label"], 1.0))

    ``AM.src["col"]`` / ``AM.dst["col"]`` read a vertex column of the edge's source /
    destination, ``AM.edge["col"]`` an edge column, ``AM.msg`` is the message (in ``aggCol``
    only), ``AM.lit(x)`` a constant; a plain Python number is accepted wherever an operand is.
    Operands combine with ``+ - * /``, unary ``-``, ``abs()``, the six comparisons, and
    ``& | ~`` on comparison results.  ``AM.when(cond, value)`` optionally takes
    ``.otherwise(value)``.  The aggregates are ``AM.sum``, ``AM.min``, ``AM.max``, ``AM.avg``
    (alias ``AM.mean``) and ``AM.count`` of ``AM.msg``, each with an optional ``.alias(name)``;
    the default names are Spark's, ``sum(MSG)`` and so on.

    These are this package's expressions over pandas frames, not Spark SQL columns: strings such
    as ``"src.x + 1"`` and functions of ``pyspark.sql.functions`` are not understood.  Everything
    is evaluated in IEEE binary64; a comparison is worth 1.0 or 0.0.  Null follows Spark where
    that is cheap to state: an operator with a null operand gives null; ``x / 0`` gives null, as
    Spark SQL does; a ``when`` without ``otherwise`` gives null where its condition is false; a
    null condition takes the ``otherwise`` branch, or gives null when there is none; a null
    message is not delivered.  One deviation: ``&`` and ``|`` with a null operand give null (Spark
    has three-valued logic: ``false & null`` is false there)."""
    src = _MessageColumns("src")
    dst = _MessageColumns("dst")
    edge = _MessageColumns("edge")
    msg = MessageExpr("msg")

    @staticmethod
    def lit(x):
        return MessageExpr.of(x)

    @staticmethod
    def when(condition, value):
        c = MessageExpr.of(condition)
        c._need_bool("when()'s condition")
        v = MessageExpr.of(value)
        return MessageExpr("when", (c, v), is_bool=v.is_bool)

    @staticmethod
    def sum(x): return MessageAggregate("sum", x)
    @staticmethod
    def min(x): return MessageAggregate("min", x)
    @staticmethod
    def max(x): return MessageAggregate("max", x)
    @staticmethod
    def avg(x): return MessageAggregate("avg", x)
    @staticmethod
    def count(x): return MessageAggregate("count", x)
    mean = avg


@dataclass(frozen=True)
class CompiledMessage:
    """A message expression as the postfix program the kernels interpret (include/lpa.h
    ``lpa_am_program``): ``ops`` are (opcode, 16-bit argument) pairs, the argument an index into
    ``consts``, ``vertex_columns`` or ``edge_columns`` for the opcodes that push."""
    ops: tuple
    consts: tuple
    vertex_columns: tuple
    edge_columns: tuple
    depth: int

    def decode(self) -> MessageExpr:
        """The expression back from the program."""
        st = []
        for code, arg in self.ops:
            op = _lib.AM_OPCODES[code]
            if op == "const":
                st.append(MessageExpr("const", value=self.consts[arg]))
            elif op in ("src", "dst"):
                st.append(MessageExpr(op, value=self.vertex_columns[arg]))
            elif op == "edge":
                st.append(MessageExpr(op, value=self.edge_columns[arg]))
            else:
                n = 1 if op in ("neg", "abs", "not") else 3 if op == "when_else" else 2
                args = st[len(st) - n:]
                del st[len(st) - n:]
                st.append(MessageExpr("when" if op == "when_else" else op, args))
        assert len(st) == 1
        return st[0]


def compile_message(expr, vertex_columns=(), edge_columns=()) -> CompiledMessage:
    """Compile a message expression to its postfix program: operands left to right, then their
    operator.  ``vertex_columns`` / ``edge_columns``: names that already hold the first column
    indices (the other direction's of the same call); the result's lists extend them.  Pure host
    code.  ``ValueError`` for ``AM.msg`` inside the message and for a limit exceeded: more than
    AM_MAX_OPS ops, a stack deeper than AM_MAX_STACK, more than AM_MAX_CONSTS constants, more
    than AM_MAX_VERTEX_COLUMNS or AM_MAX_EDGE_COLUMNS columns."""
    root = MessageExpr.of(expr)
    ops, consts = [], []
    names = {"vertex": list(vertex_columns), "edge": list(edge_columns)}
    caps = {"vertex": AM_MAX_VERTEX_COLUMNS, "edge": AM_MAX_EDGE_COLUMNS}
    depth = top = 0
    for node in root.walk():
        if node.op == "msg":
            raise ValueError(f"AM.msg appears inside the message {root}: it is what aggCol aggregates")
        if node.op in _VP_ONLY_OPS:
            raise ValueError(f"{node} appears inside the message {root}: Pregel.{node.op} belongs to a vertex "
                             "expression of Pregel.withVertexColumn")
        if node.op == "const":
            bits = np.float64(node.value).tobytes()   # 0.0 and -0.0 are two constants
            at = [np.float64(c).tobytes() for c in consts]
            if bits not in at:
                consts.append(node.value)
                at.append(bits)
            arg, pops = at.index(bits), 0
        elif node.op in _AM_COLUMN_KINDS:
            kind = _AM_COLUMN_KINDS[node.op]
            if node.value not in names[kind]:
                names[kind].append(node.value)
            arg, pops = names[kind].index(node.value), 0
        else:
            arg, pops = 0, len(node.args)
        code = "when_else" if node.op == "when" and pops == 3 else node.op
        ops.append((_AM_OPCODE[code], arg))
        depth += 1 - pops
        top = max(top, depth)
    if len(ops) > AM_MAX_OPS:
        raise ValueError(f"the message {root} compiles to {len(ops)} ops, more than AM_MAX_OPS = {AM_MAX_OPS}")
    if top > AM_MAX_STACK:
        raise ValueError(f"the message {root} needs a stack of {top} values, more than AM_MAX_STACK = {AM_MAX_STACK}")
    if len(consts) > AM_MAX_CONSTS:
        raise ValueError(f"the message {root} holds {len(consts)} constants, more than AM_MAX_CONSTS = "
                         f"{AM_MAX_CONSTS}")
    for kind in ("vertex", "edge"):
        if len(names[kind]) > caps[kind]:
            raise ValueError(f"the call reads {len(names[kind])} {kind} columns ({', '.join(names[kind])}), more "
                             f"than AM_MAX_{kind.upper()}_COLUMNS = {caps[kind]}")
    return CompiledMessage(tuple(ops), tuple(consts), tuple(names["vertex"]), tuple(names["edge"]), top)


def _check_agg_col(aggCol) -> MessageAggregate:
    if not isinstance(aggCol, MessageAggregate) or aggCol.kind not in AM_AGGREGATES:
        raise ValueError(f"aggCol must be AM.sum, AM.min, AM.max, AM.avg or AM.count of AM.msg, got {aggCol!r}")
    e = aggCol.expr
    if isinstance(e, MessageExpr) and e.op != "msg":
        for node in e.walk():
            if node.op in _AM_COLUMN_KINDS:
                raise ValueError(f"aggCol {aggCol} reads AM.{node.op}[{node.value!r}]: it aggregates AM.msg alone; "
                                 "columns belong in sendToSrc / sendToDst")
    if not isinstance(e, MessageExpr) or e.op != "msg":
        raise ValueError(f"aggCol must aggregate exactly AM.msg, got {aggCol}")
    return aggCol


def _am_column(frame: pd.DataFrame, name: str, kind: str) -> np.ndarray:
    """A column an expression reads, as float64; refused unless every value is exact and finite."""
    if name not in frame.columns:
        raise ValueError(f"the {kind} frame has no column {name!r}; it has: {','.join(map(str, frame.columns))}")
    col = frame[name]
    dt = col.dtype
    types = pd.api.types
    if not (types.is_bool_dtype(dt) or (types.is_numeric_dtype(dt) and not types.is_complex_dtype(dt))):
        raise ValueError(f"column {name!r} of the {kind} frame is not numeric or bool: dtype {dt}")
    bad = ValueError(f"column {name!r} of the {kind} frame holds NaN, None or an infinite value")
    if col.isna().any():
        raise bad
    if types.is_bool_dtype(dt):
        return col.to_numpy(dtype=bool).astype(np.float64)
    if types.is_integer_dtype(dt):
        a = col.to_numpy(dtype=np.uint64 if types.is_unsigned_integer_dtype(dt) else np.int64)
        if a.size and (int(a.max()) > AM_EXACT_INT or int(a.min()) < -AM_EXACT_INT):
            raise ValueError(f"column {name!r} of the {kind} frame holds an integer beyond +-2^53, not exact in "
                             "binary64")
        return a.astype(np.float64)
    a = col.to_numpy(dtype=np.float64)
    if not np.isfinite(a).all():
        raise bad
    return a


def _am_prepare(v: pd.DataFrame, e: pd.DataFrame, aggCol, sendToSrc, sendToDst):
    """The host side of aggregateMessages, before any handle: (aggregate, to_src, to_dst, vertex
    columns [n][rows of v], edge columns [n][rows of e])."""
    if sendToSrc is None and sendToDst is None:
        raise ValueError("Either `sendToSrc`, `sendToDst`, or both have to be provided")
    agg = _check_agg_col(aggCol)
    to_src = None if sendToSrc is None else compile_message(sendToSrc)
    to_dst = None if sendToDst is None else compile_message(
        sendToDst, *(() if to_src is None else (to_src.vertex_columns, to_src.edge_columns)))
    last = to_dst if to_dst is not None else to_src
    vcols = [_am_column(v, name, "vertex") for name in last.vertex_columns]
    ecols = [_am_column(e, name, "edge") for name in last.edge_columns]
    return agg, to_src, to_dst, vcols, ecols


# ---- Pregel: vertex programs and the builder (pure host) ----
@dataclass(frozen=True)
class CompiledVertexProgram:
    """A vertex expression as the postfix program the Pregel kernels interpret (include/lpa.h
    ``lpa_vp_program``): ``ops`` are (opcode, 16-bit argument) pairs over ``_lib.VP_OPCODES``, the
    argument an index into ``consts`` or ``columns`` for the opcodes that push."""
    ops: tuple
    consts: tuple
    columns: tuple
    depth: int

    def decode(self) -> MessageExpr:
        """The expression back from the program."""
        st = []
        for code, arg in self.ops:
            op = _lib.VP_OPCODES[code]
            if op == "const":
                st.append(MessageExpr("const", value=self.consts[arg]))
            elif op == "col":
                st.append(MessageExpr("col", value=self.columns[arg]))
            elif op == "msg":
                st.append(MessageExpr("msg"))
            else:
                n = 1 if op in ("neg", "abs", "not", "isnull") else 3 if op == "when_else" else 2
                args = st[len(st) - n:]
                del st[len(st) - n:]
                st.append(MessageExpr("when" if op == "when_else" else op, args))
        assert len(st) == 1
        return st[0]


def compile_vertex_program(expr, columns=(), n_static=None, initial=False) -> CompiledVertexProgram:
    """Compile a vertex expression of Pregel (an initial or an update expression) to its postfix
    program: operands left to right, then their operator.  ``columns``: the vertex columns of the
    run in index order, the ``n_static`` static ones (default: all) and then the Pregel columns;
    ``Pregel.col(name)`` must name one of them.  ``initial=True`` compiles an initial expression,
    which reads static columns and constants only.  Pure host code.  ``ValueError`` for
    ``Pregel.src`` / ``dst`` / ``edge`` inside the expression, an unknown column, the message or
    a Pregel column in an initial expression, and a limit exceeded (AM_MAX_OPS ops, AM_MAX_STACK
    stack values, AM_MAX_CONSTS constants)."""
    root = MessageExpr.of(expr)
    columns = list(columns)
    n_static = len(columns) if n_static is None else int(n_static)
    ops, consts = [], []
    depth = top = 0
    for node in root.walk():
        if node.op in _AM_COLUMN_KINDS:
            raise ValueError(f"{node} appears inside the vertex expression {root}: Pregel.src, Pregel.dst and "
                             "Pregel.edge belong to a message; a vertex reads its own column with Pregel.col")
        if node.op == "msg":
            if initial:
                raise ValueError(f"the initial expression {root} reads the message: no message exists before the "
                                 "first iteration")
            arg, pops = 0, 0
        elif node.op == "const":
            bits = np.float64(node.value).tobytes()   # 0.0 and -0.0 are two constants
            at = [np.float64(c).tobytes() for c in consts]
            if bits not in at:
                consts.append(node.value)
                at.append(bits)
            arg, pops = at.index(bits), 0
        elif node.op == "col":
            if node.value not in columns:
                raise ValueError(f"the vertex expression {root} reads the column {node.value!r}, which is none of: "
                                 f"{','.join(map(str, columns))}")
            arg, pops = columns.index(node.value), 0
            if initial and arg >= n_static:
                raise ValueError(f"the initial expression {root} reads the Pregel column {node.value!r}: it may read "
                                 "columns of the vertex frame and constants only")
        else:
            arg, pops = 0, len(node.args)
        code = "when_else" if node.op == "when" and pops == 3 else node.op
        ops.append((_VP_OPCODE[code], arg))
        depth += 1 - pops
        top = max(top, depth)
    if len(ops) > AM_MAX_OPS:
        raise ValueError(f"the vertex expression {root} compiles to {len(ops)} ops, more than AM_MAX_OPS = "
                         f"{AM_MAX_OPS}")
    if top > AM_MAX_STACK:
        raise ValueError(f"the vertex expression {root} needs a stack of {top} values, more than AM_MAX_STACK = "
                         f"{AM_MAX_STACK}")
    if len(consts) > AM_MAX_CONSTS:
        raise ValueError(f"the vertex expression {root} holds {len(consts)} constants, more than AM_MAX_CONSTS = "
                         f"{AM_MAX_CONSTS}")
    return CompiledVertexProgram(tuple(ops), tuple(consts), tuple(columns), top)


class Pregel:
    """``GraphFrame.pregel``: the builder of ``graphframes.lib.Pregel`` (GraphFrames 0.8) and its
    vocabulary::

        from graphframes_amd import Pregel
        ranks = (g.pregel.setMaxIter(10)
                  .withVertexColumn("rank", Pregel.lit(1.0),
                                    Pregel.coalesce(Pregel.msg(), 0.0) * 0.85 + 0.15)
                  .sendMsgToDst(Pregel.src("rank") * Pregel.src("w"))
                  .aggMsgs(Pregel.sum(Pregel.msg()))
                  .run())

    ``withVertexColumn(name, initialExpr, updateAfterAggMsgsExpr)`` adds a column (1 to
    PREGEL_MAX_COLUMNS) that lives on the GPU across the iterations; ``sendMsgToDst`` /
    ``sendMsgToSrc`` (repeatable, up to PREGEL_MAX_MESSAGES each) add a message along every edge;
    ``aggMsgs`` sets the one aggregate; ``setMaxIter`` (default 10) the number of iterations, all
    of which run: there is no early stop.  ``setCheckpointInterval`` is accepted and ignored.
    ``run()`` returns the vertex rows sorted by ``id`` with the Pregel columns (float64) added.

    In an iteration every edge evaluates the messages over the columns of its ends
    (``Pregel.src(c)``, ``Pregel.dst(c)``: a column of the vertex frame or a Pregel column) and
    its own (``Pregel.edge(c)``); a null message is not delivered; a vertex aggregates what it
    receives into ``Pregel.msg()``, which is null for a vertex that received nothing (for count
    too); every Pregel column then becomes its update expression over the vertex's own columns
    (``Pregel.col(c)``, their values before the iteration) and the message, all columns at once.
    An update expression whose value is null is an error: wrap it in ``Pregel.coalesce``.

    ``Pregel.col``, ``lit``, ``when(...).otherwise(...)``, ``coalesce(a, b)`` and ``isnull(a)``
    stand in for ``pyspark.sql.functions``; the operators, the null rules and the one deviation
    from Spark (``&`` and ``|`` with a null operand give null) are those of
    ``AggregateMessages``, whose aggregates (``AM.sum(AM.msg)``) are accepted too.  Everything is
    IEEE binary64.  Out of scope: early stopping, active-vertex expressions, checkpoints."""

    def __init__(self, graph: "GraphFrame"):
        self._graph = graph
        self._max_iter = 10
        self._columns = []   # (name, initial expression, update expression)
        self._to_src, self._to_dst = [], []
        self._agg = None

    # -- the vocabulary --
    @staticmethod
    def msg():
        return MessageExpr("msg")

    @staticmethod
    def _column(kind, name):
        if not isinstance(name, str):
            raise TypeError(f"Pregel.{kind}(...) takes a column name, got {type(name).__name__}")
        return MessageExpr(kind, value=name)

    @staticmethod
    def src(name): return Pregel._column("src", name)
    @staticmethod
    def dst(name): return Pregel._column("dst", name)
    @staticmethod
    def edge(name): return Pregel._column("edge", name)
    @staticmethod
    def col(name): return Pregel._column("col", name)

    lit = staticmethod(AggregateMessages.lit)
    when = staticmethod(AggregateMessages.when)

    @staticmethod
    def coalesce(a, b):
        """``a`` where it is not null, else ``b``."""
        a, b = MessageExpr.of(a), MessageExpr.of(b)
        return MessageExpr("coalesce", (a, b), is_bool=a.is_bool and b.is_bool)

    @staticmethod
    def isnull(a):
        """True where ``a`` is null; never null itself."""
        return MessageExpr("isnull", (MessageExpr.of(a),), is_bool=True)

    sum = staticmethod(AggregateMessages.sum)
    min = staticmethod(AggregateMessages.min)
    max = staticmethod(AggregateMessages.max)
    avg = staticmethod(AggregateMessages.avg)
    mean = avg
    count = staticmethod(AggregateMessages.count)

    # -- the builder --
    def setMaxIter(self, value):
        if not isinstance(value, (int, np.integer)) or isinstance(value, (bool, np.bool_)):
            raise TypeError(f"maxIter must be an int, got {type(value).__name__}")
        if value < 1:
            raise ValueError(f"maxIter must be at least 1, got {value}")
        self._max_iter = int(value)
        return self

    def setCheckpointInterval(self, value):
        """Accepted for GraphFrames' call surface; nothing is checkpointed."""
        return self

    def withVertexColumn(self, colName, initialExpr, updateAfterAggMsgsExpr):
        if not isinstance(colName, str):
            raise TypeError(f"a Pregel column's name is a str, got {type(colName).__name__}")
        if colName == ID or colName in self._graph.vertices.columns:
            raise ValueError(f"the Pregel column {colName!r} would replace a column of the vertex frame")
        if any(colName == name for name, _, _ in self._columns):
            raise ValueError(f"the Pregel column {colName!r} is defined twice")
        if len(self._columns) == PREGEL_MAX_COLUMNS:
            raise ValueError(f"a run holds at most PREGEL_MAX_COLUMNS = {PREGEL_MAX_COLUMNS} Pregel columns")
        self._columns.append((colName, MessageExpr.of(initialExpr), MessageExpr.of(updateAfterAggMsgsExpr)))
        return self

    def _send(self, to, msgExpr, what):
        if len(to) == PREGEL_MAX_MESSAGES:
            raise ValueError(f"a run holds at most PREGEL_MAX_MESSAGES = {PREGEL_MAX_MESSAGES} {what} messages")
        to.append(MessageExpr.of(msgExpr))
        return self

    def sendMsgToSrc(self, msgExpr):
        return self._send(self._to_src, msgExpr, "sendMsgToSrc")

    def sendMsgToDst(self, msgExpr):
        return self._send(self._to_dst, msgExpr, "sendMsgToDst")

    def aggMsgs(self, aggExpr):
        self._agg = _check_agg_col(aggExpr)
        return self

    def _prepare(self):
        """The host side of run(), before any handle: (aggregate kind, to_src, to_dst, init and
        update programs, the Pregel names, static vertex columns [n][rows of v], edge columns
        [n][rows of e])."""
        v, e = self._graph.vertices, self._graph.edges
        if not self._columns:
            raise ValueError("no vertex column: call withVertexColumn at least once")
        if not self._to_src and not self._to_dst:
            raise ValueError("no message: call sendMsgToSrc, sendMsgToDst, or both")
        if self._agg is None:
            raise ValueError("no aggregate: call aggMsgs")
        pregel_names = [name for name, _, _ in self._columns]
        static = []
        exprs = self._to_src + self._to_dst + [x for _, i, u in self._columns for x in (i, u)]
        for node in (n for x in exprs for n in x.walk()):
            if node.op in ("src", "dst", "col") and node.value not in pregel_names and node.value not in static:
                static.append(node.value)
        names = static + pregel_names
        if len(names) > AM_MAX_VERTEX_COLUMNS:
            raise ValueError(f"the run holds {len(names)} vertex columns ({', '.join(names)}), the Pregel ones "
                             f"included, more than AM_MAX_VERTEX_COLUMNS = {AM_MAX_VERTEX_COLUMNS}")
        vcols = [_am_column(v, name, "vertex") for name in static]
        edge_names = ()
        to_src, to_dst = [], []
        for exprs, out in ((self._to_src, to_src), (self._to_dst, to_dst)):
            for x in exprs:
                out.append(compile_message(x, names, edge_names))
                edge_names = out[-1].edge_columns
        ecols = [_am_column(e, name, "edge") for name in edge_names]
        init = [compile_vertex_program(i, names, len(static), initial=True) for _, i, _ in self._columns]
        update = [compile_vertex_program(u, names, len(static)) for _, _, u in self._columns]
        return self._agg.kind, to_src, to_dst, init, update, pregel_names, vcols, ecols

    def run(self) -> pd.DataFrame:
        """The vertex rows sorted by ``id`` with every Pregel column (float64) after ``maxIter``
        iterations.  Everything that can be refused is refused with ``ValueError`` before any
        device work: no vertex column, message or aggregate; a column the frames lack, that is
        not numeric or bool, or that holds NaN, None, an infinite value or an integer beyond
        +-2^53; an initial expression that reads a Pregel column or the message;
        ``Pregel.src`` / ``dst`` / ``edge`` in a vertex expression, ``Pregel.col`` / ``coalesce``
        / ``isnull`` in a message; a limit exceeded.  An update (or initial) expression whose
        value is null raises ``ValueError`` naming the column and the iteration."""
        agg, to_src, to_dst, init, update, names, vcols, ecols = self._prepare()
        gf = self._graph
        ig = gf._indexed()
        rep = gf._first_rows()
        V, m = ig.num_vertices, int(ig.src.size)
        vc = np.stack([c[rep] for c in vcols]) if vcols else np.empty((0, V), dtype=np.float64)
        ec = np.stack([c[ig.kept] for c in ecols]) if ecols else np.empty((0, m), dtype=np.float64)
        try:
            cols = gf._gpu_graph().pregel(self._max_iter, agg, to_src, to_dst, init, update, vc, ec)
        except PregelNullError as err:
            what = "initial" if err.iteration == 0 else "update"
            raise ValueError(f"Pregel column {names[err.column]!r}: the {what} expression is null in iteration "
                             f"{err.iteration} at the vertex {ig.ids[err.vertex]!r}; a column holds no null: give "
                             "the value to take with Pregel.coalesce(expression, value)") from None
        return _attach(gf.vertices, ig, {name: cols[j] for j, name in enumerate(names)})


def _check_cc_algorithm(algorithm):
    if algorithm not in CC_ALGORITHMS:
        # graphframes.lib.ConnectedComponents.setAlgorithm: require(supportedAlgorithms.contains(value), ...)
        raise ValueError(f"Supported algorithms are {{graphx, graphframes}}: {algorithm}")


def _check_schema(v: pd.DataFrame, e: pd.DataFrame):
    # messages as raised by graphframes.GraphFrame.__init__ (0.6.0)
    if ID not in v.columns:
        raise ValueError("Vertex ID column {} missing from vertex DataFrame, which has columns: {}"
                         .format(ID, ",".join(map(str, v.columns))))
    if SRC not in e.columns:
        raise ValueError("Source vertex ID column {} missing from edge DataFrame, which has columns: {}"
                         .format(SRC, ",".join(map(str, e.columns))))
    if DST not in e.columns:
        raise ValueError("Destination vertex ID column {} missing from edge DataFrame, which has columns: {}"
                         .format(DST, ",".join(map(str, e.columns))))


@dataclass
class IndexedGraph:
    """Dense view of a (vertices, edges) pair: ids sorted ascending, int32 edges."""
    ids: np.ndarray          # unique vertex ids, ascending
    src: np.ndarray          # int32 dense
    dst: np.ndarray          # int32 dense
    integral: bool           # integral ids -> labels are original ids
    dropped_edges: int = 0
    kept: np.ndarray | None = None   # bool per input edge row: both endpoints are vertex ids

    @property
    def num_vertices(self) -> int:
        return int(self.ids.size)


def index_graph(v: pd.DataFrame, e: pd.DataFrame) -> IndexedGraph:
    ids_col = v[ID].to_numpy()
    integral = pd.api.types.is_integer_dtype(v[ID].dtype)
    ids = np.unique(ids_col)
    n = ids.size
    s_raw = e[SRC].to_numpy()
    d_raw = e[DST].to_numpy()
    if n == 0:
        return IndexedGraph(ids, np.empty(0, np.int32), np.empty(0, np.int32), integral, len(e),
                            np.zeros(len(e), bool))
    if integral:
        s_raw = s_raw.astype(ids.dtype, copy=False) if pd.api.types.is_integer_dtype(e[SRC].dtype) else s_raw
        d_raw = d_raw.astype(ids.dtype, copy=False) if pd.api.types.is_integer_dtype(e[DST].dtype) else d_raw
    s = np.searchsorted(ids, s_raw)
    d = np.searchsorted(ids, d_raw)
    s_ok = (s < n)
    d_ok = (d < n)
    s_ok[s_ok] = ids[s[s_ok]] == s_raw[s_ok]
    d_ok[d_ok] = ids[d[d_ok]] == d_raw[d_ok]
    keep = s_ok & d_ok
    return IndexedGraph(ids, s[keep].astype(np.int32), d[keep].astype(np.int32), integral,
                        int((~keep).sum()), keep)


def _label_values(ig: IndexedGraph, dense_labels: np.ndarray) -> np.ndarray:
    if ig.integral:
        return ig.ids[dense_labels].astype(np.int64)
    return dense_labels.astype(np.int64)


def _attach(v: pd.DataFrame, ig: IndexedGraph, per_vertex: dict) -> pd.DataFrame:
    """Vertex rows (sorted by id, all columns kept) + per-vertex columns."""
    out = v.sort_values(ID, kind="stable").reset_index(drop=True)
    pos = np.searchsorted(ig.ids, out[ID].to_numpy())
    for name, values in per_vertex.items():
        out[name] = values[pos]
    return out


class GraphFrame:
    """``graphframes.GraphFrame`` call surface over pandas DataFrames.

    ``GraphFrame(v, e).labelPropagation(maxIter)`` mirrors Graphframes.py:78-81.
    """

    def __init__(self, v: pd.DataFrame, e: pd.DataFrame, device: int = 0):
        _check_schema(v, e)
        self._v = v
        self._e = e
        self._device = device
        self._ig = None
        self._graph = None

    @property
    def vertices(self) -> pd.DataFrame:
        return self._v

    @property
    def edges(self) -> pd.DataFrame:
        return self._e

    def _indexed(self) -> IndexedGraph:
        if self._ig is None:
            self._ig = index_graph(self._v, self._e)
        return self._ig

    def _gpu_graph(self) -> Graph:
        if self._graph is None:
            ig = self._indexed()
            self._graph = Graph(ig.src, ig.dst, ig.num_vertices, device=self._device)
        return self._graph

    def labelPropagation(self, maxIter: int) -> pd.DataFrame:
        """Static LPA for exactly ``maxIter`` synchronous supersteps (GraphX
        LabelPropagation.run via Pregel).  Returns vertices + ``label`` (int64)."""
        _check_max_iter(maxIter)
        ig = self._indexed()
        dense = self._gpu_graph().run(int(maxIter))
        return _attach(self._v, ig, {LABEL: _label_values(ig, dense)})

    def connectedComponents(self, algorithm: str = "graphframes", checkpointInterval: int = 2,
                            broadcastThreshold: int = 1000000) -> pd.DataFrame:
        """``GraphFrame.connectedComponents``: vertices + ``component`` (int64), the
        smallest member of each vertex's connected component (direction, duplicates and
        self-loops ignored) -- its original id for integral ids (the value GraphFrames
        returns), its dense index in ascending id order otherwise, as for ``label``.
        ``algorithm`` must be "graphframes" or "graphx" (both name the one GPU algorithm
        here); ``checkpointInterval`` and ``broadcastThreshold`` steer Spark's execution
        of the GraphFrames algorithm and are accepted and ignored."""
        _check_cc_algorithm(algorithm)
        ig = self._indexed()
        dense = self._gpu_graph().components()
        return _attach(self._v, ig, {COMPONENT: _label_values(ig, dense)})

    def stronglyConnectedComponents(self, maxIter: int) -> pd.DataFrame:
        """``GraphFrame.stronglyConnectedComponents(maxIter)`` (GraphX
        ``lib.StronglyConnectedComponents``): vertices + ``component`` (int64).  Once the
        rounds have converged it is the smallest member of each vertex's strongly connected
        component -- its original id for integral ids (the value GraphFrames returns), its
        dense index in ascending id order otherwise, as for ``label``.  ``maxIter`` bounds
        GraphX's rounds (trim, forward colouring, backward sweep) and the result when it stops
        them early is GraphX's too: a vertex whose component has not been written yet holds
        its own id.  ``maxIter`` is required, as in GraphFrames."""
        _check_scc_max_iter(maxIter)
        ig = self._indexed()
        dense = self._gpu_graph().strongly_connected_components(int(maxIter))
        return _attach(self._v, ig, {COMPONENT: _label_values(ig, dense)})

    def louvain(self, maxLevels: int = 64, maxRounds: int = 1000) -> pd.DataFrame:
        """Louvain community detection -- this package's own addition, not a GraphFrames call
        (like ``clusteringCoefficient`` and ``outlierScores``): a modularity-maximising
        detector on the same symmetrised multigraph ``labelPropagation`` votes on, synchronous
        and deterministic, in exact integer arithmetic (``Graph.louvain`` states the rounds).
        Returns the vertex rows sorted by id + ``label`` (int64): the smallest member of each
        vertex's community -- its original id for integral ids, its dense index in ascending
        id order otherwise, as ``labelPropagation``'s ``label``.  ``outlierScores(labels=...)``
        takes the result as it takes ``labelPropagation``'s.  ``.attrs["modularity"]`` is the
        modularity of the partition, ``.attrs["levels"]`` the list of per-level dicts
        (vertices, communities, rounds, damped_rounds, moves, numerator).  ``maxLevels`` bounds
        the aggregation levels, ``maxRounds`` the rounds of one level (a path or a cycle of n
        vertices needs about n / 2)."""
        _check_louvain(maxLevels, maxRounds)
        ig = self._indexed()
        dense, _, levels, summ = self._gpu_graph().louvain(int(maxLevels), int(maxRounds), stats=True)
        out = _attach(self._v, ig, {LABEL: _label_values(ig, dense)})
        out.attrs["modularity"] = summ["modularity"]
        out.attrs["levels"] = levels
        return out

    def triangleCount(self) -> pd.DataFrame:
        """``GraphFrame.triangleCount``: vertices + ``count`` (int64), the number of
        triangles passing through each vertex.  As in GraphX ``TriangleCount`` the graph
        is first made canonical: self-loops dropped, direction ignored, duplicate edges
        collapsed."""
        ig = self._indexed()
        return _attach(self._v, ig, {COUNT: self._gpu_graph().triangle_count()})

    def clusteringCoefficient(self) -> pd.DataFrame:
        """Local clustering coefficient per vertex -- this package's own addition, not a
        GraphFrames call (like ``degrees`` and ``outlierScores``).  Returns vertices +
        ``count`` (triangles through the vertex, int64), ``degree`` (distinct neighbours
        in the simple undirected graph, int64) and ``lcc`` (float64) =
        2 count / (degree (degree - 1)), 0.0 where degree < 2, computed in numpy from the
        exact integers.  ``.attrs["transitivity"]`` is 3 T / wedges of the whole graph
        (0.0 without wedges)."""
        ig = self._indexed()
        count, deg, summ = self._gpu_graph().triangle_count(stats=True)
        pairs = deg * (deg - 1)
        lcc = np.zeros(count.shape, np.float64)
        np.divide(2.0 * count, pairs, out=lcc, where=pairs > 0)
        out = _attach(self._v, ig, {COUNT: count, "degree": deg, "lcc": lcc})
        wedges = summ["wedges"]
        out.attrs["transitivity"] = 3.0 * summ["n_triangles"] / wedges if wedges > 0 else 0.0
        return out

    def coreNumber(self) -> pd.DataFrame:
        """Core number per vertex (k-core decomposition) -- this package's own addition, not a
        GraphFrames call (like ``clusteringCoefficient`` and ``louvain``).  On the canonical
        simple undirected graph (self-loops dropped, direction ignored, duplicates collapsed, as
        ``triangleCount``), ``core`` (int64) is the largest k such that the vertex lies in a
        subgraph where every vertex has at least k neighbours; 0 without a neighbour.  Returns
        the vertex rows sorted by id, all columns kept, + ``core``.  ``.attrs["degeneracy"]`` is
        the largest core number, ``.attrs["core_sizes"]`` the list ``np.bincount(core)``: the
        vertices of each core number."""
        ig = self._indexed()
        core = self._gpu_graph().core_numbers().astype(np.int64)
        out = _attach(self._v, ig, {CORE: core})
        sizes = np.bincount(core)
        out.attrs["degeneracy"] = max(int(sizes.size) - 1, 0)
        out.attrs["core_sizes"] = [int(x) for x in sizes]
        return out

    def scan(self, epsilon: float = 0.7, mu: int = 2) -> pd.DataFrame:
        """SCAN structural clustering (Xu, Yuruk, Feng, Schweiger, KDD 2007) -- this package's own
        addition, not a GraphFrames call (like ``louvain`` and ``coreNumber``).  On the canonical
        simple undirected graph (self-loops dropped, direction ignored, duplicates collapsed, as
        ``triangleCount``) an edge is similar when the structural similarity of its ends,
        (common neighbours + 2) / sqrt((d[u] + 1) (d[v] + 1)), is at least ``epsilon``; a vertex
        with at least ``mu`` similar closed neighbours (itself counted) is a core; cores joined
        over similar edges form a cluster and similar neighbours of a core are its borders.
        Every other vertex is a hub, when its neighbours lie in at least two clusters, or an
        outlier.  Returns the vertex rows sorted by id, all columns kept, + ``label`` (int64: the
        smallest core of the vertex's cluster, a hub's or outlier's own id -- original ids for
        integral ids, dense indices in ascending id order otherwise, as ``labelPropagation``'s
        ``label``; ``outlierScores(labels=...)`` takes the result) + ``role`` (str: ``core``,
        ``border``, ``hub`` or ``outlier``).  ``.attrs`` holds the summary: simple_edges,
        triangles, similar_edges, n_clusters, n_cores, n_borders, n_hubs, n_outliers,
        largest_cluster and largest_cluster_label (as ``label``; None without a cluster)."""
        epsilon, mu = _check_scan(epsilon, mu, "epsilon")
        ig = self._indexed()
        dense, role, _, summ = self._gpu_graph().scan(epsilon, mu, stats=True)
        names = np.array(SCAN_ROLES, dtype=object)
        out = _attach(self._v, ig, {LABEL: _label_values(ig, dense), ROLE: names[role]})
        big = summ["largest_cluster_label"]
        summ["largest_cluster_label"] = None if big < 0 else int(_label_values(ig, np.array([big]))[0])
        out.attrs.update(summ)
        return out

    def structuralSimilarity(self) -> pd.DataFrame:
        """The per-edge quantities ``scan`` decides by -- this package's own addition.  Returns the
        edge rows whose two ends are vertex ids (the rows the graph keeps), all columns kept, in
        input order, + ``common`` (int64: the common neighbours of the row's ends in the canonical
        simple undirected graph) + ``similarity`` (float64: (common + 2) / sqrt((d[src] + 1)
        (d[dst] + 1)), computed on the host from ``common`` and the simple degrees, for reading
        only: ``scan`` decides by the root-free integer-exact test).  Rows of one edge, in either
        direction, carry the same values.  A self-loop row is no edge of the simple graph: it
        shows ``common`` -1 and ``similarity`` NaN."""
        ig = self._indexed()
        g = self._gpu_graph()
        common = g.scan(1.0, 1, common=True)[2].astype(np.int64)
        deg = g.core_numbers(max_k=0, stats=True)[1].astype(np.float64)
        sim = np.full(common.shape, np.nan, np.float64)
        ok = common >= 0
        sim[ok] = (common[ok] + 2.0) / np.sqrt((deg[ig.src[ok]] + 1.0) * (deg[ig.dst[ok]] + 1.0))
        out = self._e[ig.kept].reset_index(drop=True) if ig.kept is not None else self._e.reset_index(drop=True)
        out[COMMON] = common
        out[SIMILARITY] = sim
        return out

    def _bc_sources(self, sources, k, seed):
        """The dense ids of the sources of ``betweennessCentrality`` (None: every vertex); every
        argument error is raised here, before any device work."""
        V = self._indexed().num_vertices
        if sources is not None and k is not None:
            raise ValueError("betweennessCentrality: give sources or k, not both")
        if k is not None:
            if not isinstance(k, (int, np.integer)) or isinstance(k, (bool, np.bool_)):
                raise TypeError(f"k must be an int, got {type(k).__name__}")
            if not isinstance(seed, (int, np.integer)) or isinstance(seed, (bool, np.bool_)):
                raise TypeError(f"seed must be an int, got {type(seed).__name__}")
            if not 1 <= k <= V:
                raise ValueError(f"k must belong to [1, {V}] (the number of vertices), got {k}")
            return np.sort(np.random.default_rng(int(seed)).choice(V, size=int(k), replace=False)).astype(np.int32)
        if sources is None:
            return None
        if isinstance(sources, (str, bytes)) or not isinstance(sources, (list, tuple, np.ndarray)):
            raise TypeError(f"sources must be a list, tuple or array of vertex ids, got {type(sources).__name__}")
        if isinstance(sources, np.ndarray) and sources.ndim != 1:
            raise TypeError(f"sources must be one-dimensional, got {sources.ndim} dimensions")
        if len(sources) == 0:
            raise ValueError("betweennessCentrality: sources is empty")
        dense = []
        for sid in sources:
            sid = sid.item() if isinstance(sid, np.generic) else sid
            try:
                pos = None if sid is None else self._source_dense(sid)
            except ValueError:
                pos = None
            if pos is None:
                raise ValueError(f"betweennessCentrality: source {sid!r} is not a vertex id")
            dense.append(pos)
        if len(set(dense)) != len(dense):
            raise ValueError("betweennessCentrality: a source is repeated")
        return np.asarray(dense, dtype=np.int32)

    def betweennessCentrality(self, sources=None, k: int | None = None, seed: int = 0, normalized: bool = True,
                              directed: bool = True) -> pd.DataFrame:
        """Betweenness centrality per vertex -- this package's own addition, not a GraphFrames
        call (like ``louvain`` and ``coreNumber``): the share of the shortest paths that pass
        through a vertex, ``networkx.betweenness_centrality``'s definition on the simple graph
        of the input (the distinct edges src -> dst with src != dst: duplicate edges and
        self-loops change nothing).  ``directed=False``: every edge counts in both directions,
        the simple undirected graph of ``triangleCount`` and ``coreNumber``.  Returns the vertex
        rows sorted by id, all columns kept, + ``betweenness`` (float64).  With neither
        ``sources`` nor ``k`` the result is exact (every vertex a source) and equals
        ``networkx.betweenness_centrality(G, normalized=normalized)``.  ``sources`` (a non-empty
        list, tuple or 1-D array of distinct vertex ids) or ``k`` (an int in [1, V]: the pivots
        ``np.sort(np.random.default_rng(seed).choice(V, size=k, replace=False))`` as dense ids,
        ascending id order) give the pivot estimate, the sum over those sources scaled by
        V / |sources| as networkx scales its ``k`` samples.  With raw the unscaled sum:
        ``normalized=False`` gives raw V / |S| (directed) or raw V / |S| / 2 (undirected),
        ``normalized=True`` raw V / |S| / ((V - 1) (V - 2)), all zeros when V <= 2; V counts
        every vertex row.  An id that is no vertex id, a repeat, an empty ``sources`` or both
        ``sources`` and ``k`` raise ``ValueError`` before any device work.  ``.attrs`` holds
        ``sources`` (their number), ``max_depth`` (the largest distance from a source) and
        ``exact`` (bool).  The numbers of shortest paths are binary64, as in networkx: above
        2^53 they are rounded, the result is still deterministic -- bit-identical across runs
        and input edge orders."""
        dense = self._bc_sources(sources, k, seed)
        ig = self._indexed()
        V = ig.num_vertices
        raw, summ = self._gpu_graph().betweenness(dense, directed=bool(directed), stats=True)
        n = V if dense is None else int(dense.size)
        if normalized:
            bc = raw * (V / n) / ((V - 1) * (V - 2)) if V > 2 else np.zeros(V, np.float64)
        else:
            bc = raw * (V / n) if V > 0 else raw
            if not directed:
                bc = bc / 2
        out = _attach(self._v, ig, {BETWEENNESS: bc})
        out.attrs["sources"] = n
        out.attrs["max_depth"] = int(summ["max_depth"])
        out.attrs["exact"] = dense is None
        return out

    def kCore(self, k: int) -> "GraphFrame":
        """The k-core as a graph -- this package's own addition (see ``coreNumber``): the
        sub-multigraph induced by the vertices of core number >= ``k``.  Returns a
        **GraphFrame**, as ``pageRank`` does: ``.vertices`` is the surviving vertex rows, sorted
        by id, all columns kept, + ``core`` (int64) capped at ``k`` (the peeling stops at level
        ``k``); ``.edges`` the input edges whose endpoints both survive, in input order, with
        all their columns -- duplicates and self-loops among survivors included.  ``k = 0``
        keeps every vertex; a ``k`` above the degeneracy gives two empty tables.  The result
        feeds ``labelPropagation``, ``louvain`` and ``outlierScores`` as any GraphFrame: cutting
        to a k-core first is the usual cure for thousands of tiny fringe communities."""
        _check_core_k(k)
        ig = self._indexed()
        core = self._gpu_graph().core_numbers(max_k=int(k)).astype(np.int64)
        vdf = _attach(self._v, ig, {CORE: core})
        vdf = vdf[vdf[CORE].to_numpy() >= k].reset_index(drop=True)
        inside = core >= k
        keep = ig.kept.copy()
        keep[ig.kept] = inside[ig.src] & inside[ig.dst]
        edf = self._e[keep].reset_index(drop=True)
        return GraphFrame(vdf, edf, device=self._device)

    def _source_dense(self, sourceId):
        """Dense id of ``sourceId`` (None: none); a ValueError when it is no vertex id."""
        if sourceId is None:
            return None
        ids = self._indexed().ids
        try:
            pos = int(np.searchsorted(ids, sourceId))
            found = pos < ids.size and bool(ids[pos] == sourceId)
        except TypeError:
            found = False
        if not found:
            raise ValueError(f"sourceId {sourceId!r} is not a vertex id")
        return pos

    def pageRank(self, resetProbability: float = 0.15, sourceId=None, maxIter: int | None = None,
                 tol: float | None = None) -> "GraphFrame":
        """``GraphFrame.pageRank(maxIter=...)``: static PageRank (GraphX
        ``PageRank.runWithOptions``) of the directed multigraph as given -- duplicate edges
        are edges, a sink's mass is lost every superstep, and the ranks are normalised at the
        end to sum to the number of vertices.  ``sourceId``: the personalised form (ranks sum
        to 1).  Returns a **GraphFrame**, as GraphFrames does: ``.vertices`` is the vertex
        rows (sorted by id) + ``pagerank`` (float64), ``.edges`` the edges whose endpoints
        are both vertex ids, in input order, + ``weight`` (float64) = 1 / out-degree of
        ``src``.  ``tol`` (GraphX ``runUntilConvergence``, another algorithm) raises
        ``NotImplementedError``."""
        _check_page_rank(resetProbability, maxIter, tol)
        ig = self._indexed()
        source = self._source_dense(sourceId)
        rank, odeg, _, _ = self._gpu_graph().pagerank(int(maxIter), float(resetProbability), source, stats=True)
        vdf = _attach(self._v, ig, {PAGERANK: rank})
        edf = self._e[ig.kept].reset_index(drop=True)
        edf[WEIGHT] = 1.0 / odeg[ig.src].astype(np.float64)
        return GraphFrame(vdf, edf, device=self._device)

    def parallelPersonalizedPageRank(self, resetProbability: float = 0.15, sourceIds=None,
                                     maxIter: int | None = None) -> "GraphFrame":
        """``GraphFrame.parallelPersonalizedPageRank(resetProbability, sourceIds, maxIter)``
        (GraphX ``PageRank.runParallelPersonalizedPageRank``): the personalised static PageRank
        of ``pageRank(maxIter=..., sourceId=s)`` for every s of ``sourceIds`` in one call.
        Returns a **GraphFrame**, as GraphFrames does: ``.vertices`` is the vertex rows (sorted
        by id) + ``pageranks``, an object column of float64 arrays of length
        ``len(sourceIds)`` whose entry i belongs to ``sourceIds[i]``, in the order given;
        ``.edges`` the edges whose endpoints are both vertex ids, in input order, + ``weight``
        (float64) = 1 / out-degree of ``src``.  A source may repeat: its entries are then equal
        (GraphX keeps only the last of a repeat and gives 0 / 0 for the earlier ones; that
        accident is not reproduced).  ``sourceIds`` (a non-empty list, tuple or 1-D array) and
        ``maxIter`` are required; an id that is no vertex id raises ``ValueError`` before any
        device work."""
        _check_parallel_page_rank(resetProbability, sourceIds, maxIter)
        dense = []
        for sid in sourceIds:
            sid = sid.item() if isinstance(sid, np.generic) else sid
            try:
                pos = None if sid is None else self._source_dense(sid)
            except ValueError:
                pos = None
            if pos is None:
                raise ValueError(f"parallelPersonalizedPageRank: sourceIds entry {sid!r} is not a vertex id")
            dense.append(pos)
        ig = self._indexed()
        g = self._gpu_graph()
        ranks = g.parallel_pagerank(dense, int(maxIter), float(resetProbability))
        _, odeg, _, _ = g.pagerank(1, stats=True)
        V = ig.num_vertices
        per_vertex = np.empty(V, dtype=object)   # element by element: numpy would make a list of rows 2-D
        by_vertex = np.ascontiguousarray(ranks.T)
        for v in range(V):
            per_vertex[v] = by_vertex[v]
        vdf = _attach(self._v, ig, {PAGERANKS: per_vertex})
        edf = self._e[ig.kept].reset_index(drop=True)
        edf[WEIGHT] = 1.0 / odeg[ig.src].astype(np.float64)
        return GraphFrame(vdf, edf, device=self._device)

    def _landmarks_dense(self, landmarks):
        """(the landmarks as given, repeats collapsed; their dense ids); a TypeError when
        ``landmarks`` is no list, tuple or array, a ValueError when one is no vertex id."""
        if isinstance(landmarks, (str, bytes)) or not isinstance(landmarks, (list, tuple, np.ndarray)):
            raise TypeError(f"landmarks must be a list, tuple or array of vertex ids, got {type(landmarks).__name__}")
        if isinstance(landmarks, np.ndarray) and landmarks.ndim != 1:
            raise TypeError(f"landmarks must be one-dimensional, got {landmarks.ndim} dimensions")
        keys, dense = [], []
        for lm in landmarks:
            lm = lm.item() if isinstance(lm, np.generic) else lm
            try:
                pos = None if lm is None else self._source_dense(lm)
            except ValueError:
                pos = None
            if pos is None:
                # GraphFrames: NoSuchVertexException
                raise ValueError(f"shortestPaths: landmark {lm!r} is not a vertex id")
            if pos not in dense:
                keys.append(lm)
                dense.append(pos)
        return keys, dense

    def shortestPaths(self, landmarks) -> pd.DataFrame:
        """``GraphFrame.shortestPaths(landmarks)`` (GraphX ``lib.ShortestPaths``): the vertex
        rows (sorted by id, all columns kept) + ``distances``, an object column of dicts
        ``{landmark id: distance}``: the number of edges on a shortest directed path from the
        vertex to the landmark along src -> dst (0 at the landmark itself).  A landmark that
        cannot be reached is absent from the dict, as in GraphFrames.  The keys are the
        caller's own id values, in the order the landmarks were given, repeats collapsed.
        ``landmarks`` must be a list, tuple or array; a landmark that is no vertex id raises
        ``ValueError`` (GraphFrames: ``NoSuchVertexException``) before any device work; an
        empty list gives ``{}`` for every vertex."""
        keys, dense = self._landmarks_dense(landmarks)
        ig = self._indexed()
        V = ig.num_vertices
        maps = np.empty(V, dtype=object)
        if not keys:
            for v in range(V):
                maps[v] = {}
        else:
            dist = self._gpu_graph().shortest_paths(dense)
            maps[:] = [{keys[l]: int(dist[l, v]) for l in np.flatnonzero(dist[:, v] >= 0)} for v in range(V)]
        return _attach(self._v, ig, {DISTANCES: maps})

    def bfs(self, fromExpr, toExpr, edgeFilter=None, maxPathLength: int = 10, *, maxPaths=None) -> pd.DataFrame:
        """``GraphFrame.bfs(fromExpr, toExpr, edgeFilter, maxPathLength)`` (GraphFrames
        ``lib.BFS``): every shortest path from a vertex satisfying ``fromExpr`` to a vertex
        satisfying ``toExpr`` over the edges satisfying ``edgeFilter`` (``None``: all), of at
        most ``maxPathLength`` edges; self-loops are never on a path, a duplicate edge gives one
        more path.

        Expressions are **pandas** syntax, not Spark SQL: a ``str`` is evaluated with
        ``DataFrame.eval`` on the vertex frame (the edge frame for ``edgeFilter``), so write
        ``"id == 'a'"``, not ``"id = 'a'"``; it must yield a boolean column.  A boolean Series or
        array of the frame's length is taken positionally; a callable is called with the frame.
        Where an id repeats in the vertex frame its first row stands for the vertex.

        The result has two-level columns, the pandas form of Spark's struct columns: the top
        level is ``from, e0, v1, e1, ..., to``, the second every vertex column (vertex groups)
        or every edge column (edge groups), so ``paths["from"]["id"]`` reads as
        ``paths.select("from.id")`` does.  One row per path, sorted by the tuple of input-edge
        row numbers ``(e0, e1, ...)`` (GraphFrames promises no order).  When the two sets share
        a vertex the result is those vertices, sorted by id, under ``from`` and ``to``; when a
        set is empty or no path of at most ``maxPathLength`` edges exists it is
        ``vertices.iloc[0:0]``; neither of the first two touches the GPU.
        ``.attrs["length"]`` is the number of edges of a path (0 for shared vertices, -1 for
        none), ``.attrs["paths"]`` the number of rows.  ``maxPaths``: the paths are counted
        before they are materialised, and a count above it raises ``ValueError``."""
        _check_bfs(maxPathLength, maxPaths)
        v, e = self._v, self._e
        fm = _bfs_mask(v, fromExpr, "fromExpr")
        tm = _bfs_mask(v, toExpr, "toExpr")
        ef = None if edgeFilter is None else _bfs_mask(e, edgeFilter, "edgeFilter")
        ig = self._indexed()
        V = ig.num_vertices
        # the first row of every id stands for the vertex
        pos = np.searchsorted(ig.ids, v[ID].to_numpy())
        rep = np.zeros(V, dtype=np.int64)
        rep[pos[::-1]] = np.arange(len(v) - 1, -1, -1)
        F, T = fm[rep], tm[rep]

        def none():
            out = v.iloc[0:0].copy()
            out.attrs["length"], out.attrs["paths"] = -1, 0
            return out

        if not F.any() or not T.any():
            return none()
        both = np.flatnonzero(F & T)
        if both.size:
            rows = v.iloc[rep[both]].reset_index(drop=True)
            out = pd.concat([rows, rows], axis=1, keys=["from", "to"])
            out.attrs["length"], out.attrs["paths"] = 0, int(both.size)
            return out
        keep = None if ef is None else ef[ig.kept]
        length, level, eidx = self._gpu_graph().bfs(F, T, keep, int(maxPathLength))
        if length <= 0:
            return none()
        n = count_paths(level, ig.src, ig.dst, eidx, length)
        if maxPaths is not None and n > maxPaths:
            raise ValueError(f"bfs: {n} paths of {length} edges, more than maxPaths = {maxPaths}")
        verts, edges = enumerate_paths(level, ig.src, ig.dst, eidx, length)
        in_row = np.flatnonzero(ig.kept)   # edge index of the dense graph -> row of the edge frame
        names, parts = [], []
        for j in range(length + 1):
            names.append("from" if j == 0 else "to" if j == length else f"v{j}")
            parts.append(v.iloc[rep[verts[:, j]]].reset_index(drop=True))
            if j < length:
                names.append(f"e{j}")
                parts.append(e.iloc[in_row[edges[:, j]]].reset_index(drop=True))
        out = pd.concat(parts, axis=1, keys=names)
        out.attrs["length"], out.attrs["paths"] = int(length), int(len(out))
        return out

    def _first_rows(self) -> np.ndarray:
        """The row of the vertex frame that stands for every dense id: the first one."""
        ig = self._indexed()
        pos = np.searchsorted(ig.ids, self._v[ID].to_numpy())
        rep = np.zeros(ig.num_vertices, dtype=np.int64)
        rep[pos[::-1]] = np.arange(len(self._v) - 1, -1, -1)
        return rep

    def _motif_terms(self, parsed: ParsedMotif, plan, want_edges: bool):
        return [(parsed.terms[i].src_var, parsed.terms[i].dst_var, int(parsed.terms[i].negated),
                 int(want_edges and parsed.terms[i].edge is not None)) for i in plan]

    def find(self, pattern: str, *, maxRows=None) -> pd.DataFrame:
        """``GraphFrame.find(pattern)`` (GraphFrames motif finding): structural pattern matching
        such as ``g.find("(a)-[e]->(b); (b)-[e2]->(a)")``.

        A pattern is terms separated by ``;``.  A term is ``(a)-[e]->(b)``, negated with a
        leading ``!``, or a lone vertex ``(a)``; ``()`` and ``[]`` are anonymous.  A named
        vertex is one variable wherever it appears, every ``()`` a fresh one, every positive
        term has its own edge.  A row is one assignment of vertices to the vertex variables and
        of **rows of the edge frame** to the positive terms' edges such that every edge goes
        from its ``src`` variable's vertex to its ``dst`` variable's; a negated term keeps the
        rows for which no edge row goes from its first vertex to its second.  There is one row
        per assignment of all variables, the anonymous ones included, which are then dropped:
        duplicate edges and anonymous elements multiply rows as a chain of joins does, rows are
        never deduplicated, and variables need not be distinct (in
        ``"(a)-[e]->(b); (b)-[e2]->(a)"`` a self-loop matches with ``a == b``; filter
        afterwards, ``m[m["a"]["id"] != m["b"]["id"]]``).  Edges whose ``src`` or ``dst`` is no
        vertex id are no edges.

        Refused with ``ValueError``, before any device work: an empty pattern or a term that
        does not parse; a name used for a vertex and an edge; an edge name in two terms; a
        named edge in a negated term; a negated term with an anonymous vertex or with a vertex
        no positive term binds; positive terms that are not one connected pattern (GraphFrames
        would cross-join); a lone ``(a)`` that occurs in no edge term unless it is the whole
        pattern; a pattern that names nothing; more than 8 positive or 8 negated terms.

        The result has two-level columns, as ``bfs``: the top level is the named elements in
        order of first appearance in the pattern, the second every vertex column (vertex names)
        or every edge column (edge names).  Where an id repeats in the vertex frame its first
        row stands for the vertex.  Rows are sorted by the tuple of (dense vertex id or edge
        row) in column order.  ``.attrs["rows"]`` is the row count, ``.attrs["plan"]`` the terms
        in the order they ran.  An empty result keeps the columns.  ``(a)`` alone returns the
        vertices under ``a`` without touching the GPU.  ``maxRows`` bounds every table,
        intermediate ones too: a step that needs more raises ``ValueError``."""
        parsed = parse_motif(pattern)
        _check_max_rows(maxRows)
        plan = plan_motif(parsed)
        v, e = self._v, self._e
        ig = self._indexed()
        rep = self._first_rows()
        if not plan:
            rows = v.iloc[rep].reset_index(drop=True)
            out = pd.concat([rows], axis=1, keys=[parsed.lone[0]])
            out.attrs["rows"], out.attrs["plan"] = int(len(out)), []
            return out
        terms = self._motif_terms(parsed, plan, True)
        var_of = {nm: i for i, nm in enumerate(parsed.var_names) if nm is not None}
        term_of = {parsed.terms[i].edge: k for k, i in enumerate(plan) if parsed.terms[i].edge is not None}
        vcols, ecols = self._gpu_graph().motif(parsed.n_vars, terms, var_out=sorted(var_of.values()),
                                               max_rows=maxRows)
        cols = [vcols[var_of[nm]] if k == "v" else ecols[term_of[nm]] for nm, k in parsed.names]
        order = np.lexsort(tuple(c for c in reversed(cols)))
        in_row = np.flatnonzero(ig.kept)   # edge index of the dense graph -> row of the edge frame
        parts = []
        for (nm, k), c in zip(parsed.names, cols):
            c = c[order]
            parts.append((v.iloc[rep[c]] if k == "v" else e.iloc[in_row[c]]).reset_index(drop=True))
        out = pd.concat(parts, axis=1, keys=[nm for nm, _ in parsed.names])
        out.attrs["rows"], out.attrs["plan"] = int(len(out)), [str(parsed.terms[i]) for i in plan]
        return out

    def motifCount(self, pattern: str) -> int:
        """The exact number of rows ``find(pattern)`` would return, with nothing materialised:
        every step runs, the last table is only counted.  This package's own addition
        (GraphFrames has ``find(pattern).count()``, which builds the rows first)."""
        parsed = parse_motif(pattern)
        plan = plan_motif(parsed)
        if not plan:
            return int(self._indexed().num_vertices)
        return self._gpu_graph().motif(parsed.n_vars, self._motif_terms(parsed, plan, False), count_only=True)

    def aggregateMessages(self, aggCol, sendToSrc=None, sendToDst=None) -> pd.DataFrame:
        """``GraphFrame.aggregateMessages(aggCol, sendToSrc, sendToDst)``: every edge sends the
        value of ``sendToSrc`` to its source and of ``sendToDst`` to its destination (either may
        be omitted, not both), every vertex aggregates what it receives with ``aggCol``.  The
        expressions are built from ``AggregateMessages`` (used as ``AM``; its docstring has the
        vocabulary, the null rules and the one deviation from Spark): this package's expressions
        over pandas frames, not Spark SQL columns or strings.

        Returns a DataFrame with ``id`` and the aggregate column (``sum(MSG)`` and so on, or the
        alias), one row per vertex that received at least one non-null message, sorted by ``id``.
        Sums, minima, maxima and averages are float64, ``count`` is int64; ``avg`` is
        ``sum / count``.  Edges whose ``src`` or ``dst`` is no vertex id are no edges, a duplicate
        edge sends again, a self-loop with both directions given delivers both messages to its
        vertex; where an id repeats in the vertex frame its first row stands for the vertex.

        Refused with ``ValueError`` before any device work: neither direction given; an
        ``aggCol`` that is not one of the five aggregates of exactly ``AM.msg``; ``AM.msg``
        inside a message; a column the frame lacks; a column that is not numeric or bool; a
        column that holds NaN, None or an infinite value, or an integer beyond +-2^53; a message
        beyond AM_MAX_OPS ops, AM_MAX_STACK stack values or AM_MAX_CONSTS constants, or a call
        that reads more than AM_MAX_VERTEX_COLUMNS vertex or AM_MAX_EDGE_COLUMNS edge columns.
        A bare comparison as a message sends 1.0 or 0.0."""
        agg, to_src, to_dst, vcols, ecols = _am_prepare(self._v, self._e, aggCol, sendToSrc, sendToDst)
        ig = self._indexed()
        rep = self._first_rows()
        V, m = ig.num_vertices, int(ig.src.size)
        vc = np.stack([c[rep] for c in vcols]) if vcols else np.empty((0, V), dtype=np.float64)
        ec = np.stack([c[ig.kept] for c in ecols]) if ecols else np.empty((0, m), dtype=np.float64)
        res = self._gpu_graph().aggregate_messages(to_src, to_dst, vc, ec)
        got = res["count"] > 0
        if agg.kind == "avg":
            values = res["sum"][got] / res["count"][got]
        else:
            values = res[agg.kind][got]
        return pd.DataFrame({ID: ig.ids[got], agg.name: values})

    @property
    def pregel(self) -> Pregel:
        """``GraphFrame.pregel``: a new ``Pregel`` builder over this graph (its docstring has the
        calls, the vocabulary and the semantics)."""
        return Pregel(self)

    def inDegrees(self) -> pd.DataFrame:
        """Vertices + ``inDegree`` (int64): the kept edges ending at each vertex, duplicates
        counted.  Every vertex has a row, with 0 where GraphFrames' property leaves the
        vertex out; a method, like ``degrees``."""
        ig = self._indexed()
        _, _, ideg, _ = self._gpu_graph().pagerank(1, stats=True)
        return _attach(self._v, ig, {"inDegree": ideg})

    def outDegrees(self) -> pd.DataFrame:
        """Vertices + ``outDegree`` (int64): the kept edges leaving each vertex, duplicates
        counted; zeros included, a method (see ``inDegrees``)."""
        ig = self._indexed()
        _, odeg, _, _ = self._gpu_graph().pagerank(1, stats=True)
        return _attach(self._v, ig, {"outDegree": odeg})

    def dense_labels(self, maxIter: int) -> np.ndarray:
        _check_max_iter(maxIter)
        return self._gpu_graph().run(int(maxIter))

    def degrees(self) -> pd.DataFrame:
        """Symmetrised degree per vertex (each directed edge counts at both ends)."""
        ig = self._indexed()
        return _attach(self._v, ig, {"degree": self._gpu_graph().degrees().astype(np.int64)})

    def outlierScores(self, labels: pd.DataFrame | None = None, mode: str = "L1", maxIter: int = 5,
                      subIter: int = 5) -> "OutlierResult":
        return outlier_scores(self._v, self._e, labels=labels, mode=mode, maxIter=maxIter,
                              subIter=subIter, _gf=self)

    def close(self):
        if self._graph is not None:
            self._graph.close()
            self._graph = None


def label_propagation(vertices: pd.DataFrame, edges: pd.DataFrame, maxIter: int,
                      device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).labelPropagation(maxIter)``."""
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.labelPropagation(maxIter)
    finally:
        gf.close()


def connected_components(vertices: pd.DataFrame, edges: pd.DataFrame, device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).connectedComponents()``."""
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.connectedComponents()
    finally:
        gf.close()


def strongly_connected_components(vertices: pd.DataFrame, edges: pd.DataFrame, maxIter: int,
                                  device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).stronglyConnectedComponents(maxIter)``."""
    _check_scc_max_iter(maxIter)
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.stronglyConnectedComponents(maxIter)
    finally:
        gf.close()


def louvain(vertices: pd.DataFrame, edges: pd.DataFrame, maxLevels: int = 64, maxRounds: int = 1000,
            device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).louvain(maxLevels, maxRounds)``."""
    _check_louvain(maxLevels, maxRounds)
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.louvain(maxLevels, maxRounds)
    finally:
        gf.close()


def triangle_count(vertices: pd.DataFrame, edges: pd.DataFrame, device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).triangleCount()``."""
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.triangleCount()
    finally:
        gf.close()


def core_number(vertices: pd.DataFrame, edges: pd.DataFrame, device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).coreNumber()``."""
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.coreNumber()
    finally:
        gf.close()


def scan(vertices: pd.DataFrame, edges: pd.DataFrame, epsilon: float = 0.7, mu: int = 2,
         device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).scan(epsilon, mu)``."""
    _check_scan(epsilon, mu, "epsilon")
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.scan(epsilon, mu)
    finally:
        gf.close()


def structural_similarity(vertices: pd.DataFrame, edges: pd.DataFrame, device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).structuralSimilarity()``."""
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.structuralSimilarity()
    finally:
        gf.close()


def betweenness_centrality(vertices: pd.DataFrame, edges: pd.DataFrame, sources=None, k: int | None = None,
                           seed: int = 0, normalized: bool = True, directed: bool = True,
                           device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).betweennessCentrality(...)``."""
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.betweennessCentrality(sources=sources, k=k, seed=seed, normalized=normalized, directed=directed)
    finally:
        gf.close()


def k_core(vertices: pd.DataFrame, edges: pd.DataFrame, k: int, device: int = 0) -> "GraphFrame":
    """Function form of ``GraphFrame(vertices, edges).kCore(k)``: the k-core as a GraphFrame."""
    _check_core_k(k)
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.kCore(k)
    finally:
        gf.close()


def page_rank(vertices: pd.DataFrame, edges: pd.DataFrame, maxIter: int, resetProbability: float = 0.15,
              sourceId=None, device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).pageRank(resetProbability, sourceId,
    maxIter=maxIter).vertices``: the vertex table + ``pagerank``."""
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.pageRank(resetProbability=resetProbability, sourceId=sourceId, maxIter=maxIter).vertices
    finally:
        gf.close()


def parallel_personalized_page_rank(vertices: pd.DataFrame, edges: pd.DataFrame, sourceIds, maxIter: int,
                                    resetProbability: float = 0.15, device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).parallelPersonalizedPageRank(
    resetProbability, sourceIds, maxIter).vertices``: the vertex table + ``pageranks``."""
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.parallelPersonalizedPageRank(resetProbability=resetProbability, sourceIds=sourceIds,
                                               maxIter=maxIter).vertices
    finally:
        gf.close()


def shortest_paths(vertices: pd.DataFrame, edges: pd.DataFrame, landmarks, device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).shortestPaths(landmarks)``."""
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.shortestPaths(landmarks)
    finally:
        gf.close()


def bfs(vertices: pd.DataFrame, edges: pd.DataFrame, fromExpr, toExpr, edgeFilter=None, maxPathLength: int = 10, *,
        maxPaths=None, device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).bfs(fromExpr, toExpr, edgeFilter,
    maxPathLength, maxPaths=maxPaths)``."""
    _check_bfs(maxPathLength, maxPaths)
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.bfs(fromExpr, toExpr, edgeFilter, maxPathLength, maxPaths=maxPaths)
    finally:
        gf.close()


def find(vertices: pd.DataFrame, edges: pd.DataFrame, pattern: str, *, maxRows=None, device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).find(pattern, maxRows=maxRows)``."""
    parse_motif(pattern)
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.find(pattern, maxRows=maxRows)
    finally:
        gf.close()


def aggregate_messages(vertices: pd.DataFrame, edges: pd.DataFrame, aggCol, sendToSrc=None, sendToDst=None,
                       device: int = 0) -> pd.DataFrame:
    """Function form of ``GraphFrame(vertices, edges).aggregateMessages(aggCol, sendToSrc,
    sendToDst)``; the host checks run before a handle is created."""
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.aggregateMessages(aggCol, sendToSrc=sendToSrc, sendToDst=sendToDst)
    finally:
        gf.close()


def motif_count(vertices: pd.DataFrame, edges: pd.DataFrame, pattern: str, device: int = 0) -> int:
    """Function form of ``GraphFrame(vertices, edges).motifCount(pattern)``."""
    parse_motif(pattern)
    gf = GraphFrame(vertices, edges, device=device)
    try:
        return gf.motifCount(pattern)
    finally:
        gf.close()


@dataclass
class OutlierResult:
    """Outlier stage output.

    communities: one row per community ``label`` with ``size`` (members,
        Graphframes.py:100-104 / the print at :120) and ``incident_edges``
        (distinct directed edges touching it, len(Edges_List) at :115-118).
    vertices: vertex rows + ``label`` (+ ``sub_label`` in L2) + ``outlier`` flag.
    flagged_ids: ids of flagged vertices, ascending.
    summary: counts and the L1 threshold.
    """
    communities: pd.DataFrame
    vertices: pd.DataFrame
    flagged_ids: np.ndarray
    summary: dict = field(default_factory=dict)


def outlier_scores(vertices: pd.DataFrame, edges: pd.DataFrame, labels: pd.DataFrame | None = None,
                   mode: str = "L1", maxIter: int = 5, subIter: int = 5, device: int = 0,
                   _gf: GraphFrame | None = None) -> OutlierResult:
    """Community-size / incident-edge histograms and outlier flags on the GPU.

    ``labels``: a DataFrame with ``id`` and ``label`` as returned by
    ``labelPropagation`` (computed here with ``maxIter`` when omitted).
    mode "L1": threshold rule over top-level community sizes; "L2": second LPA
    (``subIter`` supersteps) on each community's induced, deduplicated edge set
    and the threshold rule per community (the commented Steps 5-6,
    Graphframes.py:121-137).
    """
    if mode not in ("L1", "L2"):
        raise ValueError(f"mode must be 'L1' or 'L2', got {mode!r}")
    gf = _gf if _gf is not None else GraphFrame(vertices, edges, device=device)
    try:
        ig = gf._indexed()
        g = gf._gpu_graph()
        if labels is None:
            _check_max_iter(maxIter)
            dense = g.run(int(maxIter))
        else:
            if ID not in labels.columns or LABEL not in labels.columns:
                raise ValueError("labels must have columns 'id' and 'label'")
            lab = labels.drop_duplicates(ID).set_index(ID)[LABEL]
            lab_vals = lab.reindex(ig.ids).to_numpy()
            if pd.isna(lab_vals).any():
                raise ValueError("labels must cover every vertex id")
            lab_vals = lab_vals.astype(np.int64)
            if ig.integral:
                dense = np.searchsorted(ig.ids, lab_vals)
                if (dense >= ig.num_vertices).any() or (ig.ids[np.minimum(dense, ig.num_vertices - 1)] != lab_vals).any():
                    raise ValueError("labels must be vertex ids")
            else:
                dense = lab_vals
            dense = dense.astype(np.int32)
        res = g.outlier(dense, mode=mode, sub_iter=subIter)
        size, inc, flags = res["size"], res["incident"], res["flags"]
        present = np.flatnonzero(size > 0)
        communities = pd.DataFrame({LABEL: _label_values(ig, present.astype(np.int64)),
                                    "size": size[present], "incident_edges": inc[present]})
        per_vertex = {LABEL: _label_values(ig, dense.astype(np.int64)), "outlier": flags}
        if res["sub_labels"] is not None:
            per_vertex["sub_label"] = _label_values(ig, res["sub_labels"].astype(np.int64))
        vdf = _attach(gf.vertices, ig, per_vertex)
        flagged = ig.ids[np.flatnonzero(flags)]
        return OutlierResult(communities, vdf, flagged, res["summary"])
    finally:
        if _gf is None:
            gf.close()
