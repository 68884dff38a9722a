"""CPU oracle for the LPA + outlier hot path -- TEST INFRASTRUCTURE ONLY.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline``
leg may import this module, and only as the checker.  The product path
(the HIP library behind ``graphframes_amd``) never calls it.

Two restatements of the same semantics:

* ``lpa`` / ``outlier_l1`` / ``outlier_l2`` -- ctypes bindings to ``liboracle.so``
  (``oracle/lpa_oracle.c``, OpenMP C), usable at full test sizes;
* ``lpa_py`` / ``outlier_l1_py`` / ``outlier_l2_py`` -- pure-Python loops, for tiny known-answer
  cases, used to cross-check the C oracle.

Reference anchors: Graphframes.py:81 (``labelPropagation(maxIter=5)``),
Graphframes.py:92-137 (outlier stage), upstream GraphX 2.4.5
``lib/LabelPropagation.scala`` + ``Pregel.scala`` (not vendored; restated).

Parity status: unpinned by the reference itself (it has no tests and prints no
labels); pinned to upstream-suite-shaped KATs and the R9 sample facts.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from collections import Counter

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "liboracle.so")
_lib = None

P_IN_Q32_09 = 3865470566  # floor(0.9 * 2^32): SBM p_in


def build() -> str:
    """Compile oracle/lpa_oracle.c (make) if the .so is missing or stale."""
    src = os.path.join(_HERE, "lpa_oracle.c")
    if (not os.path.exists(_LIB_PATH)) or os.path.getmtime(_LIB_PATH) < os.path.getmtime(src):
        subprocess.run(["make", "-s", "-C", _HERE], check=True)
    return _LIB_PATH


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        build()
    lib = ctypes.CDLL(_LIB_PATH)
    i32p = ctypes.POINTER(ctypes.c_int32)
    i64p = ctypes.POINTER(ctypes.c_int64)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    lib.oracle_lpa.argtypes = [ctypes.c_int32, ctypes.c_int64, i32p, i32p, ctypes.c_int32,
                               i32p, i32p, i64p]
    lib.oracle_lpa.restype = ctypes.c_int
    lib.oracle_superstep_csr.argtypes = [ctypes.c_int32, i64p, i32p, i32p, i32p]
    lib.oracle_superstep_csr.restype = ctypes.c_int
    lib.oracle_build_csr.argtypes = [ctypes.c_int32, ctypes.c_int64, i32p, i32p, i64p, i32p]
    lib.oracle_build_csr.restype = ctypes.c_int
    lib.oracle_outlier_l1.argtypes = [ctypes.c_int32, ctypes.c_int64, i32p, i32p, i32p,
                                      i64p, i64p, u8p, i64p]
    lib.oracle_outlier_l1.restype = ctypes.c_int
    lib.oracle_outlier_l2.argtypes = [ctypes.c_int32, ctypes.c_int64, i32p, i32p, i32p,
                                      ctypes.c_int32, i32p, u8p, i64p]
    lib.oracle_outlier_l2.restype = ctypes.c_int
    lib.oracle_gen_rmat.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64,
                                    ctypes.c_int32, i32p, i32p]
    lib.oracle_gen_rmat.restype = None
    lib.oracle_gen_sbm.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                   ctypes.c_uint32, ctypes.c_uint64, i32p, i32p]
    lib.oracle_gen_sbm.restype = None
    lib.oracle_gen_chunglu.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.oracle_gen_chunglu.restype = ctypes.c_int
    lib.oracle_num_threads.argtypes = []
    lib.oracle_num_threads.restype = ctypes.c_int
    _lib = lib
    return lib


def _p(a, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


def _edges(src, dst):
    s = np.ascontiguousarray(src, dtype=np.int32)
    d = np.ascontiguousarray(dst, dtype=np.int32)
    if s.shape != d.shape:
        raise ValueError("src/dst length mismatch")
    return s, d


def num_threads() -> int:
    return int(_load().oracle_num_threads())


def lpa(V: int, src, dst, max_iter: int, per_iter: bool = False):
    """LPA-DET (App. A).  Returns labels (int32[V]); with per_iter also the
    (max_iter, V) label history and per-superstep tie counts."""
    lib = _load()
    s, d = _edges(src, dst)
    out = np.empty(V, dtype=np.int32)
    hist = np.empty((max_iter, V), dtype=np.int32) if (per_iter and max_iter > 0) else None
    ties = np.empty(max(max_iter, 1), dtype=np.int64)
    rc = lib.oracle_lpa(V, s.size, _p(s, ctypes.c_int32), _p(d, ctypes.c_int32), max_iter,
                        _p(out, ctypes.c_int32),
                        _p(hist, ctypes.c_int32) if hist is not None else None,
                        _p(ties, ctypes.c_int64))
    if rc == -22:
        raise ValueError(f"Maximum of steps must be greater than 0, but got {max_iter}")
    if rc != 0:
        raise MemoryError("oracle_lpa failed")
    if per_iter:
        return out, hist, ties[:max_iter].copy()
    return out


def build_csr(V: int, src, dst):
    lib = _load()
    s, d = _edges(src, dst)
    rp = np.empty(V + 1, dtype=np.int64)
    col = np.empty(max(2 * s.size, 1), dtype=np.int32)
    if lib.oracle_build_csr(V, s.size, _p(s, ctypes.c_int32), _p(d, ctypes.c_int32),
                            _p(rp, ctypes.c_int64), _p(col, ctypes.c_int32)):
        raise MemoryError("oracle_build_csr failed")
    return rp, col[: 2 * s.size]


def superstep_csr(rp, col, cur):
    """One superstep on a prebuilt CSR (bench cpu_baseline timing unit)."""
    lib = _load()
    V = rp.size - 1
    nxt = np.empty(V, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    if col.size == 0:
        col = np.zeros(1, dtype=np.int32)
    lib.oracle_superstep_csr(V, _p(rp, ctypes.c_int64), _p(col, ctypes.c_int32),
                             _p(np.ascontiguousarray(cur, dtype=np.int32), ctypes.c_int32),
                             _p(nxt, ctypes.c_int32))
    return nxt


def outlier_l1(V: int, src, dst, labels):
    """Mode L1 (App. B).  Returns (size[V], inc[V], flags[V] bool, summary dict)."""
    lib = _load()
    s, d = _edges(src, dst)
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    size = np.empty(V, dtype=np.int64)
    inc = np.empty(V, dtype=np.int64)
    flags = np.empty(V, dtype=np.uint8)
    summ = np.empty(4, dtype=np.int64)
    lib.oracle_outlier_l1(V, s.size, _p(s, ctypes.c_int32), _p(d, ctypes.c_int32),
                          _p(lab, ctypes.c_int32), _p(size, ctypes.c_int64),
                          _p(inc, ctypes.c_int64), _p(flags, ctypes.c_uint8),
                          _p(summ, ctypes.c_int64))
    return size, inc, flags.astype(bool), dict(n_groups=int(summ[0]), k=int(summ[1]),
                                                 thr=int(summ[2]), n_flagged=int(summ[3]))


def outlier_l2(V: int, src, dst, labels, sub_iter: int = 5):
    """Mode L2 (App. B).  Returns (sub_labels[V], flags[V] bool, summary dict)."""
    lib = _load()
    s, d = _edges(src, dst)
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    sub = np.empty(V, dtype=np.int32)
    flags = np.empty(V, dtype=np.uint8)
    summ = np.empty(4, dtype=np.int64)
    rc = lib.oracle_outlier_l2(V, s.size, _p(s, ctypes.c_int32), _p(d, ctypes.c_int32),
                               _p(lab, ctypes.c_int32), sub_iter, _p(sub, ctypes.c_int32),
                               _p(flags, ctypes.c_uint8), _p(summ, ctypes.c_int64))
    if rc:
        raise ValueError("oracle_outlier_l2 failed")
    return sub, flags.astype(bool), dict(n_communities=int(summ[0]), n_subgroups=int(summ[1]),
                                         n_flagged=int(summ[2]),
                                         n_communities_flagged=int(summ[3]))


def gen_rmat(scale: int, edgefactor: int = 16, seed: int = 1, scramble: bool = True):
    """CPU restatement of the GPU R-MAT generator (bit-identical by construction)."""
    lib = _load()
    m = edgefactor << scale
    s = np.empty(m, dtype=np.int32)
    d = np.empty(m, dtype=np.int32)
    lib.oracle_gen_rmat(scale, m, seed, int(scramble), _p(s, ctypes.c_int32), _p(d, ctypes.c_int32))
    return s, d


def gen_sbm(V: int, blocks: int, m: int, seed: int = 20261015, p_in_q32: int = P_IN_Q32_09):
    lib = _load()
    s = np.empty(m, dtype=np.int32)
    d = np.empty(m, dtype=np.int32)
    lib.oracle_gen_sbm(V, blocks, m, p_in_q32, seed, _p(s, ctypes.c_int32), _p(d, ctypes.c_int32))
    return s, d


def gen_chunglu(V: int, m: int, gamma: float = 2.1, max_deg: float = 0.0, seed: int = 7):
    """CPU restatement of the GPU Chung-Lu generator (config C5; bit-identical)."""
    lib = _load()
    s = np.empty(m, dtype=np.int32)
    d = np.empty(m, dtype=np.int32)
    if lib.oracle_gen_chunglu(V, m, gamma, max_deg, seed, s.ctypes.data, d.ctypes.data) != 0:
        raise MemoryError("oracle_gen_chunglu: table allocation failed")
    return s, d


# ---------------------------------------------------------------------------
# Pure-Python restatement (tiny cases only): cross-checks the C oracle.
# ---------------------------------------------------------------------------
def lpa_py(V, edges, max_iter):
    """Literal App. A: sendMessage both ways, mergeMessage = Counter sum,
    vertexProgram = most common with smallest label on ties; isolated keep."""
    if max_iter <= 0:
        raise ValueError(f"Maximum of steps must be greater than 0, but got {max_iter}")
    lab = list(range(V))
    for _ in range(max_iter):
        msgs = [Counter() for _ in range(V)]
        for s, d in edges:
            msgs[s][lab[d]] += 1
            msgs[d][lab[s]] += 1
        new = lab[:]
        for v in range(V):
            if msgs[v]:
                best = max(msgs[v].values())
                new[v] = min(l for l, c in msgs[v].items() if c == best)
        lab = new
    return lab


def threshold_rule_py(group_sizes: dict):
    """App. B threshold: sort (size desc, label asc); thr = lst[-k] (k = n//10), lst[0] if k == 0."""
    lst = sorted(group_sizes.items(), key=lambda kv: (-kv[1], kv[0]))
    if not lst:
        return 0
    k = len(lst) // 10
    return lst[-k][1]


def outlier_l1_py(V, edges, labels):
    size = Counter(labels)
    inc = Counter()
    for s, d in dict.fromkeys(tuple(e) for e in edges):
        inc[labels[s]] += 1
        if labels[d] != labels[s]:
            inc[labels[d]] += 1
    thr = threshold_rule_py(size)
    flags = [size[labels[v]] < thr for v in range(V)]
    return size, inc, flags, thr


def outlier_l2_py(V, edges, labels, sub_iter):
    """Literal App. B mode L2: E' = the distinct (s, d) with equal labels, L' = lpa_py on E',
    per community the threshold rule over the counts of its members' sub-labels.
    Returns (sub_labels, flags, summary) with the summary keys of ``outlier_l2``."""
    sub_edges = list(dict.fromkeys((s, d) for s, d in (tuple(e) for e in edges) if labels[s] == labels[d]))
    sub = lpa_py(V, sub_edges, sub_iter)
    groups = Counter((labels[v], sub[v]) for v in range(V))
    thr = {}
    for l in set(labels[:V]):
        thr[l] = threshold_rule_py({g: c for g, c in groups.items() if g[0] == l})
    flags = [groups[(labels[v], sub[v])] < thr[labels[v]] for v in range(V)]
    flagged_communities = {labels[v] for v in range(V) if flags[v]}
    return sub, flags, dict(n_communities=len(thr), n_subgroups=len(groups), n_flagged=sum(flags),
                            n_communities_flagged=len(flagged_communities))
