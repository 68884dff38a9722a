"""Time Graph.motif() (lpa_motif) on an R-MAT graph generated in HBM.

    python tools/motif_time.py --scale 20 --edgefactor 16 [--warmup 1] [--calls 5] [--max-rows N] [--ref]

Five patterns: edge "(a)-[e]->(b)", reciprocal "(a)-[e]->(b); (b)-[e2]->(a)", out-wedge
"(a)-[]->(b); (a)-[]->(c)", the directed 3-cycle "(a)-[]->(b); (b)-[]->(c); (c)-[]->(a)" and
non-reciprocated "(a)-[]->(b); !(b)-[]->(a)", each in the planner's order.  Per pattern:
  count      lpa_motif with count_only (the last table is never filled) under --max-rows:
             "count_ms" (median), the exact row count and the rows after every step; a step
             that needs more than --max-rows is reported as "overflow" with the rows it needed
  full       when no table exceeds --max-rows and the final one --max-out: "lib_ms" = lpa_motif
             into a result object (destroyed, no column copied), "call_ms" = Graph.motif (the
             columns as fresh numpy arrays); medians over --calls calls after --warmup, host
             wall clock around the blocking call
  fill       three more calls under LPA_MOTIF_TIMES=1, which synchronises after every fill and
             prints its host-clock time (medians per step): "fill_rows_per_s" = child rows over fill time summed
             over the filled steps, "fill_hbm_share" = (bytes written + gathered) over that time
             against 8 TB/s.  When the final table is not materialised the lines come from a
             count_only call: the fills of the tables before the last
For the 3-cycle, "triangle_count_ms" is lpa_triangle_count on the same handle, for context (it
counts triangles of the simple undirected graph, not homomorphisms of the multigraph).
--ref: a second, smaller R-MAT (--ref-scale) on which tests/motif_ref.py's merge chain can
finish: its time on this host's CPU, and whether its sorted rows equal the GPU's.  Prints one
JSON line.
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import graphframes_amd as gfa  # noqa: E402
import numpy as np  # noqa: E402

PATTERNS = (("edge", "(a)-[e]->(b)"), ("reciprocal", "(a)-[e]->(b); (b)-[e2]->(a)"),
            ("out_wedge", "(a)-[]->(b); (a)-[]->(c)"), ("cycle3", "(a)-[]->(b); (b)-[]->(c); (c)-[]->(a)"),
            ("one_way", "(a)-[]->(b); !(b)-[]->(a)"))
HBM_BYTES_PER_S = 8e12


class StageLines:
    """stderr (the file descriptor, where the library writes) into a temporary file while active."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        text = self.tmp.read().decode("utf-8", "replace")
        self.tmp.close()
        self.rows = [{k: float(v) for k, v in re.findall(r"(\w+)=([0-9.]+)", line)}
                     for line in text.splitlines() if line.startswith("lpa_motif:")]
        rest = [line for line in text.splitlines() if not line.startswith("lpa_motif:")]
        if rest:
            print("\n".join(rest), file=sys.stderr)


def med(xs):
    return round(statistics.median(xs), 3)


def spans(xs):
    return dict(med=med(xs), min=round(min(xs), 3), max=round(max(xs), 3))


def plan_of(pattern):
    parsed = gfa.parse_motif(pattern)
    plan = gfa.plan_motif(parsed)
    terms = [(parsed.terms[i].src_var, parsed.terms[i].dst_var, int(parsed.terms[i].negated),
              int(parsed.terms[i].edge is not None)) for i in plan]
    named = [v for v, nm in enumerate(parsed.var_names) if nm is not None]
    return parsed, plan, terms, named


def lib_call(g, n_vars, terms, named, cap):
    """lpa_motif into a result object that is destroyed at once; ms."""
    import ctypes

    lib = g._lib
    arr = (gfa._lib.LpaMotifTerm * len(terms))(*[gfa._lib.LpaMotifTerm(*t) for t in terms])
    mask = np.zeros(n_vars, np.uint8)
    mask[named] = 1
    res = ctypes.c_void_p()
    t0 = time.perf_counter()
    rc = lib.lpa_motif(g._handle(), n_vars, mask.ctypes.data_as(gfa._lib._u8p), arr, len(terms), cap, 0,
                       ctypes.byref(res), None)
    ms = 1e3 * (time.perf_counter() - t0)
    lib.lpa_motif_result_destroy(res)
    assert rc == 0, gfa._lib.last_error()
    return ms


def time_pattern(g, pattern, a):
    parsed, plan, terms, named = plan_of(pattern)
    out = dict(pattern=pattern, plan=[str(parsed.terms[i]) for i in plan])
    count_terms = [t[:3] + (0,) for t in terms]
    ms = []
    try:
        for _ in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            rows, summ = g.motif(parsed.n_vars, count_terms, max_rows=a.max_rows, count_only=True, stats=True)
            ms.append(1e3 * (time.perf_counter() - t0))
    except ValueError as e:   # a step above --max-rows
        out["overflow"] = str(e)
        return out, None
    out.update(rows=rows, table_rows=summ["table_rows"], peak_rows=summ["peak_rows"], count_ms=spans(ms[a.warmup:]))
    if rows > a.max_out:
        out["full"] = f"skipped: {rows} rows, more than --max-out"
        # the fills of the tables before the last one, from a count_only call
        fill_stages(out, lambda: g.motif(parsed.n_vars, count_terms, max_rows=a.max_rows, count_only=True))
        return out, None
    lib_ms, call_ms, got = [], [], None
    for _ in range(a.warmup + a.calls):
        lib_ms.append(lib_call(g, parsed.n_vars, terms, named, a.max_rows))
        t0 = time.perf_counter()
        got = g.motif(parsed.n_vars, terms, var_out=named, max_rows=a.max_rows)
        call_ms.append(1e3 * (time.perf_counter() - t0))
    out.update(lib_ms=spans(lib_ms[a.warmup:]), call_ms=spans(call_ms[a.warmup:]))
    fill_stages(out, lambda: lib_call(g, parsed.n_vars, terms, named, a.max_rows))
    return out, (parsed, plan, got)


def fill_stages(out, call, calls=3):
    """`calls` calls under LPA_MOTIF_TIMES=1: the per-step lines (medians over the calls), the
    fill's row rate and HBM share."""
    os.environ["LPA_MOTIF_TIMES"] = "1"
    try:
        with StageLines() as cap:
            for _ in range(calls):
                call()
    finally:
        del os.environ["LPA_MOTIF_TIMES"]
    steps = sorted({int(r["step"]) for r in cap.rows})
    if steps:
        rows = []
        for k in steps:
            mine = [r for r in cap.rows if int(r["step"]) == k]
            rows.append(dict(mine[0], count_ms=med([r["count_ms"] for r in mine]), fill_ms=med([r["fill_ms"] for r in mine]),
                             fill_ms_min=min(r["fill_ms"] for r in mine), fill_ms_max=max(r["fill_ms"] for r in mine)))
        fill_s = 1e-3 * sum(r["fill_ms"] for r in rows)
        out["steps"] = [dict(step=int(r["step"]), parents=int(r["parents"]), rows=int(r["rows"]), count_ms=r["count_ms"],
                             fill_ms=r["fill_ms"], fill_ms_min=r["fill_ms_min"], fill_ms_max=r["fill_ms_max"])
                        for r in rows]
        if fill_s > 0:
            out["fill_rows_per_s"] = round(sum(r["rows"] for r in rows) / fill_s, 1)
            out["fill_hbm_share"] = round(sum(r["fill_bytes"] for r in rows) / fill_s / HBM_BYTES_PER_S, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-rows", type=int, default=1 << 31, help="cap of every table (rows)")
    ap.add_argument("--max-out", type=int, default=1 << 28, help="largest final table that is materialised")
    ap.add_argument("--patterns", default=",".join(k for k, _ in PATTERNS))
    ap.add_argument("--ref", action="store_true")
    ap.add_argument("--ref-scale", type=int, default=12)
    ap.add_argument("--ref-max-rows", type=int, default=2 * 10 ** 7)
    a = ap.parse_args()
    V = 1 << a.scale
    src, dst = gfa.gen_rmat(a.scale, a.edgefactor, seed=a.seed)
    res = dict(tool="motif_time", scale=a.scale, edgefactor=a.edgefactor, V=V, m=int(src.numel()), calls=a.calls,
               max_rows=a.max_rows)
    want = a.patterns.split(",")
    with gfa.Graph(src, dst, V) as g:
        for name, pattern in PATTERNS:
            if name not in want:
                continue
            res[name], _ = time_pattern(g, pattern, a)
            if name == "cycle3":
                ms = []
                for _ in range(a.warmup + a.calls):
                    t0 = time.perf_counter()
                    g.triangle_count()
                    ms.append(1e3 * (time.perf_counter() - t0))
                res[name]["triangle_count_ms"] = spans(ms[a.warmup:])
            print(json.dumps({name: res[name]}), file=sys.stderr, flush=True)
    del src, dst
    if a.ref:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import motif_ref

        Vr = 1 << a.ref_scale
        rs, rd = gfa.gen_rmat(a.ref_scale, a.edgefactor, seed=a.seed)
        s, d = rs.cpu().numpy(), rd.cpu().numpy()
        ref = dict(scale=a.ref_scale, V=Vr, m=int(s.size))
        b = argparse.Namespace(**{**vars(a), "max_rows": a.ref_max_rows, "max_out": a.ref_max_rows})
        with gfa.Graph(rs, rd, Vr) as g:
            for name, pattern in PATTERNS:
                if name not in want:
                    continue
                gpu, got = time_pattern(g, pattern, b)
                if got is None:
                    ref[name] = dict(skipped=gpu.get("overflow") or gpu.get("full"))
                    continue
                parsed, plan, (vcols, ecols) = got
                sp = motif_ref.spec(parsed)
                t0 = time.perf_counter()
                rows = motif_ref.merge_chain(Vr, s, d, *sp)
                ref_ms = round(1e3 * (time.perf_counter() - t0), 1)
                mine = motif_ref.rows_of(vcols, {plan[k]: c for k, c in ecols.items()}, sp[2])
                ref[name] = dict(rows=len(rows), ref_ms=ref_ms, lib_ms=gpu["lib_ms"]["med"],
                                 call_ms=gpu["call_ms"]["med"], ref_equal=bool(mine == rows))
        res["ref"] = ref
    print(json.dumps(res))


if __name__ == "__main__":
    main()
