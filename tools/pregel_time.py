"""Time Graph.pregel() (lpa_pregel) on an R-MAT graph generated in HBM.

    python tools/pregel_time.py [--scale 22] [--edgefactor 16] [--iters 10] [--warmup 3] [--calls 10] [--timeout 120]

One handle, one program: PageRank as a Pregel program (static w = 1 / outDegree, 0.0 at sinks;
send src.rank * src.w to dst; sum; rank' = 0.15 + 0.85 * coalesce(msg, 0.0); rank starts at 1.0).
    "pregel_ms"    Graph.pregel with --iters iterations
    "pregel1_ms"   the same call with one iteration: "per_iteration_ms" = (pregel - pregel1) / (iters - 1)
    "loop_ms"      the same --iters rounds as a Python loop around Graph.aggregate_messages, the
                   update in numpy: what a user had before lpa_pregel
    "pagerank_ms"  Graph.pagerank(--iters) on the same handle
Each is the host wall clock around the blocking call, median of --calls calls after --warmup
warm-ups; each call runs under a watchdog of --timeout seconds that ends the process when the call
does not return.  The three results are compared (normalised ranks, relative difference) before
anything is printed.  Prints one JSON line.
"""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import graphframes_amd as gfa  # noqa: E402
import numpy as np  # noqa: E402


def timed(fn, limit):
    """fn() under its own watchdog; ms."""
    faulthandler.dump_traceback_later(limit, exit=True)
    try:
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)
    finally:
        faulthandler.cancel_dump_traceback_later()


def spans(xs):
    return dict(med=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=120)
    a = ap.parse_args()
    if a.iters < 2:
        ap.error("--iters must be at least 2")
    P = gfa.Pregel
    V = 1 << a.scale
    src, dst = gfa.gen_rmat(a.scale, a.edgefactor, seed=1)
    out = dict(scale=a.scale, edgefactor=a.edgefactor, V=V, m=int(src.numel()), iters=a.iters)
    with gfa.Graph(src, dst, V) as g:
        _, outdeg, _, _ = g.pagerank(1, stats=True)
        w = np.zeros((1, V))
        np.divide(1.0, outdeg, out=w[0], where=outdeg > 0)
        names = ["w", "rank"]
        send = gfa.compile_message(P.src("rank") * P.src("w"), names)
        init = gfa.compile_vertex_program(P.lit(1.0), names, 1, initial=True)
        update = gfa.compile_vertex_program(0.15 + 0.85 * P.coalesce(P.msg(), 0.0), names, 1)
        res = {}

        def pregel(iters):
            res["pregel"] = g.pregel(iters, "sum", [], [send], [init], [update], w, None, stats=True)

        def loop():
            cols = np.concatenate([w, np.ones((1, V))])
            for _ in range(a.iters):
                got = g.aggregate_messages(None, send, cols, None)
                cols[1] = 0.15 + 0.85 * got["sum"]
            res["loop"] = cols[1]

        def pagerank():
            res["pagerank"] = g.pagerank(a.iters)

        for name, fn in (("pregel_ms", lambda: pregel(a.iters)), ("pregel1_ms", lambda: pregel(1)), ("loop_ms", loop),
                         ("pagerank_ms", pagerank)):
            ms = [timed(fn, a.timeout) for _ in range(a.warmup + a.calls)][a.warmup:]
            out[name] = dict(spans(ms), calls=[round(x, 1) for x in ms])
        timed(lambda: pregel(a.iters), a.timeout)
        rank, summ = res["pregel"]
        rank = rank[0] * (V / rank[0].sum())
        for other in ("loop", "pagerank"):
            r = res[other] * (V / res[other].sum())
            out[f"max_rel_diff_{other}"] = float(np.max(np.abs(rank - r) / r))
            assert out[f"max_rel_diff_{other}"] < 1e-9, other
        out["summary"] = summ
        out["per_iteration_ms"] = round((out["pregel_ms"]["med"] - out["pregel1_ms"]["med"]) / (a.iters - 1), 3)
        out["loop_over_pregel"] = round(out["loop_ms"]["med"] / out["pregel_ms"]["med"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
