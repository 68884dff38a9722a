"""Time Graph.aggregate_messages() (lpa_aggregate_messages) on an R-MAT graph generated in HBM.

    python tools/am_time.py [--scale 22] [--edgefactor 16] [--warmup 3] [--calls 10] [--timeout 120]

One handle.  "am_ms": sum(AM.src["x"]) sent to dst -- the host wall clock around the blocking call,
median of --calls calls after --warmup warm-ups.  "pagerank_ms": pagerank(1) on the same handle, the
same pull shape (a gather per in-edge, a sum per vertex).  Each call runs under a watchdog of
--timeout seconds that ends the process when the call does not return.  "stages_ms": three more
aggregation calls under LPA_AM_TIMES=1, which synchronises after every stage and prints its
host-clock time (medians): lists (the edge lists and form lists), upload (the program and the
columns), reduce (the three launches), out (the copies to the host).
Bytes per edge of the reduce / the PageRank superstep, as streamed (the gathered column entry is
8 bytes more in either): the aggregation reads an 8-byte edge row and a 4-byte column entry per
row, PageRank a 4-byte column entry.  Prints one JSON line.
"""
import argparse
import faulthandler
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

AM_BYTES_PER_EDGE = 8 + 4
PR_BYTES_PER_EDGE = 4


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
        mark = "lpa_aggregate_messages:"
        self.rows = [{k: float(v) for k, v in re.findall(r"(\w+)=([0-9.]+)", line)}
                     for line in text.splitlines() if line.startswith(mark)]
        rest = [line for line in text.splitlines() if not line.startswith(mark)]
        if rest:
            print("\n".join(rest), file=sys.stderr)


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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=120)
    a = ap.parse_args()
    AM = gfa.AggregateMessages
    V = 1 << a.scale
    src, dst = gfa.gen_rmat(a.scale, a.edgefactor, seed=1)
    out = dict(scale=a.scale, edgefactor=a.edgefactor, V=V, m=int(src.numel()))
    with gfa.Graph(src, dst, V) as g:
        prog = gfa.compile_message(AM.src["x"])
        x = np.random.default_rng(1).random((1, V))
        res = {}

        def am():
            res["am"] = g.aggregate_messages(None, prog, x, None, stats=True)

        def pr():
            res["pr"] = g.pagerank(1, stats=True)

        for name, fn in (("am_ms", am), ("pagerank_ms", pr)):
            ms = [timed(fn, a.timeout) for _ in range(a.warmup + a.calls)][a.warmup:]
            out[name] = dict(spans(ms), calls=[round(x, 1) for x in ms])
        os.environ["LPA_AM_TIMES"] = "1"
        with StageLines() as lines:
            for _ in range(3):
                timed(am, a.timeout)
        del os.environ["LPA_AM_TIMES"]
        out["stages_ms"] = {k: round(statistics.median(r[k] for r in lines.rows), 3)
                            for k in ("lists_ms", "upload_ms", "reduce_ms", "out_ms")} if lines.rows else None
        summ = res["am"][1]
        assert np.array_equal(res["am"][0]["count"], res["pr"][2]), "count of the messages != in-degree"
        out["summary"] = summ
        out["ratio"] = round(out["am_ms"]["med"] / out["pagerank_ms"]["med"], 3)
        out["bytes_per_edge"] = dict(am=AM_BYTES_PER_EDGE, pagerank=PR_BYTES_PER_EDGE,
                                     ratio=AM_BYTES_PER_EDGE / PR_BYTES_PER_EDGE)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
