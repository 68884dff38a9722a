"""Time Graph.bfs() (lpa_bfs) on an R-MAT graph generated in HBM, beside lpa_shortest_paths.

    python tools/bfs_time.py --scale 22 --edgefactor 16 [--warmup 1] [--calls 5] [--ref]

One source (the vertex of highest out-degree), no edge filter, two workloads:
  far    the target is a vertex at the largest finite distance from the source (the smallest such
         id), so the forward search expands L levels, one fewer than a full search;
  near   the target is an out-neighbour of an out-neighbour (distance 2): the early stop.
Host wall clock around the blocking call, medians over --calls calls after --warmup: "call_ms"
is Graph.bfs (fresh numpy outputs, the marked edges as an index array), "lib_ms" lpa_bfs itself
into buffers that live across the calls.  A handle
created under LPA_BFS_TIMES=1 prints one line of stage times per call on stderr (host clocks
between the synchronisations the call makes anyway, plus one after the backward sweep); they are
collected through a redirected stderr and give the build / forward / backward / mark shares
("sets": the masks counted on the host; "other": the rest of the call, the temporaries given back).
"arcs_per_s" is the distinct arcs over the forward time (the usual traversed-edges rate of a
full-graph search; the near workload stops early, so there it is only an upper-bound style
figure and is left out).  `far` runs under each schedule: the default switch, LPA_BFS_ALPHA=0
(push only) and LPA_BFS_PULL=1 (pull only), each on a handle of its own; results are compared.
The comparison: lpa_shortest_paths with the source as the single landmark on the TRANSPOSED edge
list does the same traversal (all levels, 64-bit words); its calls alternate with the far calls
of the default schedule.  Its distances also choose the targets.  --ref compares level and the
marked edges with tests/bfs_ref.py on this host's CPU.  Prints one JSON line.
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
import torch  # noqa: E402

SCHEDULES = (("default", {}), ("push_only", {"LPA_BFS_ALPHA": "0"}), ("pull_only", {"LPA_BFS_PULL": "1"}))
STAGES = ("sets", "build", "forward", "backward", "mark", "other")


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
        self.rows = [{k: float(v) for k, v in re.findall(r"(\w+)_ms=([0-9.]+)", line)}
                     for line in text.splitlines() if line.startswith("lpa_bfs:")]
        rest = [line for line in text.splitlines() if not line.startswith("lpa_bfs:")]
        if rest:
            print("\n".join(rest), file=sys.stderr)


def med(xs):
    return round(statistics.median(xs), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--schedules", default="default,push_only,pull_only")
    ap.add_argument("--ref", action="store_true")
    a = ap.parse_args()
    V = 1 << a.scale
    src, dst = gfa.gen_rmat(a.scale, a.edgefactor, seed=a.seed)
    res = dict(tool="bfs_time", scale=a.scale, edgefactor=a.edgefactor, V=V, m=int(src.numel()), calls=a.calls)
    # the transposed graph: the comparison call, and the distances that choose the targets
    gt = gfa.Graph(dst, src, V)
    rank = torch.empty(V, dtype=torch.float64, device="cuda:0")
    _, _, indeg_t, _ = gt.pagerank(1, out=rank, stats=True)    # in-degree of the transpose = out-degree
    source = int(torch.argmax(indeg_t).item())
    del rank, indeg_t
    dist, sp_summ = gt.shortest_paths([source], stats=True)
    dist = dist[0]
    L = int(dist.max())
    far, near = int(np.flatnonzero(dist == L)[0]), int(np.flatnonzero(dist == 2)[0])
    res.update(source=source, far_target=far, far_distance=L, near_target=near, reached=int((dist >= 0).sum()))
    F = np.zeros(V, bool)
    F[source] = True
    T = {"far": np.zeros(V, bool), "near": np.zeros(V, bool)}
    T["far"][far] = True
    T["near"][near] = True
    # the library call alone, into buffers that live across the calls
    level_buf, edge_buf = np.empty(V, np.int32), np.empty(int(src.numel()), np.uint8)
    i32p = gfa._lib._i32p

    def u8(x):
        return x.view(np.uint8).ctypes.data_as(gfa._lib._u8p)

    os.environ["LPA_BFS_TIMES"] = "1"
    first = None
    for name, env in SCHEDULES:
        if name not in a.schedules.split(","):
            continue
        for key, val in env.items():
            os.environ[key] = val
        g = gfa.Graph(src, dst, V)
        for key in env:
            del os.environ[key]
        loads = ("far", "near") if name == "default" else ("far",)
        ms = {k: [] for k in loads}
        lib_ms = {k: [] for k in loads}
        sp_ms = []
        with StageLines() as cap:
            for it in range(a.warmup + a.calls):
                for k in loads:
                    t0 = time.perf_counter()
                    g.bfs(F, T[k], None, 1 << 20)
                    ms[k].append(1e3 * (time.perf_counter() - t0))
                    t0 = time.perf_counter()
                    rc = g._lib.lpa_bfs(g._handle(), u8(F), u8(T[k]), None, 1 << 20, level_buf.ctypes.data_as(i32p),
                                        u8(edge_buf), None)
                    lib_ms[k].append(1e3 * (time.perf_counter() - t0))
                    assert rc == 0
                if name == "default":   # alternating with the comparison call
                    t0 = time.perf_counter()
                    gt.shortest_paths([source])
                    sp_ms.append(1e3 * (time.perf_counter() - t0))
        rows = {k: cap.rows[2 * i + 1::2 * len(loads)][a.warmup:] for i, k in enumerate(loads)}   # the library calls' lines
        out = {}
        for k in loads:
            length, level, eidx, summ = g.bfs(F, T[k], None, 1 << 20, stats=True)
            t, tl = ms[k][a.warmup:], lib_ms[k][a.warmup:]
            st = {s: med([r[s] for r in rows[k]]) for s in STAGES}
            out[k] = dict(call_ms=med(t), call_min_ms=round(min(t), 3), call_max_ms=round(max(t), 3),
                          lib_ms=med(tl), lib_min_ms=round(min(tl), 3), lib_max_ms=round(max(tl), 3),
                          **{s + "_ms": v for s, v in st.items()}, **summ)
            if k == "far":
                out[k]["arcs_per_s"] = round(summ["arcs"] / (st["forward"] * 1e-3), 1)
                if first is None:
                    first = (length, level, eidx)
                out[k]["same_as_first"] = bool(length == first[0] and np.array_equal(level, first[1])
                                               and np.array_equal(eidx, first[2]))
        if name == "default":
            t = sp_ms[a.warmup:]
            res["shortest_paths_transposed"] = dict(call_ms=med(t), call_min_ms=round(min(t), 3),
                                                    call_max_ms=round(max(t), 3), **sp_summ)
        g.close()
        res[name] = out
    gt.close()
    if a.ref:
        print(json.dumps(dict(res, note="GPU done, numpy reference running")), flush=True)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import bfs_ref

        s, d = src.cpu().numpy(), dst.cpu().numpy()
        t0 = time.perf_counter()
        ref = bfs_ref.levels_dag(V, s, d, F, T["far"], None, 1 << 20)
        res["ref_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        res["ref_equal"] = bool(ref["length"] == first[0] and np.array_equal(ref["level"], first[1])
                                and np.array_equal(np.flatnonzero(ref["on_edge"]), first[2]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
