"""Time Graph.parallel_pagerank() (lpa_parallel_pagerank) on an R-MAT graph generated in HBM.

    python tools/ppr_time.py --scale 24 --edgefactor 16 [--sources 64] [--iters 10] [--batch 16]
                             [--warmup 1] [--calls 5] [--check]

Host wall clock around the blocking call, ranks written into a device tensor.  --sources ids
are drawn with a fixed seed from the vertices that have an out-edge.  --batch sets
LPA_PPR_BATCH before the handle is created (without it the handle takes the library's
default).  A call is the build (once, whatever the number of passes) plus, per pass,
max_iter supersteps and a finish, so the split is taken from two call lengths (medians over
--calls calls after --warmup, alternating the lengths; min and max beside them):

    per iteration per pass   = (t(1 + iters) - t(1)) / iters / batches
    per iteration per source = that / batch_width
    build + finish           = t(1) - batches * per iteration per pass

To compare: tools/pagerank_time.py at the same scale in the same session gives the
single-source per-iteration time (per_iter_ms) and the single-source call (call_ms); this
tool's call_ms for --iters supersteps stands against --sources times that call.  --check
also compares column 0 with Graph.pagerank(source=...) of the same handle against the bound
of tests/pr_ref.py.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=24)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--source-seed", type=int, default=7)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    if a.batch is not None:
        os.environ["LPA_PPR_BATCH"] = str(a.batch)
    import graphframes_amd as gfa
    import torch

    V = 1 << a.scale
    src, dst = gfa.gen_rmat(a.scale, a.edgefactor, seed=a.seed)
    has_out = torch.zeros(V, dtype=torch.bool, device=src.device)
    has_out[src.long()] = True
    cand = torch.nonzero(has_out).flatten()
    gen = torch.Generator().manual_seed(a.source_seed)
    pick = torch.randperm(cand.numel(), generator=gen)[:a.sources]
    sources = [int(x) for x in cand[pick.to(cand.device)].cpu()]
    g = gfa.Graph(src, dst, V)
    del src, dst, has_out, cand
    torch.cuda.empty_cache()
    out = torch.empty((len(sources), V), dtype=torch.float64, device="cuda:0")
    lengths = (1, 1 + a.iters, a.iters)
    for _ in range(a.warmup):
        for k in lengths:
            g.parallel_pagerank(sources, k, out=out)
    ms = {k: [] for k in lengths}
    for _ in range(a.calls):
        for k in lengths:
            t0 = time.perf_counter()
            g.parallel_pagerank(sources, k, out=out)
            ms[k].append(1e3 * (time.perf_counter() - t0))
    _, sums, summ = g.parallel_pagerank(sources, a.iters, out=out, stats=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    batches, width = summ["batches"], summ["batch_width"]
    per_pass = (med[1 + a.iters] - med[1]) / a.iters / batches
    # the spread of the per-iteration figure: the extreme differences of the two call lengths
    lo = (min(ms[1 + a.iters]) - max(ms[1])) / a.iters / batches
    hi = (max(ms[1 + a.iters]) - min(ms[1])) / a.iters / batches
    res = dict(tool="ppr_time", scale=a.scale, edgefactor=a.edgefactor, V=V, sources=len(sources), iters=a.iters,
               calls=a.calls, call_ms=round(med[a.iters], 3), call_min_ms=round(min(ms[a.iters]), 3),
               call_max_ms=round(max(ms[a.iters]), 3), one_iter_call_ms=round(med[1], 3),
               one_iter_call_min_ms=round(min(ms[1]), 3), one_iter_call_max_ms=round(max(ms[1]), 3),
               long_call_ms=round(med[1 + a.iters], 3), long_call_min_ms=round(min(ms[1 + a.iters]), 3),
               long_call_max_ms=round(max(ms[1 + a.iters]), 3),
               per_iter_per_pass_ms=round(per_pass, 4), per_iter_per_source_ms=round(per_pass / width, 4),
               per_iter_per_source_min_ms=round(lo / width, 4), per_iter_per_source_max_ms=round(hi / width, 4),
               build_finish_ms=round(med[1] - batches * per_pass, 3), **summ)
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import pr_ref

        one = torch.empty(V, dtype=torch.float64, device="cuda:0")
        g.pagerank(a.iters, source=sources[0], out=one)
        ref = one.cpu().numpy()
        got = out[0].cpu().numpy()
        pos = ref > 0
        res["worst_rel_diff_vs_single"] = float((abs(got[pos] - ref[pos]) / ref[pos]).max())
        res["same_zero_pattern"] = bool(((got == 0) == (ref == 0)).all())
        res["bound"] = pr_ref.bound(a.iters, summ["max_in_degree"], V)
    g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
