"""Filtered search on the headline set: the planned path and the time of BOTH paths per selectivity.

31,173 x 768 (bench.py's clustered set and graph), k = 10, 10,000 queries, random masks at selectivities 0.001 ... 0.5.  Per
point: ultra_fast.filtered_plan's choice; the exact scan of the passing rows (hnswgpu_exact_knn_filtered_dev) -- call time,
the time of filtered_group_kernel alone (the handle's profiling events), the row bytes it requests per second against the
gather ceilings DESIGN section 3 quotes, and its fma rate against the chip's f32 VALU rate; the graph walk at the planned ef'
(hnswgpu_hnsw_search_filtered_dev; the library serves ef <= 4096, larger plans are timed there and marked).

The IVF leg (an index this tool builds on the same rows: --ivf-nlist lists, --ivf-nprobe probes, --ivf-nq queries per call), at
the same selectivities: the filtered list scan (hnswgpu_ivf_search_filtered_dev) against default-filtered-search's equivalent --
the unfiltered hnswgpu_ivf_search_dev at 3k and the take of the first k passing entries (on the device, torch) -- and the
unfiltered call at k, the baseline; the mean number of results per query each returns.  The two are timed alternately, --rounds
windows of --reps calls each between device events, and the median window is reported.  Writes profiles/filtered_search.txt.

    python tools/filtered_sweep.py [--legs hnsw,ivf] [--nq 10000] [--reps 5] [--out profiles/filtered_search.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (the headline set, its builder and the gather ceilings)

SELECTIVITIES = [0.001, 0.002, 0.005, 0.01, 0.02, 0.03, 0.05, 0.1, 0.2, 0.5]
VALU_FMA_PER_S = 256 * 4 * 32 * 2.4e9   # 256 CUs x 4 SIMDs x 32 lanes, one f32 fma per lane and clock at 2.4 GHz


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternated(fns, reps, rounds):
    """Median per-call time of every fn, their windows alternating (other work shares the machine: a drift hits them alike)."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t[i].append(window(fn, reps))
    return [float(np.median(x)) for x in t]


def ivf_leg(args, base, n, dim, k):
    from hnsw_clj_amd import engine

    dev = torch.device("cuda", 0)
    nq, nprobe = args.ivf_nq, args.ivf_nprobe
    Q = torch.from_numpy(bench.make_31k("clustered", 43, nq)).to(dev)
    idx = engine.Index(base, "cosine", 0)
    idx.ivf_build(args.ivf_nlist, 5, 42)
    mk = lambda kk: (torch.empty((nq, kk), dtype=torch.int32, device=dev), torch.empty((nq, kk), dtype=torch.float32, device=dev))  # noqa: E731
    out_f, out_u, out_3 = mk(k), mk(k), mk(3 * k)
    lines = ["",
             "IVF-FLAT filtered search, %d x %d cosine, %d lists (5 Lloyd iterations), nprobe %d, k = %d, %d queries per call"
             % (n, dim, args.ivf_nlist, nprobe, k, nq),
             "median of %d alternating windows of %d calls; default = hnswgpu_ivf_search_dev at 3k + the take of the first k passing entries"
             % (args.rounds, args.reps),
             "",
             "%8s %7s | %11s %8s | %10s %8s | %12s" % ("select.", "p", "filtered ms", "results", "default ms", "results", "unfiltered ms")]
    for s in SELECTIVITIES:
        bits = np.random.default_rng(int(s * 1e6)).random(n) < s
        p = int(bits.sum())
        mask = torch.from_numpy(engine.pack_mask(bits, n).view(np.int32).copy()).to(dev)
        bits_d = torch.from_numpy(bits).to(dev)
        taken = {}

        def default():
            ids, d = idx.ivf_search_dev(Q, 3 * k, nprobe, out=out_3)
            ok = (ids >= 0) & bits_d[ids.clamp(min=0).long()]
            keep = ok & (torch.cumsum(ok, 1) <= k)
            taken["n"] = keep.sum()

        t_f, t_d, t_u = alternated([lambda: idx.ivf_search_filtered_dev(Q, k, nprobe, mask, out=out_f), default,
                                    lambda: idx.ivf_search_dev(Q, k, nprobe, out=out_u)], args.reps, args.rounds)
        res_f = float((out_f[0] >= 0).sum().item()) / nq
        res_d = float(taken["n"].item()) / nq
        lines.append("%8.3f %7d | %11.3f %8.2f | %10.3f %8.2f | %12.3f" % (s, p, t_f, res_f, t_d, res_d, t_u))
    idx.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="hnsw,ivf")
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ivf-nq", type=int, default=1024)
    ap.add_argument("--ivf-nlist", type=int, default=128)
    ap.add_argument("--ivf-nprobe", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_search.txt"))
    args = ap.parse_args()
    legs = args.legs.split(",")

    from hnsw_clj_amd import engine, ultra_fast

    dev = torch.device("cuda", 0)
    n, dim, k = bench.N31K, bench.DIM, bench.K
    base = bench.make_31k("clustered", 42, n)
    lines = []
    if "hnsw" in legs:
        lines += hnsw_leg(args, engine, ultra_fast, dev, base, n, dim, k)
    if "ivf" in legs:
        lines += ivf_leg(args, base, n, dim, k)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


def hnsw_leg(args, engine, ultra_fast, dev, base, n, dim, k):
    Q = torch.from_numpy(bench.make_31k("clustered", 43, args.nq)).to(dev)
    idx = engine.Index(base, "cosine", 0)
    idx.hnsw_build(bench.M, bench.EFC, 42, **bench.BUILDERS["heuristic"])
    out = (torch.empty((args.nq, k), dtype=torch.int32, device=dev), torch.empty((args.nq, k), dtype=torch.float32, device=dev))
    tq = 32                                                     # queries per resident group at ld 768
    groups = (args.nq + tq - 1) // tq
    lines = ["filtered search, %d x %d cosine, k = %d, %d queries per call, %d timed calls per figure" % (n, dim, k, args.nq, args.reps),
             "gather ceilings (DESIGN section 3): %.1f-%.1f TB/s Infinity-Cache resident, %.1f-%.1f TB/s beyond it; f32 VALU rate %.1f T fma/s"
             % (bench.IC_GATHER_GBS[0] / 1e3, bench.IC_GATHER_GBS[1] / 1e3, bench.HBM_GATHER_GBS[0] / 1e3, bench.HBM_GATHER_GBS[1] / 1e3,
                VALU_FMA_PER_S / 1e12),
             "",
             "%8s %7s %6s %6s | %9s %9s %9s %8s | %9s %5s | %s" % ("select.", "p", "plan", "ef'", "scan ms", "kernel ms", "rows TB/s", "fma frac",
                                                                  "graph ms", "ef", "faster")]
    crossover = None
    for s in SELECTIVITIES:
        bits = np.random.default_rng(int(s * 1e6)).random(n) < s
        p = int(bits.sum())
        plan, ef2 = ultra_fast.filtered_plan(n, p, k)
        mask = torch.from_numpy(engine.pack_mask(bits, n).view(np.int32).copy()).to(dev)
        scan_ms = timed(lambda: idx.exact_knn_filtered_dev(Q, k, mask, out=out), args.reps)
        idx.set_profiling(True)
        idx.get_profile(engine.PROF_IVF_SCAN, reset=True)
        for _ in range(args.reps):
            idx.exact_knn_filtered_dev(Q, k, mask, out=out)
        kern_ms, launches = idx.get_profile(engine.PROF_IVF_SCAN, reset=True)
        idx.set_profiling(False)
        kern_ms = kern_ms / max(launches, 1)
        row_tbs = groups * p * 4.0 * dim / (kern_ms * 1e-3) / 1e12 if kern_ms > 0 else float("nan")
        fma = args.nq * float(p) * dim / (kern_ms * 1e-3) / VALU_FMA_PER_S if kern_ms > 0 else float("nan")
        ef_run = min(ef2, 4096)
        graph_ms = timed(lambda: idx.hnsw_search_filtered_dev(Q, k, mask, ef_run, out=out), args.reps)
        faster = "scan" if scan_ms <= graph_ms else "graph"
        if crossover is None and faster == "graph":
            crossover = s
        lines.append("%8.3f %7d %6s %6d | %9.3f %9.3f %9.2f %8.2f | %9.3f %5d%s | %s%s"
                     % (s, p, plan, ef2, scan_ms, kern_ms, row_tbs, fma, graph_ms, ef_run, "*" if ef_run != ef2 else " ", faster,
                        "" if faster == plan else "  (plan: %s)" % plan))
    lines += ["",
              "* the plan's ef' exceeds the library's limit of 4096: the graph walk is timed at 4096 (and cannot expect 3k passing entries)",
              "rule: scan while p^2 <= 3 k n (p <= ef') or 3 k n / p > 1024 -- at this n and k up to p = 967 (3.1 %)",
              "measured: the graph walk is the faster path from selectivity %s" % ("%.3f" % crossover if crossover else "> 0.5 (never in this sweep)")]
    idx.close()
    return lines


if __name__ == "__main__":
    main()
