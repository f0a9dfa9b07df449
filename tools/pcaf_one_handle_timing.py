"""P-HNSW search: the one-handle path (hnswgpu_pcaf_search_dev: projection, filter, merge + refine) beside the three-handle
composition (hnswgpu_dense_distances_dev, hnswgpu_exact_knn_dev, hnswgpu_rerank_dev) it can replace, in one process on one card.

100,000 x 768 clustered, normalised rows (bench.py's generator), n_components 100, k 10, k_filter 32; batches of 1, 32 and 1024
queries resident on the device.  Per batch size both paths are warmed up, then timed call by call with device events, the two
alternating; the median of --reps calls and the range are written.  Before timing, the two paths' results are compared (ids
equal on all but a few queries whose kf-th and (kf + 1)-th projected distances tie within f32 rounding; distances within 1e-4).

    python tools/pcaf_one_handle_timing.py [--reps 50] [--out profiles/pcaf_one_handle_vs_composition.txt] [--kernels DIR]

Kernel times and launch counts come from a collection of their own, per batch size:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/nq<NQ> -- python tools/pcaf_one_handle_timing.py --trace NQ

--trace runs TRACE_CALLS searches of each path at one batch size and nothing else after the indexes are made; --kernels DIR reads
DIR/nq<NQ>/**/*kernel_stats.csv and appends, per path, the kernels of a search, their launches per search and mean times, and the
filter kernel's bytes per second: the projected rows (n x Tp x 4 B + norms) once per block of 32 queries over its mean time.
"""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T, K, KF = 100000, 100, 10, 32
BATCHES = (1, 32, 1024)
TRACE_CALLS = 20
COPY_CEILING = 6.29e12  # B/s: the measured device copy the project's roofline figures use


def setting():
    import torch

    import bench
    from hnsw_clj_amd import datagen, pcaf

    base = bench.make_31k("clustered", 42, N)
    Q = bench.make_31k("clustered", 43, max(BATCHES))
    data = datagen.indexed(base)
    one = pcaf.build_index(data, n_components=T, k_filter=KF, one_handle=True)
    three = pcaf.build_index(data, n_components=T, k_filter=KF)
    return pcaf, one, three, torch.from_numpy(Q).to("cuda:0")


def measure(reps, out):
    import torch

    pcaf, one, three, Q = setting()
    lines = ["P-HNSW search, %d x %d rows, n_components %d, k %d, k_filter %d; ms per call, median (min - max) of %d calls"
             % (N, Q.shape[1], T, K, KF, reps), "%6s  %28s  %28s  %s" % ("nq", "composition (three handles)", "one handle", "ratio")]
    for nq in BATCHES:
        q = Q[:nq].contiguous()
        paths = {"three": lambda: pcaf.search_batch_dev(three, q, K), "one": lambda: pcaf.search_batch_dev(one, q, K)}
        for _ in range(5):
            res = {name: fn() for name, fn in paths.items()}
        torch.cuda.synchronize()
        same = (res["one"][0] == res["three"][0]).all(dim=1).sum().item()
        assert same >= nq - max(1, nq // 8), "ids differ on %d of %d queries" % (nq - same, nq)
        assert torch.allclose(torch.sort(res["one"][1]).values, torch.sort(res["three"][1]).values, rtol=1e-4, atol=1e-4)
        ms = {name: [] for name in paths}
        for _ in range(reps):
            for name, fn in paths.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        cell = {name: "%8.4f (%7.4f - %7.4f)" % (np.median(v), min(v), max(v)) for name, v in ms.items()}
        lines.append("%6d  %28s  %28s  %.2f" % (nq, cell["three"], cell["one"], np.median(ms["one"]) / np.median(ms["three"])))
        print(lines[-1], flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def trace(nq):
    import torch

    pcaf, one, three, Q = setting()
    q = Q[:nq].contiguous()
    for index in (three, one):
        for _ in range(TRACE_CALLS):
            pcaf.search_batch_dev(index, q, K)
        torch.cuda.synchronize()


def kernels(directory, out):
    tp = (T + 7) // 8 * 8
    lines = ["", "Kernels of a search (rocprofv3 --kernel-trace --stats, %d searches per path; kernels with fewer calls belong "
             "to the indexes' construction, and the projection kernel's mean includes its one build launch): launches per search, "
             "mean us" % TRACE_CALLS]
    for nq in BATCHES:
        rows = []
        for path in glob.glob(os.path.join(directory, "nq%d" % nq, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows += list(csv.DictReader(f))
        lines.append("nq %d" % nq)
        total = 0.0
        for r in sorted(rows, key=lambda r: r["Name"]):
            calls, mean_us = int(r["Calls"]), float(r["AverageNs"]) / 1e3
            if calls < TRACE_CALLS:  # (the indexes' construction)
                continue
            name = r["Name"].split("(")[0][-70:]
            lines.append("  %-70s %3d x %9.2f" % (name, calls // TRACE_CALLS, mean_us))
            if "pcaf_" in name:
                total += calls // TRACE_CALLS * mean_us
            if "pcaf_filter_kernel" in name:
                nbytes = (nq + 31) // 32 * N * (tp + 1) * 4
                lines.append("    filter: %.1f MB of projected rows per launch = %.2f TB/s (%.2f of the %.2f TB/s copy ceiling)"
                             % (nbytes / 1e6, nbytes / mean_us / 1e6, nbytes / mean_us * 1e6 / COPY_CEILING, COPY_CEILING / 1e12))
        lines.append("  one-handle kernels together: %.2f us" % total)
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcaf_one_handle_vs_composition.txt"))
    ap.add_argument("--trace", type=int)
    ap.add_argument("--kernels")
    a = ap.parse_args()
    if a.trace:
        trace(a.trace)
    elif a.kernels:
        kernels(a.kernels, a.out)
    else:
        measure(a.reps, a.out)
