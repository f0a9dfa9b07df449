"""The hybrid LSH index on the headline set: build time, bucket sizes, and per mode time / QPS / recall, beside the graph traversal
at the nearest recall.

31,173 x 768 (bench.py's clustered, normalised set), cosine, k = 10, the reference's index (8 tables x 12 bits, Random(42)).  Per
mode (hybrid_lsh.clj:350-364) and batch size: the host clock around hnswgpu_lsh_search_dev + a synchronise, the median of --reps
runs after a warm-up; recall@10 against hnswgpu_exact_knn; and, measured the same way in the same run, hnswgpu_hnsw_search_dev at
the ef (of --efs) whose recall on the same queries is nearest.  The share of probed rows that sit in buckets of more than 1,000
rows says how much of the bucket scan is one wave walking a long bucket.  Two query sets of bench.py: 'clustered' from seed 43
(generated like the base but around other cluster centres: every base row is far from them) and 'clustered_same_mixture'
(held-out rows of the base's own mixture: queries that have near neighbours).  Writes profiles/hybrid_lsh.txt.

    python tools/lsh_sweep.py [--reps 5] [--out profiles/hybrid_lsh.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (the headline set and its graph builder)

BATCHES = [1, 32, 1024, 10000]
LONG_BUCKET = 1000


def timed(fn, reps):
    """Median wall time in ms of fn() + synchronise, after one warm-up"""
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def recall(ids, exact):
    return float(np.mean([len(set(a[a >= 0].tolist()) & set(b.tolist())) / exact.shape[1] for a, b in zip(ids, exact)]))


def sweep(args, idx, H, Qh, sizes, efs, k, dev, lines):
    Q = torch.from_numpy(Qh).to(dev)
    exact = idx.exact_knn_dev(Q, k)[0].cpu().numpy()
    qcodes = idx.lsh_hash(Qh).astype(np.int64)
    hnsw_recall = {ef: recall(idx.hnsw_search_dev(Q, k, ef)[0].cpu().numpy(), exact) for ef in efs}
    lines.append("%-9s %6s %7s | %9s %11s %7s | %5s %7s %9s %11s | %9s %9s" % ("mode", "probes", "batch", "ms", "QPS", "recall", "ef", "recall", "hnsw ms", "hnsw QPS", "results", "long rows"))
    for mode, (probes, radius) in H.MODE_CONFIGS.items():
        ids = idx.lsh_search(Q, k, probes, radius, 2 * k, k)[0].cpu().numpy()
        rec = recall(ids, exact)
        found = float((ids >= 0).sum()) / len(ids)
        ef = min(efs, key=lambda e: abs(hnsw_recall[e] - rec))
        probed = np.concatenate([sizes[t][qcodes[:, t] ^ (0 if j == 0 else 1 << (j - 1))] for t in range(probes) for j in range(1 + radius)])
        long_share = float(probed[probed > LONG_BUCKET].sum()) / max(float(probed.sum()), 1.0)
        for nq in BATCHES:
            Qb = Q[:nq].contiguous()
            out = (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
            ms = timed(lambda: idx.lsh_search(Qb, k, probes, radius, 2 * k, k, out=out), args.reps)
            hms = timed(lambda: idx.hnsw_search_dev(Qb, k, ef, out=out), args.reps)
            lines.append("%-9s %3dx%-2d %7d | %9.3f %11.0f %7.4f | %5d %7.4f %9.3f %11.0f | %9.2f %8.1f%%"
                         % (mode, probes, 1 + radius, nq, ms, nq / ms * 1e3, rec, ef, hnsw_recall[ef], hms, nq / hms * 1e3, found, 100 * long_share))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--efs", default="10,12,16,20,24,32,48,64,100,200")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybrid_lsh.txt"))
    args = ap.parse_args()

    from hnsw_clj_amd import engine
    from hnsw_clj_amd import hybrid_lsh as H

    dev = torch.device("cuda", 0)
    n, dim, k = bench.N31K, bench.DIM, bench.K
    base = bench.make_31k("clustered", 42, n)
    Qh = bench.make_31k("clustered", 43, max(BATCHES))
    idx = engine.Index(base, "cosine", 0)
    t_build = timed(lambda: idx.lsh_build(H.NUM_HASH_TABLES, H.NUM_HASH_BITS, H.PROJECTION_DIM, H.SEED), args.reps)
    _, _, off, _ = idx.lsh_get()
    sizes = np.diff(off, axis=1)
    filled = sizes[sizes > 0]
    lines = ["hybrid LSH, %d x %d cosine (clustered, normalised), %d tables x %d bits, k = %d" % (n, dim, H.NUM_HASH_TABLES, H.NUM_HASH_BITS, k),
             "host clock around the call + synchronise, median of %d after a warm-up" % args.reps,
             "",
             "build (planes, hash, counting sort on the host, upload): %.1f ms" % t_build,
             "buckets per table %d, non-empty %.0f on average; rows per bucket: mean %.2f, mean of the non-empty %.2f, max %d"
             % (sizes.shape[1], (sizes > 0).sum() / sizes.shape[0], sizes.mean(), filled.mean(), sizes.max()),
             "bucket sizes, percentiles of the non-empty (50 / 90 / 99 / 99.9): %s" % " / ".join("%d" % v for v in np.percentile(filled, [50, 90, 99, 99.9])),
             ""]
    idx.hnsw_build(bench.M, bench.EFC, 42, **bench.BUILDERS["heuristic"])
    efs = [int(e) for e in args.efs.split(",")]
    held_out = bench.make_31k("clustered_same_mixture", 43, max(BATCHES))
    for label, Qh in (("queries: 'clustered', seed 43 (other cluster centres than the base: every row is far)", Qh),
                      ("queries: 'clustered_same_mixture' (held-out rows of the base's own mixture)", held_out)):
        lines += ["", label]
        sweep(args, idx, H, Qh, sizes, efs, k, dev, lines)
    lines += ["",
              "probes: tables x buckets per table; recall / results / long rows: over the %d queries of a set; results: mean rows returned of k = %d;" % (max(BATCHES), k),
              "long rows: share of the probed rows that sit in buckets of more than %d rows (one wave walks a bucket)" % LONG_BUCKET,
              "hnsw: graph M = %d, efc = %d (bench.py's builder), at the ef of {%s} with the nearest recall on the same queries" % (bench.M, bench.EFC, args.efs)]
    idx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
