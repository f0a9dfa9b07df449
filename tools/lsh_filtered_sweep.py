"""The allow-mask through the hybrid LSH bucket scan: time, rows returned and recall by pass fraction, beside post-filtering.

One handle: --n x 128 rows of datagen's clustered set (256 centres, noise 0.3, L2-normalised), cosine, the reference's index
(8 tables x 12 bits, Random(42)), mode :balanced (6 tables x 3 buckets, takes 2 k / k), k = 10; 1024 held-out rows of the same
mixture as queries.  Per batch size (1 and 1024): the host clock around the _dev entry + a synchronise, the median of --reps runs
after a warm-up, for hnswgpu_lsh_search, hnswgpu_lsh_search_filtered at pass fractions 1.0 / 0.5 / 0.1 / 0.01 and
hnswgpu_lsh_search_filtered_each with 8 distinct masks at 0.1 (equal masks adjacent).  Per fraction, over the 1024 queries: the
mean number of rows returned and recall@10 against hnswgpu_exact_knn_filtered, for the filtered call and for post-filtering a 3 k
unfiltered search (protocol.default_filtered_search's rule).

--unfiltered-only times hnswgpu_lsh_search alone and writes one JSON line: run from a checkout without the filtered entry points,
its output is this run's --baseline (the same search on the same data by an older library).

    python tools/lsh_filtered_sweep.py [--reps 20] [--baseline FILE] [--out profiles/lsh_filtered_search.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DIM, K, NQ = 128, 10, 1024
BATCHES = [1, 1024]
FRACTIONS = [1.0, 0.5, 0.1, 0.01]
EACH_MASKS, EACH_FRACTION = 8, 0.1


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
    """Mean share of the exact answer's rows (fewer than k where fewer pass) that were returned"""
    r = [len(set(a[a >= 0].tolist()) & set(b[b >= 0].tolist())) / max(int((b >= 0).sum()), 1) for a, b in zip(ids, exact) if (b >= 0).any()]
    return float(np.mean(r)) if r else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--unfiltered-only", action="store_true")
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsh_filtered_search.txt"))
    args = ap.parse_args()

    from hnsw_clj_amd import datagen, engine
    from hnsw_clj_amd import hybrid_lsh as H

    dev = torch.device("cuda", 0)
    n, k = args.n, K
    x = datagen.generate_dataset(n + NQ, DIM, "clustered", num_clusters=256, noise_level=0.3, seed=42, dtype=np.float64)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    base, Qh = x[:n].astype(np.float32), x[n:].astype(np.float32)
    probes, radius = H.mode_config("balanced")
    idx = engine.Index(base, "cosine", 0)
    idx.lsh_build(H.NUM_HASH_TABLES, H.NUM_HASH_BITS, H.PROJECTION_DIM, H.SEED)
    Q = torch.from_numpy(Qh).to(dev)

    def outs(nq):
        return (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))

    unfiltered = {}
    for nq in BATCHES:
        Qb, out = Q[:nq].contiguous(), outs(nq)
        unfiltered[nq] = timed(lambda: idx.lsh_search(Qb, k, probes, radius, 2 * k, k, out=out), args.reps)
    if args.unfiltered_only:
        line = json.dumps({"n": n, "reps": args.reps, "unfiltered_ms": {str(b): unfiltered[b] for b in BATCHES}})
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        idx.close()
        return

    baseline = json.load(open(args.baseline)) if args.baseline else None
    _, _, off, _ = idx.lsh_get()
    sizes = np.diff(off, axis=1)
    filled = sizes[sizes > 0]
    rng = np.random.default_rng(1)
    u = rng.random(n)
    lines = ["hybrid LSH filtered search, %d x %d cosine (clustered, normalised), %d tables x %d bits, mode balanced (%d x %d), k = %d"
             % (n, DIM, H.NUM_HASH_TABLES, H.NUM_HASH_BITS, probes, 1 + radius, k),
             "host clock around the _dev entry + synchronise, median of %d after a warm-up; rows / recall over %d held-out queries" % (args.reps, NQ),
             "rows per bucket: mean of the non-empty %.1f, percentiles (50 / 90 / 99): %s, max %d"
             % (filled.mean(), " / ".join("%d" % v for v in np.percentile(filled, [50, 90, 99])), sizes.max()),
             "",
             "%-28s %6s | %9s %8s | %8s %7s | %10s %9s" % ("call", "batch", "ms", "x unfilt", "rows", "recall", "post rows", "post rec")]
    wide = idx.lsh_search(Q, 3 * k, probes, radius, 6 * k, 3 * k)[0].cpu().numpy()   # what post-filtering starts from
    for nq in BATCHES:
        if baseline:
            b = baseline["unfiltered_ms"][str(nq)]
            lines.append("%-28s %6d | %9.3f %8.2f |" % ("lsh_search, parent commit", nq, b, b / unfiltered[nq]))
        lines.append("%-28s %6d | %9.3f %8.2f |" % ("lsh_search", nq, unfiltered[nq], 1.0))
        Qb, out = Q[:nq].contiguous(), outs(nq)
        for p in FRACTIONS:
            allow = u < p
            words = torch.from_numpy(engine.pack_mask(allow, n).view(np.int32)).to(dev)
            ms = timed(lambda: idx.lsh_search_filtered(Qb, k, words, probes, radius, 2 * k, k, out=out), args.reps)
            ids = idx.lsh_search_filtered(Q, k, words, probes, radius, 2 * k, k)[0].cpu().numpy()
            assert allow[ids[ids >= 0]].all()
            exact = idx.exact_knn_filtered_dev(Q, k, words)[0].cpu().numpy()
            post = np.full_like(ids, -1)
            for q in range(NQ):
                keep = [r for r in wide[q] if r >= 0 and allow[r]][:k]
                post[q, :len(keep)] = keep
            lines.append("%-28s %6d | %9.3f %8.2f | %8.2f %7.4f | %10.2f %9.4f"
                         % ("lsh_search_filtered p=%.2f" % p, nq, ms, ms / unfiltered[nq], (ids >= 0).sum() / NQ, recall(ids, exact),
                            (post >= 0).sum() / NQ, recall(post, exact)))
        masks = [rng.random(n) < EACH_FRACTION for _ in range(EACH_MASKS)]
        which = [q * EACH_MASKS // nq for q in range(nq)]   # equal masks adjacent
        packed = [engine.pack_mask(m, n) for m in masks]
        words = torch.from_numpy(np.stack([packed[w] for w in which]).view(np.int32)).to(dev)
        ms = timed(lambda: idx.lsh_search_filtered_each(Qb, k, words, probes, radius, 2 * k, k, out=out), args.reps)
        ids = out[0].cpu().numpy()
        assert all(masks[w][r[r >= 0]].all() for w, r in zip(which, ids))
        lines.append("%-28s %6d | %9.3f %8.2f | %8.2f" % ("_each, %d masks p=%.2f" % (min(EACH_MASKS, nq), EACH_FRACTION), nq, ms,
                                                         ms / unfiltered[nq], (ids >= 0).sum() / nq))
        lines.append("")
    lines += ["x unfilt: time over this library's hnswgpu_lsh_search at the same batch; rows: mean rows returned of k = %d;" % k,
              "recall: share of hnswgpu_exact_knn_filtered's rows returned; post: a 3 k unfiltered search (takes 6 k / 3 k), failing rows dropped, k kept"]
    idx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
