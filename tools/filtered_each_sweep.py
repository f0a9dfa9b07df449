"""One allow-mask per query on the headline set: the batched call against what callers did before it.

31,173 x 768 (bench.py's clustered set), cosine, k = 10, batches of 32 / 256 / 1024 queries.  Mask families: `same` (one mask,
10 % of the rows), 4 and 64 tenants (the rows dealt to tenants at random, the queries dealt to tenants in turn -- a caller that
does NOT sort its batch -- and the same batch sorted by tenant, as ultra_fast.search_batch_filtered_each orders it), one disjoint
mask per query (query q: rows q, q + nq, ...), 1 % random per query.  Per point, the host entry points (masks and queries from
host memory, results back: every call ends in a synchronise), timed with the host clock, one warm-up, then five rounds in which
the compared paths alternate; median, min and max:

  (a) exact_knn_filtered_each, one call;
  (b) a loop of nq single-query exact_knn_filtered calls;
  (c) `same` only: exact_knn_filtered on the whole batch.

Writes profiles/filtered_each.txt.

    python tools/filtered_each_sweep.py [--nq 32,256,1024] [--rounds 5] [--out profiles/filtered_each.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402  (the headline set)


def families(n, nq, rng):
    """name -> [nq][n] bool"""
    out = {}
    out["same"] = np.repeat((rng.random(n) < 0.1)[None, :], nq, axis=0)
    for t in (4, 64):
        owner = rng.integers(0, t, n)
        dealt = np.stack([owner == (q % t) for q in range(nq)])
        out["%d tenants, dealt" % t] = dealt
        out["%d tenants, sorted" % t] = dealt[np.argsort(np.arange(nq) % t, kind="stable")]
    disjoint = np.zeros((nq, n), np.bool_)
    for q in range(nq):
        disjoint[q, q::nq] = True
    out["disjoint"] = disjoint
    out["1 % random"] = rng.random((nq, n)) < 0.01
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", default="32,256,1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_each.txt"))
    args = ap.parse_args()

    from hnsw_clj_amd import engine

    n, dim, k = bench.N31K, bench.DIM, bench.K
    base = bench.make_31k("clustered", 42, n)
    idx = engine.Index(base, "cosine", 0)
    lines = ["one allow-mask per query, %d x %d cosine, k = %d; host entry points, host clock, 1 warm-up + %d alternating rounds" % (n, dim, k, args.rounds),
             "(a) exact_knn_filtered_each   (b) nq calls of exact_knn_filtered, one query each   (c) exact_knn_filtered, the whole batch",
             "ms: median [min .. max]",
             "",
             "%5s %-20s %9s | %26s | %26s | %26s | %7s %7s" % ("nq", "family", "rows/q", "(a) ms", "(b) ms", "(c) ms", "(a)/(b)", "(a)/(c)")]
    for nq in [int(x) for x in args.nq.split(",")]:
        Q = bench.make_31k("clustered", 43, nq)
        for name, bits in families(n, nq, np.random.default_rng(nq)).items():
            masks = engine.pack_masks(bits, n)
            paths = [("a", lambda: idx.exact_knn_filtered_each(Q, k, masks)),
                     ("b", lambda: [idx.exact_knn_filtered(Q[q:q + 1], k, masks[q]) for q in range(nq)])]
            if name == "same":
                paths.append(("c", lambda: idx.exact_knn_filtered(Q, k, masks[0])))
            got = {p: fn() for p, fn in paths}                      # the warm-up, and the results agree
            bi = np.concatenate([r[0] for r in got["b"]])
            bd = np.concatenate([r[1] for r in got["b"]])
            assert np.array_equal(got["a"][0], bi) and np.array_equal(got["a"][1].view(np.uint32), bd.view(np.uint32)), name
            if "c" in got:
                assert np.array_equal(got["a"][0], got["c"][0]) and np.array_equal(got["a"][1].view(np.uint32), got["c"][1].view(np.uint32))
            t = {p: [] for p, _ in paths}
            for _ in range(args.rounds):
                for p, fn in paths:
                    t0 = time.perf_counter()
                    fn()
                    t[p].append((time.perf_counter() - t0) * 1e3)
            cell = lambda x: "%8.3f [%7.3f .. %7.3f]" % (float(np.median(x)), min(x), max(x))  # noqa: E731
            ma, mb = float(np.median(t["a"])), float(np.median(t["b"]))
            lines.append("%5d %-20s %9.0f | %26s | %26s | %26s | %7.3f %7s"
                         % (nq, name, bits.sum(axis=1).mean(), cell(t["a"]), cell(t["b"]), cell(t["c"]) if "c" in t else "-", ma / mb,
                            "%.3f" % (ma / float(np.median(t["c"]))) if "c" in t else "-"))
            print(lines[-1], flush=True)
    idx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
