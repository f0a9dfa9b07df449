"""IVF-FLAT filtered search with one allow-mask per query: the batched call against what callers had before it.

The project's IVF configuration -- n x 768 rows from datagen (gaussian), n / 1024 x 1.05 ~ 1000 rows per list (1M rows: 1024
lists), nprobe 32, k 10, cosine -- or a quarter of it (--n 250000 --nlist 256: the same list length, so the same rows per probed
list).  Per (nq, selectivity), with nq DISTINCT random masks at that selectivity, on the device entry points (queries, masks and
results stay on the device; every timed window ends in a synchronise; host clock):

  (a) ivf_search_filtered_each_dev, one call;
  (b) the only way without it: a loop of nq single-query ivf_search_filtered_dev calls with the same masks;
  (c) the floor: ONE single-mask ivf_search_filtered_dev call of nq queries (mask of query 0) -- the compacted scan, which reads
      nothing for a failing position, where (a) reads 4 B of list ids and a gathered mask word for each.

One warm-up of every path (which also checks that (a) and (b) agree in ids and distance bits), then `--rounds` rounds in which the
paths alternate; median [min .. max] in ms and the ratios of the medians.  Writes profiles/ivf_filtered_each.txt.

    python tools/ivf_filtered_each_time.py [--n 1000000 --nlist 1024] [--nq 1,32,256,1024] [--sel 0.01,0.1,0.5] [--rounds 5]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def device_masks(torch, dev, nq, n, sel, seed):
    """[nq][(n + 31) / 32] int32 words on the device, every bit below n set with probability sel, a different draw per query."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    W = (n + 31) // 32
    weights = (torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, dtype=torch.int64, device=dev))
    out = torch.empty((nq, W), dtype=torch.int32, device=dev)
    for q in range(nq):
        bits = torch.zeros(W * 32, dtype=torch.int64, device=dev)
        bits[:n] = (torch.rand(n, generator=g, device=dev) < sel).to(torch.int64)
        words = (bits.view(W, 32) * weights).sum(dim=1)                  # in [0, 2^32)
        out[q] = torch.where(words >= (1 << 31), words - (1 << 32), words).to(torch.int32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", default="1,32,256,1024")
    ap.add_argument("--sel", default="0.01,0.1,0.5")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kmeans-iterations", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_filtered_each.txt"))
    args = ap.parse_args()

    import torch

    from hnsw_clj_amd import datagen, engine

    assert engine.device_count() >= 1, "no GPU: this tool measures on the device and has no other path"
    dev = torch.device("cuda", 0)
    n, dim, k, nprobe = args.n, args.dim, args.k, args.nprobe
    nqs = [int(x) for x in args.nq.split(",")]
    t0 = time.perf_counter()
    base = datagen.generate_dataset(n, dim)
    Qh = datagen.generate_dataset(max(nqs), dim, seed=43)
    print("data: %.1f s" % (time.perf_counter() - t0), flush=True)
    t0 = time.perf_counter()
    idx = engine.Index(base, "cosine", 0)
    idx.ivf_build(args.nlist, args.kmeans_iterations, 42)
    _, off, _ = idx.get_ivf()
    lens = np.diff(off)
    print("index: %.1f s" % (time.perf_counter() - t0), flush=True)
    del base
    Qd = torch.from_numpy(Qh).to(dev)
    lines = ["IVF-FLAT filtered search, one allow-mask per query: %d x %d (datagen, gaussian) cosine, %d lists (%d iterations; rows per list "
             "mean %.0f, max %d), nprobe %d, k %d" % (n, dim, args.nlist, args.kmeans_iterations, lens.mean(), lens.max(), nprobe, k),
             "device entry points, nq distinct random masks per point, host clock around enqueue + synchronise, 1 warm-up + %d alternating rounds" % args.rounds,
             "(a) ivf_search_filtered_each_dev, one call   (b) nq calls of ivf_search_filtered_dev, one query each   "
             "(c) ivf_search_filtered_dev, nq queries, ONE mask",
             "ms: median [min .. max]",
             "",
             "%5s %5s | %26s | %29s | %26s | %7s %7s" % ("nq", "sel", "(a) ms", "(b) ms", "(c) ms", "(a)/(b)", "(a)/(c)")]
    for nq in nqs:
        for sel in [float(x) for x in args.sel.split(",")]:
            masks = device_masks(torch, dev, nq, n, sel, 1000 * nq + int(sel * 100))
            Q = Qd[:nq].contiguous()
            oa = (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
            ob = (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
            oc = (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
            qs = [Q[q:q + 1] for q in range(nq)]
            outs = [(ob[0][q:q + 1], ob[1][q:q + 1]) for q in range(nq)]
            rows = [masks[q] for q in range(nq)]

            def a():
                idx.ivf_search_filtered_each_dev(Q, k, nprobe, masks, out=oa)

            def b():
                for q in range(nq):
                    idx.ivf_search_filtered_dev(qs[q], k, nprobe, rows[q], out=outs[q])

            def c():
                idx.ivf_search_filtered_dev(Q, k, nprobe, rows[0], out=oc)

            paths = [("a", a), ("b", b), ("c", c)]
            for _, fn in paths:                                         # the warm-up ...
                fn()
            torch.cuda.synchronize()
            assert torch.equal(oa[0], ob[0]) and torch.equal(oa[1].view(torch.int32), ob[1].view(torch.int32)), \
                "nq %d sel %g: the batched call and the single calls differ" % (nq, sel)   # ... and the results agree
            t = {p: [] for p, _ in paths}
            for _ in range(args.rounds):
                for p, fn in paths:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    t[p].append((time.perf_counter() - t0) * 1e3)
            cell = lambda x, w: ("%%%d.3f [%%%d.3f .. %%%d.3f]" % (w, w, w)) % (float(np.median(x)), min(x), max(x))  # noqa: E731
            ma, mb, mc = (float(np.median(t[p])) for p in "abc")
            lines.append("%5d %5.2f | %26s | %29s | %26s | %7.3f %7.3f" % (nq, sel, cell(t["a"], 7), cell(t["b"], 8), cell(t["c"], 7), ma / mb, ma / mc))
            print(lines[-1], flush=True)
            del masks, rows
    idx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
