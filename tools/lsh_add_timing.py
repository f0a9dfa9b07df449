"""hnswgpu_lsh_add on the headline set: what a batch of rows costs a live hybrid LSH index, beside the only alternative there was
before (create over all rows + install the planes), and an add of every row into an empty handle beside a build.

31,173 x 768 (bench.py's clustered, normalised set), cosine, the reference's index (8 tables x 12 bits, Random(42)).  The host clock
around calls that end in a device synchronise (every call timed here waits for its stream before it returns); per line the
median of --reps runs after one warm-up, with the range beside it.  An add changes its handle, so every run of an add gets a
fresh handle, made outside the timed window.
  (a) lsh_add of the last 1,024 rows into a handle over the first 30,149
  (b) Index(all 31,173 rows) + set_lsh(planes), and its two halves
  (c) lsh_add of all 31,173 rows into an empty handle with tables, beside lsh_build on a handle over all rows; the add uploads the
      rows and computes their norms, which the build's handle did in its create -- that is (b)'s first half
Every grown handle's tables are compared with the fresh handle's before anything is written.  Writes profiles/lsh_add.txt.

    python tools/lsh_add_timing.py [--reps 5] [--out profiles/lsh_add.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402  (the headline set)

BATCH = 1024


def timed(setup, fn, reps):
    """(median, min, max) wall time in ms of fn(state) over `reps` runs after one warm-up; setup() -> state and state.close() are
    outside the window"""
    t = []
    for r in range(reps + 1):
        state = setup()
        t0 = time.perf_counter()
        made = fn(state)
        dt = (time.perf_counter() - t0) * 1e3
        for h in (state, made):
            if h is not None:
                h.close()
        if r:
            t.append(dt)
    return float(np.median(t)), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsh_add.txt"))
    args = ap.parse_args()

    from hnsw_clj_amd import engine
    from hnsw_clj_amd import hybrid_lsh as H

    n, dim = bench.N31K, bench.DIM
    base = bench.make_31k("clustered", 42, n)
    n0 = n - BATCH
    shape = (H.NUM_HASH_TABLES, H.NUM_HASH_BITS, H.PROJECTION_DIM, H.SEED)

    def with_tables(rows):
        ix = engine.Index(rows, "cosine", 0)
        ix.lsh_build(*shape)
        ix.sync()
        return ix

    def bare(rows):
        ix = engine.Index(rows, "cosine", 0)
        ix.sync()
        return ix

    def fresh(planes):
        ix = engine.Index(base, "cosine", 0)
        ix.set_lsh(planes)
        return ix

    # what is timed computes what it should: both grown handles against the fresh one
    with with_tables(base) as full:
        want = full.lsh_get()
    planes = want[0]
    for first in (n0, 0):
        with with_tables(base[:first]) as ix:
            ix.lsh_add(base[first:])
            if not all(np.array_equal(a, b) for a, b in zip(ix.lsh_get(), want)):
                raise SystemExit("the handle grown from %d rows differs from the fresh one" % first)

    def add(new):
        def run(ix):
            ix.lsh_add(new)
        return run

    rows = [
        ("(a) lsh_add of %d rows into a handle over %d" % (BATCH, n0), timed(lambda: with_tables(base[:n0]), add(base[n0:]), args.reps)),
        ("(b) Index(all %d rows) + set_lsh(planes)" % n, timed(lambda: None, lambda _: fresh(planes), args.reps)),
        ("      of which Index(all rows): upload, norms", timed(lambda: None, lambda _: bare(base), args.reps)),
        ("      of which set_lsh: hash, codes back, host sort, ids up", timed(lambda: bare(base), lambda ix: ix.set_lsh(planes), args.reps)),
        ("(c) lsh_add of all %d rows into an empty handle with tables" % n,
         timed(lambda: with_tables(base[:0]), add(base), args.reps)),
        ("    lsh_build on a handle over all rows", timed(lambda: bare(base), lambda ix: ix.lsh_build(*shape), args.reps)),
    ]
    lines = ["hnswgpu_lsh_add, %d x %d cosine (clustered, normalised), %d tables x %d bits" % (n, dim, shape[0], shape[1]),
             "host clock around calls that end in a device synchronise; median of %d after a warm-up [min .. max], ms" % args.reps,
             "every add runs on a fresh handle made outside the timed window; the grown tables equal the fresh handle's",
             ""]
    for label, (med, lo, hi) in rows:
        lines.append("%-62s %9.3f  [%8.3f .. %8.3f]" % (label, med, lo, hi))
    a, b, up, sort, c, build = (rows[i][1][0] for i in range(6))
    lines += ["",
              "(a) / (b) = %.3f: a batch of %d rows costs %.2f ms where the rebuild costs %.2f ms" % (a / b, BATCH, a, b),
              "(c): the add of every row takes %.2f ms, the build %.2f ms on a handle whose rows are already on the device." % (c, build),
              "     Of the build, %.2f ms draw the planes on the host (lsh_build - set_lsh); of the add, %.2f ms are the upload and the"
              % (build - sort, up),
              "     norms ((b)'s first half).  Hash + buckets alone: add - upload = %.2f ms by the device placement, %.2f ms by set_lsh's"
              % (c - up, sort),
              "     read-back and host sort: %.2f x" % ((c - up) / sort)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
