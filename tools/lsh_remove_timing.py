"""hnswgpu_lsh_remove on the headline set: what a batch of rows that leave costs a live hybrid LSH index, beside the only alternative
there was before (create over the kept rows + install the planes), and the fixed cost of a call (one row).

31,173 x 768 (bench.py's clustered, normalised set), cosine, the reference's index (8 tables x 12 bits, Random(42)).  The host clock
around calls that end in a device synchronise (every call timed here waits for its stream before it returns); per line the
median of --reps runs after one warm-up, with the range beside it.  A removal changes its handle, so every run of one gets a
fresh handle, made outside the timed window.
  (a) lsh_remove of 1,024 scattered rows from a handle over all 31,173
  (b) Index(the 30,149 kept rows) + set_lsh(planes), and its two halves
  (c) lsh_remove of a single row: the fixed cost of a call
The shrunken handle's tables are compared with the fresh handle's before anything is written.  Writes profiles/lsh_remove.txt.

    python tools/lsh_remove_timing.py [--reps 5] [--out profiles/lsh_remove.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsh_remove.txt"))
    args = ap.parse_args()

    from hnsw_clj_amd import engine
    from hnsw_clj_amd import hybrid_lsh as H

    n, dim = bench.N31K, bench.DIM
    base = bench.make_31k("clustered", 42, n)
    shape = (H.NUM_HASH_TABLES, H.NUM_HASH_BITS, H.PROJECTION_DIM, H.SEED)
    gone = np.sort(np.random.default_rng(7).choice(n, BATCH, replace=False)).astype(np.int32)
    keep = np.ones(n, np.bool_)
    keep[gone] = False
    kept_rows = np.ascontiguousarray(base[keep])

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
        ix = engine.Index(kept_rows, "cosine", 0)
        ix.set_lsh(planes)
        return ix

    # what is timed computes what it should: the shrunken handle against the fresh one over the kept rows
    with with_tables(base) as ix:
        planes = ix.lsh_get()[0]
        kept = ix.lsh_remove(gone)
        if not np.array_equal(kept, np.flatnonzero(keep)):
            raise SystemExit("lsh_remove kept other rows than the mask")
        with fresh(planes) as want:
            if not all(np.array_equal(a, b) for a, b in zip(ix.lsh_get(), want.lsh_get())):
                raise SystemExit("the shrunken handle differs from the fresh one over the kept rows")
            if not np.array_equal(ix.norms().view(np.uint32), want.norms().view(np.uint32)):
                raise SystemExit("the shrunken handle's norms differ from the fresh one's")

    def remove(rows):
        def run(ix):
            ix.lsh_remove(rows)
        return run

    rows = [
        ("(a) lsh_remove of %d scattered rows from a handle over %d" % (BATCH, n), timed(lambda: with_tables(base), remove(gone), args.reps)),
        ("(b) Index(the %d kept rows) + set_lsh(planes)" % len(kept_rows), timed(lambda: None, lambda _: fresh(planes), args.reps)),
        ("      of which Index(kept rows): upload, norms", timed(lambda: None, lambda _: bare(kept_rows), args.reps)),
        ("      of which set_lsh: hash, codes back, host sort, ids up", timed(lambda: bare(kept_rows), lambda ix: ix.set_lsh(planes), args.reps)),
        ("(c) lsh_remove of one row (the fixed cost of a call)", timed(lambda: with_tables(base), remove(gone[BATCH // 2:BATCH // 2 + 1]), args.reps)),
    ]
    lines = ["hnswgpu_lsh_remove, %d x %d cosine (clustered, normalised), %d tables x %d bits" % (n, dim, shape[0], shape[1]),
             "host clock around calls that end in a device synchronise; median of %d after a warm-up [min .. max], ms" % args.reps,
             "every removal runs on a fresh handle made outside the timed window; the shrunken tables equal the fresh handle's",
             ""]
    for label, (med, lo, hi) in rows:
        lines.append("%-62s %9.3f  [%8.3f .. %8.3f]" % (label, med, lo, hi))
    a, b, up, sort, c = (rows[i][1][0] for i in range(5))
    lines += ["",
              "(a) / (b) = %.3f: %d rows leave in %.2f ms where the rebuild over the kept rows costs %.2f ms" % (a / b, BATCH, a, b),
              "(c) / (a) = %.3f: a call costs %.2f ms whatever it removes -- the kept rows, codes and bucket ids are copied once per call"
              % (c / a, c)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
