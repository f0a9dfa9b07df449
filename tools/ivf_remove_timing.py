"""hnswgpu_ivf_remove on the headline set: what a batch of rows that leave costs a live IVF-FLAT index, at a few batch sizes, beside
the only alternative there was before: a fresh handle over the kept rows from host memory (create + set_rejection_test + set_ivf
with the same centroids and the compacted lists).

31,173 x 768 (bench.py's clustered, normalised set), cosine, 24 lists (the reference's default partition count) from
ivf_build(24, 3, 42), rejection mode 1 (the default: int8 tiles and the half copy exist at dim 768).  The host clock around calls
that end in a device synchronise; per line the median of --reps runs after one warm-up, with the range beside it.  A removal
changes its handle, so every run of one gets a fresh handle (create + set_ivf), made outside the timed window.  The rebuild is
given its compacted lists ready-made: the host pass that would compute them is NOT in its time.

Every batch size is a step of its own: a child process under its own time limit that first compares the shrunken handle with the
fresh one (get_ivf, norms, one search's bits) and then measures.  The first step that fails or runs out of time ends the run and
nothing is written.  No threshold is set: the file records what was measured.  Writes profiles/ivf_remove.txt.

    python tools/ivf_remove_timing.py [--reps 5] [--out profiles/ivf_remove.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (1, 1024, 8192)
NLIST, MODE = 24, 1
STEP_SECONDS = 240


def timed(setup, fn, reps):
    """(median, min, max) wall time in ms of fn(state) over `reps` runs after one warm-up; setup() -> state and state.close() are
    outside the window"""
    import numpy as np

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


def step(m, reps):
    """One batch size, in a process of its own: check, then measure; one JSON line on stdout."""
    import numpy as np

    import bench  # (the headline set)
    from hnsw_clj_amd import engine

    n, dim = bench.N31K, bench.DIM
    base = bench.make_31k("clustered", 42, n)
    with engine.Index(base, "cosine", 0) as b:
        b.set_rejection_test(MODE)
        b.ivf_build(NLIST, 3, 42)
        cen, off0, ids0 = b.get_ivf()
    gone = np.random.default_rng(7).choice(n, m, replace=False).astype(np.int32)
    keep = np.ones(n, np.bool_)
    keep[gone] = False
    kept_rows = np.ascontiguousarray(base[keep])
    new_id = np.full(n, -1, np.int64)                        # the compacted lists: dropped entries close up, the rest renumbered
    new_id[keep] = np.arange(keep.sum())
    stays = keep[ids0]
    off1 = off0 - np.concatenate([[0], np.cumsum(~stays)])[off0]
    ids1 = new_id[ids0][stays].astype(np.int32)

    def live():
        ix = engine.Index(base, "cosine", 0)
        ix.set_rejection_test(MODE)
        ix.set_ivf(cen, off0, ids0)
        ix.sync()
        return ix

    def fresh(_=None):
        ix = engine.Index(kept_rows, "cosine", 0)
        ix.set_rejection_test(MODE)
        ix.set_ivf(cen, off1, ids1)
        return ix

    def bare(_=None):
        ix = engine.Index(kept_rows, "cosine", 0)
        ix.sync()
        return ix

    # what is timed computes what it should: the shrunken handle against the fresh one over the kept rows
    Q = np.ascontiguousarray(base[:16])
    with live() as ix, fresh() as want:
        kept = ix.ivf_remove(gone)
        if not np.array_equal(kept, np.flatnonzero(keep)):
            raise SystemExit("ivf_remove kept other rows than the mask")
        if not all(np.array_equal(a, b) for a, b in zip(ix.get_ivf(), (cen, off1, ids1))):
            raise SystemExit("the shrunken lists differ from the compacted lists")
        if not np.array_equal(ix.norms().view(np.uint32), want.norms().view(np.uint32)):
            raise SystemExit("the shrunken handle's norms differ from the fresh one's")
        want.ivf_set_stream_state(ix.ivf_stream_state())     # (mode 1: one first-search verdict for both)
        (gi, gd), (wi, wd) = ix.ivf_search(Q, 10, 4), want.ivf_search(Q, 10, 4)
        if not (np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))):
            raise SystemExit("the shrunken handle's search differs from the fresh one's")

    def remove(ix):
        ix.ivf_remove(gone)

    out = {"m": m, "n": n, "dim": dim, "kept": int(keep.sum()),
           "remove": timed(live, remove, reps),
           "rebuild": timed(lambda: None, fresh, reps),
           "create": timed(lambda: None, bare, reps),
           "set_ivf": timed(bare, lambda ix: ix.set_ivf(cen, off1, ids1), reps)}
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_remove.txt"))
    ap.add_argument("--step", type=int, default=None, help="(internal) measure this batch size and print one JSON line")
    args = ap.parse_args()
    if args.step is not None:
        return step(args.step, args.reps)

    results = []
    for m in BATCHES:   # each GPU step in a process of its own, under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(m), "--reps", str(args.reps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired:
            raise SystemExit("step m = %d did not finish within %d s: nothing written" % (m, STEP_SECONDS))
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("step m = %d failed with exit status %d: nothing written" % (m, p.returncode))
        results.append(json.loads(line[-1][len("RESULT "):]))

    r0 = results[0]
    lines = ["hnswgpu_ivf_remove, %d x %d cosine (clustered, normalised), %d lists, rejection mode %d" % (r0["n"], r0["dim"], NLIST, MODE),
             "host clock around calls that end in a device synchronise; median of %d after a warm-up [min .. max], ms" % args.reps,
             "every removal runs on a fresh handle made outside the timed window; the shrunken handle equals the fresh handle's lists,",
             "norms and one search's bits; the rebuild is given its compacted lists ready-made (the host pass for them is not timed)",
             ""]
    fmt = "%-66s %9.3f  [%8.3f .. %8.3f]"
    for r in results:
        lines += [fmt % (("(a) ivf_remove of %d scattered rows from a handle over %d" % (r["m"], r["n"]),) + tuple(r["remove"])),
                  fmt % (("(b) Index(the %d kept rows) + set_rejection_test + set_ivf" % r["kept"],) + tuple(r["rebuild"])),
                  fmt % (("      of which Index(kept rows): upload, norms",) + tuple(r["create"])),
                  fmt % (("      of which set_ivf: lists up, permute, int8 tiles, half copy",) + tuple(r["set_ivf"])),
                  "      (a) / (b) = %.3f: %s" % (r["remove"][0] / r["rebuild"][0],
                                                  "the removal is faster" if r["remove"][0] < r["rebuild"][0] else "the removal is NOT faster than the rebuild"),
                  ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
