"""hnswgpu_lsh_update on the headline set: what a batch of rows that take new values costs a live hybrid LSH index, at a few batch
sizes, beside the two things there were before: (a) a fresh handle over the base with the new values from host memory (create +
set_lsh with the same planes: an upload of the whole base, a read-back of every code, a counting sort on the host), and
(b) hnswgpu_lsh_remove + hnswgpu_lsh_add of the same rows -- the old workaround, which LOSES the ids: the rows come back as
n - m .. n - 1 and every id above a removed one shifts.

31,173 x 768 (bench.py's clustered, normalised set), cosine, the reference's index (8 tables x 12 bits, Random(42)).  The new values
are other rows of the same set with a little noise, normalised again: in a table some keep their bucket, most move.  The host clock
around calls that end in a device synchronise; per line the median of --reps runs after one warm-up, with the range beside it.
The update, the rebuild and the pair alternate in one process.  An update changes its handle, so every run of one gets a fresh
handle (create + set_lsh), made outside the timed window.

Every batch size is a step of its own: a child process under its own time limit that first compares the updated handle with the
fresh one (lsh_get array for array, norms, one search's bits) and then measures.  The first step that fails or runs out of time
ends the run and nothing is written.  No threshold is set: the file records what was measured.

    python tools/lsh_update_timing.py [--reps 5] [--out profiles/lsh_update.txt] [--kernels DIR]

Per-kernel times come from a collection of their own, never combined with counters, one per batch size:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/m<M> -- python tools/lsh_update_timing.py --trace <M>

--trace runs --reps + 1 updates of M rows on ONE handle (the values alternate between two sets, so rows move in every call) and
nothing else after the handle is made; --kernels DIR reads the dispatch records DIR/m<M>/**/*kernel_trace.csv, drops what ran
before the first update's first kernel (the handle's creation) and the warm-up call, and appends every kernel's mean time per
call to the file.
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (1, 1024, 8192)
STEP_SECONDS = 240
FIRST_KERNEL = "lsh_update_stage_kernel"


def _setting(m):
    """The headline set, the reference's index shape, m scattered row ids and two sets of new values for them"""
    import numpy as np

    import bench  # (the headline set)
    from hnsw_clj_amd import hybrid_lsh as H

    n, dim = bench.N31K, bench.DIM
    base = bench.make_31k("clustered", 42, n)
    shape = (H.NUM_HASH_TABLES, H.NUM_HASH_BITS, H.PROJECTION_DIM, H.SEED)
    rng = np.random.default_rng(7)
    at = rng.choice(n, m, replace=False).astype(np.int32)    # scattered rows
    sets = []
    for _ in range(2):
        new = base[rng.choice(n, m)] + 0.05 * rng.standard_normal((m, dim)).astype(np.float32) / np.sqrt(dim)
        sets.append(np.ascontiguousarray(new / np.linalg.norm(new, axis=1, keepdims=True), np.float32))
    return base, shape, at, sets


def step(m, reps):
    """One batch size, in a process of its own: check, then measure; one JSON line on stdout."""
    import numpy as np

    from hnsw_clj_amd import engine

    base, shape, at, (new, _) = _setting(m)
    n, dim = base.shape
    cur = base.copy()
    cur[at] = new
    with engine.Index(base, "cosine", 0) as b:
        b.lsh_build(*shape)
        planes, codes0 = b.lsh_get()[:2]

    def live():
        ix = engine.Index(base, "cosine", 0)
        ix.set_lsh(planes)
        ix.sync()
        return ix

    def fresh(_=None):
        fx = engine.Index(cur, "cosine", 0)
        fx.set_lsh(planes)
        return fx

    # what is timed computes what it should: the updated handle against the fresh one over the base with the new values
    Q = np.ascontiguousarray(base[:16])
    with live() as ix, fresh() as want:
        ix.lsh_update(at, new)
        got = ix.lsh_get()
        if not all(np.array_equal(a, b) for a, b in zip(got, want.lsh_get())):
            raise SystemExit("the updated handle's tables differ from the fresh one's")
        if not np.array_equal(ix.norms().view(np.uint32), want.norms().view(np.uint32)):
            raise SystemExit("the updated handle's norms differ from the fresh one's")
        (gi, gd), (wi, wd) = ix.lsh_search(Q, 10), want.lsh_search(Q, 10)
        if not (np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))):
            raise SystemExit("the updated handle's search differs from the fresh one's")
        moved = got[1][at] != codes0[at]
        movers, entries = int(moved.any(axis=1).sum()), int(moved.sum())

    def clock(fn, arg):
        t0 = time.perf_counter()
        made = fn(arg)
        dt = (time.perf_counter() - t0) * 1e3
        if made is not None:
            made.close()
        return dt

    def update(ix):
        ix.lsh_update(at, new)

    def pair(ix):
        ix.lsh_remove(at)
        ix.lsh_add(new)

    t = {"update": [], "rebuild": [], "pair": []}
    for r in range(reps + 1):                                # the three alternate; run 0 is the warm-up
        ix = live()
        a = clock(update, ix)
        ix.close()
        b = clock(fresh, None)
        ix = live()
        c = clock(pair, ix)
        ix.close()
        if r:
            for k, v in zip(("update", "rebuild", "pair"), (a, b, c)):
                t[k].append(v)
    out = {"m": m, "n": n, "dim": dim, "tables": shape[0], "bits": shape[1], "movers": movers, "entries": entries}
    for k, v in t.items():
        out[k] = (float(np.median(v)), min(v), max(v))
    print("RESULT " + json.dumps(out))


def trace(m, reps):
    """What the per-kernel collection runs: one handle, reps + 1 updates of the same m rows, the values alternating"""
    from hnsw_clj_amd import engine

    base, shape, at, sets = _setting(m)
    with engine.Index(base, "cosine", 0) as ix:
        ix.lsh_build(*shape)
        ix.sync()
        for r in range(reps + 1):
            ix.lsh_update(at, sets[r % 2])
    print("TRACED %d updates of %d rows" % (reps + 1, m))


def _short(name):
    hit = re.search(r"(\w+)\s*(?:<[^()]*>)?\s*\(", name)
    return hit.group(1) if hit else name.strip()[:60]


def kernel_table(directory, m):
    """[(kernel, calls per update, mean us per update)] of the updates after the warm-up call, from the dispatch records of one
    collection; None when there are none"""
    rows = []
    for path in glob.glob(os.path.join(directory, "m%d" % m, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for rec in csv.DictReader(f):
                low = {k.lower(): v for k, v in rec.items()}
                rows.append((int(low["start_timestamp"]), int(low["end_timestamp"]), low["kernel_name"]))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if FIRST_KERNEL in r[2]]
    if len(starts) < 2:
        return None
    calls = len(starts) - 1                                  # (the first update is the warm-up)
    total, count, order = {}, {}, []
    for s, e, name in rows[starts[1]:]:
        k = _short(name)
        if k not in total:
            order.append(k)
        total[k] = total.get(k, 0) + (e - s)
        count[k] = count.get(k, 0) + 1
    return [(k, count[k] / calls, total[k] / calls / 1e3) for k in order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsh_update.txt"))
    ap.add_argument("--kernels", default=None, help="directory of the rocprofv3 collections (m<M>/ per batch size)")
    ap.add_argument("--step", type=int, default=None, help="(internal) measure this batch size and print one JSON line")
    ap.add_argument("--trace", type=int, default=None, help="run updates of this batch size and nothing else (under rocprofv3)")
    args = ap.parse_args()
    if args.step is not None:
        return step(args.step, args.reps)
    if args.trace is not None:
        return trace(args.trace, args.reps)

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
    lines = ["hnswgpu_lsh_update, %d x %d cosine (clustered, normalised), %d tables x %d bits" % (r0["n"], r0["dim"], r0["tables"], r0["bits"]),
             "host clock around calls that end in a device synchronise; median of %d after a warm-up [min .. max], ms" % args.reps,
             "the three alternate in one process; every update runs on a fresh handle made outside the timed window; the updated handle",
             "equals the fresh handle's tables, norms and one search's bits; (b) is the old workaround, after which the rows have other ids",
             ""]
    fmt = "%-92s %9.3f  [%8.3f .. %8.3f]"
    for r in results:
        lines += [fmt % (("lsh_update of %d scattered rows (%d move, %d table entries) of a handle over %d" % (r["m"], r["movers"], r["entries"], r["n"]),)
                         + tuple(r["update"])),
                  fmt % (("(a) Index(the %d rows, new values) + set_lsh(planes)" % r["n"],) + tuple(r["rebuild"])),
                  fmt % (("(b) lsh_remove + lsh_add of the same %d rows (the ids are lost)" % r["m"],) + tuple(r["pair"])),
                  "      update / (a) = %.3f: %s;  update / (b) = %.3f" % (
                      r["update"][0] / r["rebuild"][0],
                      "the update is faster" if r["update"][0] < r["rebuild"][0] else "the update is NOT faster than the rebuild",
                      r["update"][0] / r["pair"][0]),
                  ""]
    if args.kernels:
        lines += ["per kernel, from a kernel trace of its own (rocprofv3 --kernel-trace, no counters; one handle, the updates after a warm-up",
                  "call): launches per update, mean microseconds per update.  The copies of base, norms and codes and the uploads are the runtime's",
                  "(a call's uploads run before its first kernel and are counted with the call before it: hence the fractional counts).", ""]
        for m in BATCHES:
            table = kernel_table(args.kernels, m)
            if table is None:
                lines += ["m = %d: no dispatch records found" % m, ""]
                continue
            lines.append("m = %d" % m)
            lines += ["    %-44s %6.2f x %10.2f us" % row for row in table]
            lines += ["    %-44s %6s   %10.2f us" % ("sum of the kernels", "", sum(r[2] for r in table)), ""]
    else:
        lines += ["no per-kernel trace was taken", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
