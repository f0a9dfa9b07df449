"""hnswgpu_ivf_update on the headline set: what a batch of rows that take new values costs a live IVF-FLAT index, at a few batch
sizes, beside the two alternatives there were before: a fresh handle over the base with the new values from host memory (create +
set_rejection_test + set_ivf with the same centroids and the updated lists), and hnswgpu_ivf_remove + hnswgpu_ivf_add of the same
rows -- the old workaround, which LOSES the ids: the rows come back as n - m .. n - 1 and every id above a removed one shifts.

31,173 x 768 (bench.py's clustered, normalised set), cosine, 24 lists (the reference's default partition count) from
ivf_build(24, 3, 42), rejection mode 1 (the default: int8 tiles and the half copy exist at dim 768).  The new values are other rows
of the same set with a little noise, normalised again: some stay in their list, some move.  The host clock around calls that end in
a device synchronise; per line the median of --reps runs after one warm-up, with the range beside it.  The update and the rebuild
alternate in one process.  An update changes its handle, so every run of one gets a fresh handle (create + set_ivf), made outside
the timed window.  The rebuild is given its lists ready-made: the host pass that would compute them is NOT in its time.  The
kernels' share of a call is the library's own profile counter (hnswgpu_get_profile, slot 3: device time from the first launch of
the chain to the last), from runs of their own with profiling on.

Every batch size is a step of its own: a child process under its own time limit that first compares the updated handle with the
fresh one (get_ivf, norms, one search's bits) and then measures.  The first step that fails or runs out of time ends the run and
nothing is written.  No threshold is set: the file records what was measured.  Writes profiles/ivf_update.txt.

    python tools/ivf_update_timing.py [--reps 5] [--out profiles/ivf_update.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCHES = (1, 1024, 8192)
NLIST, MODE = 24, 1
STEP_SECONDS = 240


def step(m, reps):
    """One batch size, in a process of its own: check, then measure; one JSON line on stdout."""
    import numpy as np

    import bench  # (the headline set)
    from hnsw_clj_amd import engine
    from ivf_update_model import updated_lists

    n, dim = bench.N31K, bench.DIM
    base = bench.make_31k("clustered", 42, n)
    with engine.Index(base, "cosine", 0) as b:
        b.set_rejection_test(MODE)
        b.ivf_build(NLIST, 3, 42)
        cen, off0, ids0 = b.get_ivf()
    rng = np.random.default_rng(7)
    at = rng.choice(n, m, replace=False).astype(np.int32)    # scattered rows
    new = base[rng.choice(n, m)] + 0.05 * rng.standard_normal((m, dim)).astype(np.float32) / np.sqrt(dim)
    new = np.ascontiguousarray(new / np.linalg.norm(new, axis=1, keepdims=True), np.float32)
    cur = base.copy()
    cur[at] = new

    def live():
        ix = engine.Index(base, "cosine", 0)
        ix.set_rejection_test(MODE)
        ix.set_ivf(cen, off0, ids0)
        ix.sync()
        return ix

    # the lists the rule gives: the updated handle's own (the assignment is the device's), checked against the model
    with live() as ix:
        ix.ivf_update(at, new)
        _, off1, ids1 = ix.get_ivf()
        where = np.empty(n, np.int64)
        where[ids1] = np.repeat(np.arange(NLIST), np.diff(off1))
        was = np.empty(n, np.int64)
        was[ids0] = np.repeat(np.arange(NLIST), np.diff(off0))
        movers = int((where[at] != was[at]).sum())
        mo, mi = updated_lists(off0, ids0, at, where[at])
        if not (np.array_equal(mo, off1) and np.array_equal(mi, ids1)):
            raise SystemExit("the updated lists differ from the model's")

        def fresh(_=None):
            fx = engine.Index(cur, "cosine", 0)
            fx.set_rejection_test(MODE)
            fx.set_ivf(cen, off1, ids1)
            return fx

        # what is timed computes what it should: the updated handle against the fresh one over the base with the new values
        Q = np.ascontiguousarray(base[:16])
        with fresh() as want:
            if not np.array_equal(ix.norms().view(np.uint32), want.norms().view(np.uint32)):
                raise SystemExit("the updated handle's norms differ from the fresh one's")
            want.ivf_set_stream_state(ix.ivf_stream_state())     # (mode 1: one first-search verdict for both)
            (gi, gd), (wi, wd) = ix.ivf_search(Q, 10, 4), want.ivf_search(Q, 10, 4)
            if not (np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))):
                raise SystemExit("the updated handle's search differs from the fresh one's")

    def clock(fn, arg):
        t0 = time.perf_counter()
        made = fn(arg)
        dt = (time.perf_counter() - t0) * 1e3
        if made is not None:
            made.close()
        return dt

    def update(ix):
        ix.ivf_update(at, new)

    def pair(ix):
        ix.ivf_remove(at)
        ix.ivf_add(new)

    t = {"update": [], "rebuild": [], "pair": [], "device": []}
    for r in range(reps + 1):                                # the update and the rebuild alternate; run 0 is the warm-up
        ix = live()
        a = clock(update, ix)
        ix.close()
        b = clock(fresh, None)
        ix = live()
        c = clock(pair, ix)
        ix.close()
        ix = live()                                          # the kernels' share: a run of its own with the profile counter on
        ix.set_profiling(True)
        ix.get_profile(engine.PROF_UPDATE)
        ix.ivf_update(at, new)
        ms, cnt = ix.get_profile(engine.PROF_UPDATE)
        ix.close()
        if cnt != 1:
            raise SystemExit("the profile counter saw %d update chains, not 1" % cnt)
        if r:
            for k, v in zip(("update", "rebuild", "pair", "device"), (a, b, c, ms)):
                t[k].append(v)
    out = {"m": m, "n": n, "dim": dim, "movers": movers}
    for k, v in t.items():
        out[k] = (float(np.median(v)), min(v), max(v))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_update.txt"))
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
    lines = ["hnswgpu_ivf_update, %d x %d cosine (clustered, normalised), %d lists, rejection mode %d" % (r0["n"], r0["dim"], NLIST, MODE),
             "host clock around calls that end in a device synchronise; median of %d after a warm-up [min .. max], ms" % args.reps,
             "(a) and (b) alternate in one process; every update runs on a fresh handle made outside the timed window; the updated handle",
             "equals the model's lists and the fresh handle's norms and one search's bits; the rebuild is given its lists ready-made",
             "(the host pass for them is not timed); (c) is the old workaround, after which the rows have other ids",
             ""]
    fmt = "%-72s %9.3f  [%8.3f .. %8.3f]"
    for r in results:
        lines += [fmt % (("(a) ivf_update of %d scattered rows (%d move) of a handle over %d" % (r["m"], r["movers"], r["n"]),) + tuple(r["update"])),
                  fmt % (("      of which on the device, first launch to last (profile counter)",) + tuple(r["device"])),
                  fmt % (("(b) Index(the %d rows, new values) + set_rejection_test + set_ivf" % r["n"],) + tuple(r["rebuild"])),
                  fmt % (("(c) ivf_remove + ivf_add of the same %d rows (the ids are lost)" % r["m"],) + tuple(r["pair"])),
                  "      (a) / (b) = %.3f: %s;  (a) / (c) = %.3f" % (
                      r["update"][0] / r["rebuild"][0],
                      "the update is faster" if r["update"][0] < r["rebuild"][0] else "the update is NOT faster than the rebuild",
                      r["update"][0] / r["pair"][0]),
                  ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
