"""hnswgpu_hnsw_update on the headline set: what a batch of rows that take new values costs a live HNSW index, at a few batch sizes,
beside the two alternatives there were before -- (a) a fresh handle over the new base from host memory, built again (create +
set_rejection_test + hnsw_build with the same builder), and (b) hnsw_remove + hnsw_add of the same rows, which hands them new ids
and new levels -- and what the graph is worth afterwards: recall@10 after 10 % and 40 % of the rows took new values, for the
updated graph, a fresh build over the same new base and the remove + add graph.

31,173 x 768 (bench.py's clustered, normalised set), cosine, the heuristic builder with M 16 and ef_construction 200, rejection
mode 1 (the default: int8 rows exist at dim 768).  The new values are rows of OTHER clusters (bench.py's generator under another
seed: other centres than the base's).  Times: the host clock around calls that end in a device synchronise (an update is host and
device work: it ends behind its last upload); per line the median of --reps runs after one warm-up, with the range beside it.
An update changes its handle, so every run of one gets a freshly built handle, made outside the timed window.  Recall: bench.py's
1,000 held-out queries (the seed-43 stream) at ef 640 and ef 100, against the exact neighbours in the new base (exact_knn).

Every batch size and every share is a step of its own: a child process under its own time limit that first checks what it
measures (n, ids and levels unchanged, the rows' new values in place, every edge inside [0, n)) and then measures.  The first step
that fails or runs out of time ends the run and nothing is written.  No threshold is set: the file records what was measured.
Writes profiles/hnsw_update.txt.

    python tools/hnsw_update_timing.py [--reps 5] [--out profiles/hnsw_update.txt]
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
SHARES = (10, 40)                # per cent of the rows updated for the recall lines
M, EFC, SEED, MODE, EFS, NQ = 16, 200, 42, 1, (640, 100), 1000
STEP_SECONDS = 420


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


def check_updated(ix, g0, g1, ids, vals):
    import numpy as np

    n = g0.n
    if ix.n != n or g1.n != n or not np.array_equal(g1.levels, g0.levels) or not np.array_equal(g1.up_off, g0.up_off):
        raise SystemExit("hnsw_update changed n, a level or up_off")
    for adj in (g1.l0_adj, g1.up_adj):
        if adj.size and (adj.min() < -1 or adj.max() >= n):
            raise SystemExit("the updated graph holds an id outside [0, n)")
    if (g1.M, g1.M0) != (g0.M, g0.M0) or not (0 <= g1.entry < n) or g1.levels[g1.entry] != g1.max_level:
        raise SystemExit("the updated graph's shape or entry point is wrong")
    probe = ids[:: max(1, len(ids) // 16)]
    for i, v in zip(probe, vals[:: max(1, len(ids) // 16)]):
        if abs(float(ix.batch_distances(v, ids=np.array([i], np.int32))[0])) > 1e-5:
            raise SystemExit("row %d did not take its new values" % i)
    linked = np.unique(g1.l0_adj[g1.l0_adj >= 0])
    if len(ids) > 1 and not np.isin(ids, linked).mean() > 0.9:
        raise SystemExit("the updated rows were not linked again")


def live_index(engine, base):
    ix = engine.Index(base, "cosine", 0)
    ix.set_rejection_test(MODE)
    ix.hnsw_build(M, EFC, SEED, heuristic=True)
    ix.sync()
    return ix


def _set(m, seed):
    """(base, ids, new values, the new base) of a step"""
    import numpy as np

    import bench  # (the headline set)

    n = bench.N31K
    base = bench.make_31k("clustered", 42, n)
    ids = np.random.default_rng(seed).choice(n, m, replace=False).astype(np.int32)
    vals = np.ascontiguousarray(bench.make_31k("clustered", 44, m), np.float32)   # rows of other clusters
    new_base = base.copy()
    new_base[ids] = vals
    return base, ids, vals, new_base


def remove_add(ix, ids, vals):
    ix.hnsw_remove(ids)
    ix.hnsw_add(vals, EFC, SEED)


def step_time(m, reps):
    """One batch size, in a process of its own: check, then measure; one JSON line on stdout."""
    import bench
    from hnsw_clj_amd import engine

    base, ids, vals, new_base = _set(m, 7)
    with live_index(engine, base) as ix:
        g0 = ix.get_graph()
        ix.hnsw_update(ids, vals, EFC)
        check_updated(ix, g0, ix.get_graph(), ids, vals)

    out = {"m": m, "n": len(base), "dim": bench.DIM,
           "update": timed(lambda: live_index(engine, base), lambda ix: ix.hnsw_update(ids, vals, EFC), reps),
           "rebuild": timed(lambda: None, lambda _: live_index(engine, new_base), reps),
           "remove_add": timed(lambda: live_index(engine, base), lambda ix: remove_add(ix, ids, vals), reps)}
    print("RESULT " + json.dumps(out))


def step_recall(share):
    """One updated share, in a process of its own: recall@10 at every ef of EFS of the updated, the freshly built and the remove +
    add graph."""
    import numpy as np

    import bench
    from hnsw_clj_amd import engine

    n = bench.N31K
    base, ids, vals, new_base = _set(n * share // 100, 11)
    Q = np.ascontiguousarray(bench.make_31k("clustered", 43, NQ))

    def recall(ix, truth):
        """recall@10 of ix's graph per ef of EFS"""
        return [float(np.mean([len(np.intersect1d(a, b)) for a, b in zip(ix.hnsw_search(Q, 10, ef)[0], truth)])) / truth.shape[1]
                for ef in EFS]

    out = {"share": share, "m": int(len(ids)), "n": n}
    with live_index(engine, base) as ix:
        g0 = ix.get_graph()
        truth0, _ = ix.exact_knn(Q, 10)
        out["before"] = recall(ix, truth0)
        ix.hnsw_update(ids, vals, EFC)
        check_updated(ix, g0, ix.get_graph(), ids, vals)
        truth, _ = ix.exact_knn(Q, 10)
        out["updated"] = recall(ix, truth)
    with live_index(engine, new_base) as ix:
        out["fresh"] = recall(ix, truth)
    with live_index(engine, base) as ix:                      # the same rows under new ids: the truth is its own
        remove_add(ix, ids, vals)
        truth_ra, _ = ix.exact_knn(Q, 10)
        out["remove_add"] = recall(ix, truth_ra)
    print("RESULT " + json.dumps(out))


def run_step(args_tail, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args_tail
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS)
    except subprocess.TimeoutExpired:
        raise SystemExit("step %s did not finish within %d s: nothing written" % (what, STEP_SECONDS))
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit("step %s failed with exit status %d: nothing written" % (what, p.returncode))
    return json.loads(line[-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_update.txt"))
    ap.add_argument("--step", type=int, default=None, help="(internal) measure this batch size and print one JSON line")
    ap.add_argument("--recall", type=int, default=None, help="(internal) recall after this share of the rows took new values, one JSON line")
    args = ap.parse_args()
    if args.step is not None:
        return step_time(args.step, args.reps)
    if args.recall is not None:
        return step_recall(args.recall)

    # each GPU step in a process of its own, under its own time limit; the first failure ends the run
    times = [run_step(["--step", str(m), "--reps", str(args.reps)], "m = %d" % m) for m in BATCHES]
    recalls = [run_step(["--recall", str(s)], "recall at %d %%" % s) for s in SHARES]

    r0 = times[0]
    lines = ["hnswgpu_hnsw_update, %d x %d cosine (clustered, normalised), heuristic graph M %d ef_construction %d, rejection mode %d"
             % (r0["n"], r0["dim"], M, EFC, MODE),
             "host clock around calls that end in a device synchronise; median of %d after a warm-up [min .. max], ms" % args.reps,
             "every update runs on a freshly built handle made outside the timed window; the new values are rows of other clusters;",
             "the rebuild is create + set_rejection_test + hnsw_build(heuristic) over the new base from host memory;",
             "the device-chain share of an update (hnswgpu_get_profile) was not measured",
             ""]
    fmt = "%-66s %9.3f  [%8.3f .. %8.3f]"
    for r in times:
        up, rb, ra = r["update"][0], r["rebuild"][0], r["remove_add"][0]
        lines += [fmt % (("hnsw_update of %d scattered rows of a handle over %d" % (r["m"], r["n"]),) + tuple(r["update"])),
                  fmt % (("(a) Index(the new base) + set_rejection_test + hnsw_build",) + tuple(r["rebuild"])),
                  fmt % (("(b) hnsw_remove + hnsw_add of the same rows (new ids, new levels)",) + tuple(r["remove_add"])),
                  "      update / (a) = %.4f: %s;  update / (b) = %.4f" % (
                      up / rb, "the update is faster" if up < rb else "the update is NOT faster than the rebuild", up / ra),
                  ""]
    lines += ["recall@10, %d held-out queries (bench.py's seed-43 stream), against the exact neighbours in the new base" % NQ,
              "(fresh: a new build over the new base; remove + add: the same rows under new ids, against its own exact neighbours)",
              ""]
    for r in recalls:
        for i, ef in enumerate(EFS):
            lines += ["%2d %% of the rows updated (%d of %d), ef %3d (before the update %.4f):  updated %.4f   fresh build %.4f   remove + add %.4f"
                      % (r["share"], r["m"], r["n"], ef, r["before"][i], r["updated"][i], r["fresh"][i], r["remove_add"][i])]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
