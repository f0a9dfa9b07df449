"""hnswgpu_hnsw_remove on the headline set: what a batch of rows that leave costs a live HNSW index, at a few batch sizes, beside
the only alternative there was before -- a fresh handle over the kept rows from host memory, built again (create +
set_rejection_test + hnsw_build with the same builder) -- and what the one-hop repair is worth: recall@10 after 10 % and 40 % of
the rows left, for the repaired graph, the same graph merely compacted (every list keeps its kept members, nothing else; made
here in numpy and installed through set_graph) and a fresh build of the kept rows.

31,173 x 768 (bench.py's clustered, normalised set), cosine, the heuristic builder with M 16 and ef_construction 200, rejection
mode 1 (the default: int8 rows exist at dim 768).  Times: the host clock around calls that end in a device synchronise (a removal
is host and device work: it ends behind its readback); per line the median of --reps runs after one warm-up, with the range
beside it.  A removal changes its handle, so every run of one gets a freshly built handle, made outside the timed window.
Recall: bench.py's 1,000 held-out queries (the seed-43 stream: other centres than the base's, the headline's 0.98 at ef 640), at
ef 640 and, where ef 640 leaves no room to tell the graphs apart, ef 100; against the exact neighbours among the kept rows
(exact_knn on the kept rows).

Every batch size and every removed share is a step of its own: a child process under its own time limit that first checks what
it measures (the kept ids, the shrunken graph's levels and shape, every edge inside the new numbering) and then measures.  The
first step that fails or runs out of time ends the run and nothing is written.  No threshold is set: the file records what was
measured.  Writes profiles/hnsw_remove.txt.

    python tools/hnsw_remove_timing.py [--reps 5] [--out profiles/hnsw_remove.txt]
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
SHARES = (10, 40)                # per cent of the rows removed for the recall lines
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


def compacted(engine, g, keep):
    """The graph g with the rows outside `keep` dropped and nothing repaired: every list keeps its kept members in their order
    under their new ids; the entry point moves as hnswgpu_hnsw_remove moves it."""
    import numpy as np

    n = len(keep)
    new_id = np.full(n, -1, np.int64)
    new_id[keep] = np.arange(keep.sum())

    def close_up(adj):
        mapped = np.where(adj >= 0, new_id[np.maximum(adj, 0)], -1)
        order = np.argsort(mapped < 0, axis=1, kind="stable")
        return np.take_along_axis(mapped, order, axis=1).astype(np.int32)

    levels = g.levels[keep]
    up_off = np.concatenate([[0], np.cumsum(levels)]).astype(np.int64)
    owner = np.repeat(np.arange(n), g.levels)
    l0 = close_up(g.l0_adj.reshape(n, -1)[keep])
    up = close_up(g.up_adj.reshape(-1, g.M)[keep[owner]])
    if keep[g.entry]:
        entry, top = int(new_id[g.entry]), g.max_level
    else:
        entry = int(np.argmax(levels))
        top = int(levels[entry])
    return engine.Graph(levels, l0, up_off, up.reshape(-1), g.M, entry, top)


def check_shrunken(g0, g1, keep, kept):
    import numpy as np

    if not np.array_equal(kept, np.flatnonzero(keep)):
        raise SystemExit("hnsw_remove kept other rows than the mask")
    n1 = int(keep.sum())
    if g1.n != n1 or not np.array_equal(g1.levels, g0.levels[keep]) or g1.up_off[-1] != g0.levels[keep].sum():
        raise SystemExit("the shrunken graph's levels are not the kept rows' levels")
    for adj in (g1.l0_adj, g1.up_adj):
        if adj.size and (adj.min() < -1 or adj.max() >= n1):
            raise SystemExit("the shrunken graph holds an id outside the new numbering")
    if (g1.M, g1.M0) != (g0.M, g0.M0) or not (0 <= g1.entry < n1) or g1.levels[g1.entry] != g1.max_level:
        raise SystemExit("the shrunken graph's shape or entry point is wrong")


def live_index(engine, base):
    ix = engine.Index(base, "cosine", 0)
    ix.set_rejection_test(MODE)
    ix.hnsw_build(M, EFC, SEED, heuristic=True)
    ix.sync()
    return ix


def step_time(m, reps):
    """One batch size, in a process of its own: check, then measure; one JSON line on stdout."""
    import numpy as np

    import bench  # (the headline set)
    from hnsw_clj_amd import engine

    n, dim = bench.N31K, bench.DIM
    base = bench.make_31k("clustered", 42, n)
    gone = np.random.default_rng(7).choice(n, m, replace=False).astype(np.int32)
    keep = np.ones(n, np.bool_)
    keep[gone] = False
    kept_rows = np.ascontiguousarray(base[keep])

    with live_index(engine, base) as ix:
        g0 = ix.get_graph()
        kept = ix.hnsw_remove(gone)
        check_shrunken(g0, ix.get_graph(), keep, kept)

    def remove(ix):
        ix.hnsw_remove(gone)

    def rebuild(_=None):
        return live_index(engine, kept_rows)

    out = {"m": m, "n": n, "dim": dim, "kept": int(keep.sum()),
           "remove": timed(lambda: live_index(engine, base), remove, reps),
           "rebuild": timed(lambda: None, rebuild, reps)}
    print("RESULT " + json.dumps(out))


def step_recall(share):
    """One removed share, in a process of its own: recall@10 at every ef of EFS of the repaired, the compacted and the freshly built
    graph."""
    import numpy as np

    import bench
    from hnsw_clj_amd import engine

    n = bench.N31K
    base = bench.make_31k("clustered", 42, n)
    Q = np.ascontiguousarray(bench.make_31k("clustered", 43, NQ))
    gone = np.random.default_rng(11).choice(n, n * share // 100, replace=False).astype(np.int32)
    keep = np.ones(n, np.bool_)
    keep[gone] = False
    kept_rows = np.ascontiguousarray(base[keep])

    def recall(ix, truth):
        """recall@10 of ix's graph per ef of EFS"""
        return [float(np.mean([len(np.intersect1d(a, b)) for a, b in zip(ix.hnsw_search(Q, 10, ef)[0], truth)])) / truth.shape[1]
                for ef in EFS]

    out = {"share": share, "m": int(len(gone)), "kept": int(keep.sum())}
    with live_index(engine, base) as ix:
        g0 = ix.get_graph()
        truth0, _ = ix.exact_knn(Q, 10)
        out["before"] = recall(ix, truth0)
        kept = ix.hnsw_remove(gone)
        check_shrunken(g0, ix.get_graph(), keep, kept)
        truth, _ = ix.exact_knn(Q, 10)
        out["repaired"] = recall(ix, truth)
    with engine.Index(kept_rows, "cosine", 0) as ix:
        ix.set_rejection_test(MODE)
        ix.set_graph(compacted(engine, g0, keep))
        out["compacted"] = recall(ix, truth)
    with live_index(engine, kept_rows) as ix:
        out["fresh"] = recall(ix, truth)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hnsw_remove.txt"))
    ap.add_argument("--step", type=int, default=None, help="(internal) measure this batch size and print one JSON line")
    ap.add_argument("--recall", type=int, default=None, help="(internal) recall after this share of the rows left, one JSON line")
    args = ap.parse_args()
    if args.step is not None:
        return step_time(args.step, args.reps)
    if args.recall is not None:
        return step_recall(args.recall)

    # each GPU step in a process of its own, under its own time limit; the first failure ends the run
    times = [run_step(["--step", str(m), "--reps", str(args.reps)], "m = %d" % m) for m in BATCHES]
    recalls = [run_step(["--recall", str(s)], "recall at %d %%" % s) for s in SHARES]

    r0 = times[0]
    lines = ["hnswgpu_hnsw_remove, %d x %d cosine (clustered, normalised), heuristic graph M %d ef_construction %d, rejection mode %d"
             % (r0["n"], r0["dim"], M, EFC, MODE),
             "host clock around calls that end in a device synchronise; median of %d after a warm-up [min .. max], ms" % args.reps,
             "every removal runs on a freshly built handle made outside the timed window; the rebuild is create + set_rejection_test +",
             "hnsw_build(heuristic) over the kept rows from host memory",
             ""]
    fmt = "%-66s %9.3f  [%8.3f .. %8.3f]"
    for r in times:
        lines += [fmt % (("(a) hnsw_remove of %d scattered rows from a handle over %d" % (r["m"], r["n"]),) + tuple(r["remove"])),
                  fmt % (("(b) Index(the %d kept rows) + set_rejection_test + hnsw_build" % r["kept"],) + tuple(r["rebuild"])),
                  "      (a) / (b) = %.4f: %s" % (r["remove"][0] / r["rebuild"][0],
                                                  "the removal is faster" if r["remove"][0] < r["rebuild"][0] else "the removal is NOT faster than the rebuild"),
                  ""]
    lines += ["recall@10, %d held-out queries (bench.py's seed-43 stream), against the exact neighbours among the kept rows" % NQ,
              "(compacted: every list keeps its kept members and nothing else -- the repair switched off; fresh: a new build of the kept rows)",
              ""]
    for r in recalls:
        for i, ef in enumerate(EFS):
            lines += ["%2d %% of the rows removed (%d of %d), ef %3d (before the removal %.4f):  repaired %.4f   compacted %.4f   fresh build %.4f"
                      % (r["share"], r["m"], r["m"] + r["kept"], ef, r["before"][i], r["repaired"][i], r["compacted"][i], r["fresh"][i])]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
