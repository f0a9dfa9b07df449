"""hnswgpu_pcaf_add / _remove / _update on a P-HNSW handle of a size a user would run: what a batch of rows that join, leave or
take new values costs a live handle, at a few batch sizes, beside the only thing there was before: a fresh handle over the rows
the handle should then hold, from host memory (hnswgpu_create + hnswgpu_set_pcaf with the same projection: an upload of the whole
base and a projection of every row).

100,000 x 768 clustered, normalised rows (256 centres, noise 0.3), cosine, T = 100 (the reference's default).  Rows that leave
or take new values are scattered; new values and new rows are other draws from the same mixture.  The host clock around calls that
end in a device synchronise; per line the median of --reps runs after one warm-up, with the range beside it.  A mutation and
its rebuild alternate in one process.  A mutation changes its handle, so every run of one gets a fresh handle (create + set_pcaf),
made outside the timed window.

Every batch size is a step of its own: a child process under its own time limit that first compares every mutated handle with the
fresh one (projected rows, norms, one search's bits) and then measures.  The first step that fails or runs out of time ends the
run and nothing is written.  No threshold is set: the file records what was measured.

    python tools/pcaf_mutation_timing.py [--reps 5] [--out profiles/pcaf_mutations.txt]

Measured on one MI355X (profiles/pcaf_mutations.txt): a call is 0.05 - 0.16 of its rebuild -- add 0.70 / 0.86 / 1.52 ms, remove
0.61 / 0.64 / 0.87 ms, update 0.72 / 0.64 / 1.94 ms at m = 1 / 1,024 / 8,192 against 10.8 - 12.8 ms -- faster at every m measured.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, DIM, T = 100000, 768, 100
BATCHES = (1, 1024, 8192)
STEP_SECONDS = 240


def _rows(rng, centres, count):
    import numpy as np

    x = centres[rng.integers(0, len(centres), count)] + 0.3 * rng.standard_normal((count, DIM)).astype(np.float32)
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True), np.float32)


def step(m, reps):
    """One batch size, in a process of its own: check, then measure; one JSON line on stdout."""
    import numpy as np

    from hnsw_clj_amd import engine, pcaf

    rng = np.random.default_rng(7)
    centres = rng.standard_normal((256, DIM)).astype(np.float32)
    base, new = _rows(rng, centres, N), _rows(rng, centres, m)
    at = rng.choice(N, m, replace=False).astype(np.int32)    # scattered rows
    P = pcaf.create_random_projection(DIM, T)
    updated = base.copy()
    updated[at] = new
    # the mutation on a live handle, and the rows the handle should then hold
    ops = {"add": (lambda ix: ix.pcaf_add(new), np.concatenate([base, new])),
           "remove": (lambda ix: ix.pcaf_remove(at), np.delete(base, at, axis=0)),
           "update": (lambda ix: ix.pcaf_update(at, new), updated)}

    def handle(rows):
        ix = engine.Index(rows, "cosine", 0)
        ix.set_pcaf(P)
        return ix

    def live():
        ix = handle(base)
        ix.sync()
        return ix

    # what is timed computes what it should: the mutated handle against the fresh one over the rows it should hold
    Q = np.ascontiguousarray(base[:16])
    for name, (mutate, rows) in ops.items():
        with live() as ix, handle(rows) as want:
            mutate(ix)
            same = (ix.n == want.n and np.array_equal(ix.pcaf_get()[1].view(np.uint32), want.pcaf_get()[1].view(np.uint32))
                    and np.array_equal(ix.norms().view(np.uint32), want.norms().view(np.uint32))
                    and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(ix.pcaf_search(Q, 10), want.pcaf_search(Q, 10))))
            if not same:
                raise SystemExit("after %s the handle differs from the fresh one" % name)

    def clock(fn, arg):
        t0 = time.perf_counter()
        made = fn(arg)
        dt = (time.perf_counter() - t0) * 1e3
        if isinstance(made, engine.Index):
            made.close()
        return dt

    t = {name: {"call": [], "rebuild": []} for name in ops}
    for r in range(reps + 1):                                # a mutation and its rebuild alternate; run 0 is the warm-up
        for name, (mutate, rows) in ops.items():
            ix = live()
            a = clock(mutate, ix)
            ix.close()
            b = clock(handle, rows)
            if r:
                t[name]["call"].append(a)
                t[name]["rebuild"].append(b)
    out = {"m": m}
    for name in ops:
        out[name] = {k: (float(np.median(v)), min(v), max(v)) for k, v in t[name].items()}
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcaf_mutations.txt"))
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

    lines = ["hnswgpu_pcaf_add / _remove / _update, %d x %d cosine (clustered, normalised), T = %d" % (N, DIM, T),
             "host clock around calls that end in a device synchronise; median of %d after a warm-up [min .. max], ms" % args.reps,
             "a mutation and its rebuild alternate in one process; every mutation runs on a fresh handle made outside the timed window;",
             "the mutated handle equals the fresh handle's projected rows, norms and one search's bits",
             ""]
    fmt = "%-86s %9.3f  [%8.3f .. %8.3f]"
    what = {"add": "pcaf_add of %d rows to a handle over %d", "remove": "pcaf_remove of %d scattered rows of a handle over %d",
            "update": "pcaf_update of %d scattered rows of a handle over %d"}
    for r in results:
        for name in ("add", "remove", "update"):
            call, rebuild = r[name]["call"], r[name]["rebuild"]
            lines += [fmt % ((what[name] % (r["m"], N),) + tuple(call)),
                      fmt % (("    Index(the rows it should then hold) + set_pcaf(projection)",) + tuple(rebuild)),
                      "    call / rebuild = %.3f: %s" % (call[0] / rebuild[0], "the call is faster" if call[0] < rebuild[0]
                                                         else "the call is NOT faster than the rebuild")]
        lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
