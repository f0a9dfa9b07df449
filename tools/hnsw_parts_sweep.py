"""Developer tool: IVF-HNSW as one forest handle against the composition of 24 handles, in ONE process.

The reference's IVF-HNSW shape (ivf_hnsw.clj: 24 partitions, M 16, ef-construction 200) is built twice from the same data --
bench.py's 31,173 x 768 clustered set --: one_handle=False (a handle, a launch and a host round trip per partition: the yardstick)
and one_handle=True (hnswgpu_hnsw_build_parts + hnswgpu_hnsw_search_parts_dev: every (query, probe) pair in one launch).  The two
search_batch_dev paths are timed alternately, five rounds each behind a warm-up round, for batches of 1, 32, 1,024 and 10,000
queries in modes `fast` (2 probes) and `precise` (5 probes); the results are asserted equal (ids and distance bits) before
anything is timed.  A time is a host clock around `reps` calls that end in a device synchronise.

usage: python tools/hnsw_parts_sweep.py [out.txt]      (prints the table; writes it to out.txt as well)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS = 5
BATCHES = ((1, 200), (32, 100), (1024, 20), (10000, 5))          # (queries, calls per timed round)
MODES = ("fast", "precise")


def main():
    import numpy as np
    import torch

    import bench
    from hnsw_clj_amd import datagen, engine, ivf_hnsw

    assert engine.device_count() >= 1, "no GPU: nothing here can be measured without one"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    base = bench.make_31k("clustered", 42, 31173)
    queries = bench.make_31k("clustered", 43, 10000)
    data = datagen.indexed(base)
    dev = torch.device("cuda", 0)
    built = {}
    for one in (False, True):
        t0 = time.perf_counter()
        built[one] = ivf_hnsw.build_ivf_hnsw_index(data, num_partitions=24, M=16, ef_construction=200, one_handle=one)
        torch.cuda.synchronize()
        say("build one_handle=%s: %.2f s (k-means included)" % (one, time.perf_counter() - t0))
    sizes = [len(r) for r in built[True].rows]
    say("partitions: %d, rows %d .. %d" % (len(sizes), min(sizes), max(sizes)))
    k = 10
    say("k %d; ms per call: median [min .. max] of %d rounds; ratio = one handle / composition (medians)" % (k, ROUNDS))
    say("%-8s %-7s %-34s %-34s %s" % ("mode", "nq", "composition (24 handles)", "one handle (forest)", "ratio"))
    for mode in MODES:
        for nq, reps in BATCHES:
            Q = torch.from_numpy(queries[:nq]).to(dev)
            a = ivf_hnsw.search_batch_dev(built[False], Q, k, mode)
            b = ivf_hnsw.search_batch_dev(built[True], Q, k, mode)
            torch.cuda.synchronize()
            assert torch.equal(a[0], b[0]), "ids differ: mode %s, %d queries" % (mode, nq)
            assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), "distance bits differ: mode %s, %d queries" % (mode, nq)
            ms = {False: [], True: []}
            for rnd in range(ROUNDS + 1):                        # round 0 warms up
                for one in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        ivf_hnsw.search_batch_dev(built[one], Q, k, mode)
                    torch.cuda.synchronize()
                    if rnd:
                        ms[one].append((time.perf_counter() - t0) / reps * 1e3)
            med = {o: float(np.median(v)) for o, v in ms.items()}
            cell = {o: "%.3f [%.3f .. %.3f]" % (med[o], min(ms[o]), max(ms[o])) for o in ms}
            say("%-8s %-7d %-34s %-34s %.3f" % (mode, nq, cell[False], cell[True], med[True] / med[False]))
    say("launch counters: hnsw_wave %d, hnsw_solo %d, hnsw_helpers %d" % tuple(engine.debug_counter(c) for c in ("hnsw_wave", "hnsw_solo", "hnsw_helpers")))
    for ix in built.values():
        ix.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
