"""Developer tool: HNSW batch-size sweep on the bench workload (31,173 x 768 manifold data, ef 100), for every
waves-per-query setting the launcher can pick.  usage: python tools/hnsw_batch_sweep.py [ef]

python tools/hnsw_batch_sweep.py --order: the wave kernel's ordered launches (HNSW_ORDER 2) against plain ones (0) in ONE process
on bench.py's own index (31,173 x 768 clustered, heuristic builder): 2,048 / 4,096 / 10,000 queries at ef 640 and ef 100, the two
settings alternating, three rounds of 10 launches each; the table hnsw_launch_plan's threshold (kOrderMinQueries) is read from.

python tools/hnsw_batch_sweep.py --dense / --rows [ef:nq ...]: the same protocol for the dense bounds table (on against off) and
for the f32 rows in flight behind it (hnswgpu_hnsw_dense_rows 2 against 4): the tables beside the two rules in hnsw_launch_plan."""
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if len(sys.argv) > 1 and sys.argv[1] == "--dense":
    # python tools/hnsw_batch_sweep.py --dense [ef:nq ...]: the dense bounds table (hnswgpu_set_hnsw_dense_bounds 2) against none (0), as --order:
    # one process, bench.py's own index, the two settings alternating, three rounds of 10 launches; the table the rule in
    # hnsw_launch_plan is read from.
    import numpy as np
    import torch

    import bench
    from hnsw_clj_amd import engine

    base = bench.make_31k("clustered", 42, 31173)
    queries = bench.make_31k("clustered", 43, 10000)
    dev = torch.device("cuda", 0)
    idx = engine.Index(base, "cosine", 0)
    idx.hnsw_build(16, 200, 42, **bench.BUILDERS["heuristic"])
    print("ef    nq      no table ms (3 rounds)     table ms (3 rounds)        table / none (medians)", flush=True)
    shapes = [tuple(int(x) for x in s.split(":")) for s in sys.argv[2:]]      # further shapes: ef:nq ...
    for ef, nq in shapes or ((640, 2048), (640, 4096), (640, 10000), (100, 4096), (100, 10000), (1600, 10000),
                             (200, 4096), (200, 10000), (320, 4096), (320, 10000)):
        Q = torch.from_numpy(queries[:nq]).to(dev)
        out = (torch.empty((nq, 10), dtype=torch.int32, device=dev), torch.empty((nq, 10), dtype=torch.float32, device=dev))
        ms = {0: [], 2: []}
        for rnd in range(4):                      # round 0 warms up
            for mode in (0, 2):
                idx.set_hnsw_dense_bounds(mode)
                idx.hnsw_search_dev(Q, 10, ef, out=out)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    idx.hnsw_search_dev(Q, 10, ef, out=out)
                torch.cuda.synchronize()
                if rnd:
                    ms[mode].append((time.perf_counter() - t0) / 10 * 1e3)
        med = {m: sorted(v)[1] for m, v in ms.items()}
        print("%-5d %-7d %-26s %-26s %.4f" % (ef, nq, " ".join("%.4f" % v for v in ms[0]), " ".join("%.4f" % v for v in ms[2]),
                                           med[2] / med[0]), flush=True)
    idx.set_hnsw_dense_bounds(1)
    print("state (mode, budget MiB, launches with the table, scratch bytes):", idx.hnsw_dense_bounds_state())
elif len(sys.argv) > 1 and sys.argv[1] == "--rows":
    # python tools/hnsw_batch_sweep.py --rows: two f32 rows in flight against four in the launches with the dense bounds table
    # (hnswgpu_hnsw_dense_rows 2 / 4), as --dense: one process, bench.py's own index, the two settings alternating, three rounds of 10
    # launches; the table the rows-in-flight rule in hnsw_launch_plan is read from.  The table is forced on (mode 2) so that the ef
    # below the dense rule's threshold are measured too.
    import numpy as np
    import torch

    import bench
    from hnsw_clj_amd import engine

    base = bench.make_31k("clustered", 42, 31173)
    queries = bench.make_31k("clustered", 43, 10000)
    dev = torch.device("cuda", 0)
    idx = engine.Index(base, "cosine", 0)
    idx.hnsw_build(16, 200, 42, **bench.BUILDERS["heuristic"])
    idx.set_hnsw_dense_bounds(2)
    print("ef    nq      two rows ms (3 rounds)     four rows ms (3 rounds)    four / two (medians)", flush=True)
    shapes = [tuple(int(x) for x in s.split(":")) for s in sys.argv[2:]]      # further shapes: ef:nq ...
    for ef, nq in shapes or ((640, 2048), (640, 4096), (640, 10000), (1600, 10000), (288, 10000), (320, 10000), (448, 10000)):
        Q = torch.from_numpy(queries[:nq]).to(dev)
        out = (torch.empty((nq, 10), dtype=torch.int32, device=dev), torch.empty((nq, 10), dtype=torch.float32, device=dev))
        ms = {2: [], 4: []}
        for rnd in range(4):                      # round 0 warms up
            for rows in (2, 4):
                idx.hnsw_dense_rows(rows)
                idx.hnsw_search_dev(Q, 10, ef, out=out)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    idx.hnsw_search_dev(Q, 10, ef, out=out)
                torch.cuda.synchronize()
                if rnd:
                    ms[rows].append((time.perf_counter() - t0) / 10 * 1e3)
        med = {m: sorted(v)[1] for m, v in ms.items()}
        print("%-5d %-7d %-26s %-26s %.4f" % (ef, nq, " ".join("%.4f" % v for v in ms[2]), " ".join("%.4f" % v for v in ms[4]),
                                           med[4] / med[2]), flush=True)
    idx.set_hnsw_dense_bounds(1)
    print("launch counter hnsw_wave %d; launches with the table %d, of them with four rows %d" % (
        engine.debug_counter("hnsw_wave"), idx.hnsw_dense_bounds_state()[2], idx.hnsw_dense_rows(0)[1]))
elif len(sys.argv) > 1 and sys.argv[1] == "--order":
    import numpy as np
    import torch

    import bench
    from hnsw_clj_amd import engine

    base = bench.make_31k("clustered", 42, 31173)
    queries = bench.make_31k("clustered", 43, 10000)
    dev = torch.device("cuda", 0)
    idx = engine.Index(base, "cosine", 0)
    idx.hnsw_build(16, 200, 42, **bench.BUILDERS["heuristic"])
    print("ef    nq      plain ms (3 rounds)        ordered ms (3 rounds)      ordered / plain (medians)", flush=True)
    for ef in (640, 100):
        for nq in (2048, 4096, 10000):
            Q = torch.from_numpy(queries[:nq]).to(dev)
            out = (torch.empty((nq, 10), dtype=torch.int32, device=dev), torch.empty((nq, 10), dtype=torch.float32, device=dev))
            ms = {0: [], 2: []}
            for rnd in range(4):                      # round 0 warms up
                for mode in (0, 2):
                    engine.set_tuning("HNSW_ORDER", mode)
                    idx.hnsw_search_dev(Q, 10, ef, out=out)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(10):
                        idx.hnsw_search_dev(Q, 10, ef, out=out)
                    torch.cuda.synchronize()
                    if rnd:
                        ms[mode].append((time.perf_counter() - t0) / 10 * 1e3)
            med = {m: sorted(v)[1] for m, v in ms.items()}
            print("%-5d %-7d %-26s %-26s %.4f" % (ef, nq, " ".join("%.4f" % v for v in ms[0]), " ".join("%.4f" % v for v in ms[2]),
                                               med[2] / med[0]), flush=True)
    engine.set_tuning("HNSW_ORDER", None)
    print("launch counters: hnsw_wave %d, hnsw_ordered %d" % (engine.debug_counter("hnsw_wave"), engine.debug_counter("hnsw_ordered")))
elif len(sys.argv) > 1 and sys.argv[1] == "--child":
    import numpy as np
    import torch

    import bench
    from hnsw_clj_amd import engine

    ef = int(sys.argv[2])
    base = bench.make_31k("manifold", 42, 31173)
    queries = bench.make_31k("manifold", 43, 10000)
    dev = torch.device("cuda", 0)
    idx = engine.Index(base, "cosine", 0)
    idx.hnsw_build(16, 200, 42)
    res = []
    for nq in (1, 8, 32, 128, 256, 512, 768, 1024, 1536, 2048, 3072, 4096, 10000):
        Q = torch.from_numpy(queries[:nq]).to(dev)
        out = (torch.empty((nq, 10), dtype=torch.int32, device=dev), torch.empty((nq, 10), dtype=torch.float32, device=dev))
        for _ in range(3):
            idx.hnsw_search_dev(Q, 10, ef, out=out)
        torch.cuda.synchronize()
        steps = 20 if nq <= 1024 else 8
        t0 = time.perf_counter()
        for _ in range(steps):
            idx.hnsw_search_dev(Q, 10, ef, out=out)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        res.append("%d:%.3fms/%.0fk" % (nq, dt * 1e3, nq / dt / 1e3))
    print("NW=%-4s " % os.environ.get("HNSWGPU_HNSW_NW", "auto") + "  ".join(res), flush=True)
else:
    ef = sys.argv[1] if len(sys.argv) > 1 else "100"
    for nw in (None, "1", "2", "4"):
        env = dict(os.environ)
        if nw:
            env["HNSWGPU_TUNE"] = "HNSW_NW=%s" % nw
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", ef], env=env, check=False)
