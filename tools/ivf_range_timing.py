"""Developer tool: hnswgpu_ivf_range_search against the exact range search and against the composition it replaces, on the data
of profiles/range_search.txt (31,173 x 768 clustered, cosine) with an IVF handle of 64 lists.  Device ms per call by events
around 5 calls, 7 alternating rounds, median [min, max]; recall = hits found / exact hits.
    a  range_search_dev                 the exact call
    b  range_search_filtered_each_dev   the composition's device part: one allow-mask per query = the rows of its probed lists
    b+ ... with its host part (wall)    ivf_search(want_probes), the nq x n mask bits built and packed on the host, the upload
    c  ivf_range_search_dev             routed, stream order
    d  ... by distance
usage: python tools/ivf_range_timing.py [out file]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bench
from hnsw_clj_amd import engine

NLIST, ROUNDS, CALLS = 64, 7, 5
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout


def say(s):
    print(s, file=out, flush=True)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / CALLS


base = bench.make_31k("clustered", 42, 31173)
queries = bench.make_31k("clustered", 43, 1024)
idx = engine.Index(base, "cosine", 0)
idx.ivf_build(NLIST, 10, 42)
_, off, list_ids = idx.get_ivf()
lens = np.diff(off)
say("31,173 x 768 clustered, cosine, %d lists (rows per list: min %d, median %d, max %d); device ms per call (events around %d calls), "
    "%d alternating rounds: median [min, max]" % (NLIST, lens.min(), np.median(lens), lens.max(), CALLS, ROUNDS))
dev = torch.device("cuda", 0)
dense = idx.dense_distances_dev(torch.from_numpy(queries).to(dev))
for nq in (1, 32, 1024):
    Q = torch.from_numpy(queries[:nq]).to(dev)
    for hits in (10, 1000):
        rad = torch.kthvalue(dense[:nq], hits, dim=1).values.contiguous()
        exact = idx.range_search_dev(Q, rad, 0)[0]
        torch.cuda.synchronize()
        cap = int(exact[-1])
        for nprobe in (4, 16):
            t0 = time.perf_counter()
            probes = idx.ivf_search(queries[:nq], 1, nprobe, want_probes=True)[2]
            bits = np.zeros((nq, idx.n), np.bool_)
            for q in range(nq):
                for l in probes[q]:
                    bits[q, list_ids[off[l]:off[l + 1]]] = True
            masks = torch.from_numpy(engine.pack_masks(bits, idx.n).view(np.int32)).to(dev)
            torch.cuda.synchronize()
            host_ms = (time.perf_counter() - t0) * 1e3
            found = int(idx.ivf_range_search_dev(Q, rad, nprobe, 0)[0][-1])
            via_masks = int(idx.range_search_filtered_each_dev(Q, rad, masks, 0)[0][-1])
            assert found == via_masks, (found, via_masks)
            bufs = (torch.empty(nq + 1, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                    torch.empty(cap, dtype=torch.float32, device=dev))
            runs = {"a exact range_search_dev": lambda: idx.range_search_dev(Q, rad, cap, out=bufs),
                    "b range_search_filtered_each_dev, masks ready": lambda: idx.range_search_filtered_each_dev(Q, rad, masks, cap, out=bufs),
                    "c ivf_range_search_dev, stream order": lambda: idx.ivf_range_search_dev(Q, rad, nprobe, cap, out=bufs),
                    "d ivf_range_search_dev, by distance": lambda: idx.ivf_range_search_dev(Q, rad, nprobe, cap, by_distance=True, out=bufs)}
            ms = {k: [] for k in runs}
            for rnd in range(ROUNDS + 1):             # round 0 warms up
                for k, fn in runs.items():
                    t = timed(fn)
                    if rnd:
                        ms[k].append(t)
            say("nq %4d, ~%4d exact hits per query (%d), nprobe %2d of %d: %d found, recall %.3f" % (nq, hits, cap, nprobe, NLIST, found, found / cap))
            for k, v in ms.items():
                say("    %-48s %8.3f [%8.3f, %8.3f]" % (k, np.median(v), min(v), max(v)))
            say("    %-48s %8.3f   (once)" % ("b+ the composition's host part (wall)", host_ms))
idx.close()
