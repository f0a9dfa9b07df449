"""P-HNSW filtered search (hnswgpu_pcaf_search_filtered_dev / _each_dev) beside the unfiltered search (hnswgpu_pcaf_search_dev)
in one process on one card: what the gather and the id build cost (all-ones mask against no mask) and what compaction buys
(10 % and 1 % of random bits against 100 %).

N x 768 clustered rows made on the device from a seed, n_components 100, k 10, k_filter 32; batches of 32 and 1024 queries resident
on the device.  Rows: no mask; one mask at 100 %, 10 %, 1 %; one mask per query with all rows equal (10 %); one mask per query,
all distinct (32 distinct 10 % masks per block of 32 queries).  Every row is warmed up, then timed in windows of --calls launches
between two device events, the rows alternating window by window; the median of --reps windows and their range are written, per
call.  Before timing, the all-ones results are compared bit for bit with the unfiltered ones and the 10 % results with the mask.

    python tools/pcaf_filtered_timing.py [--n 1000000] [--reps 15] [--calls 20] [--out profiles/pcaf_filtered.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, T, K, KF = 768, 100, 10, 32
BATCHES = (32, 1024)


def main(n, reps, calls, out):
    import torch

    from hnsw_clj_amd import engine

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(42)
    centers = torch.randn((64, DIM), generator=g, device=dev)
    base = centers[torch.randint(0, 64, (n,), generator=g, device=dev)] + 0.6 * torch.randn((n, DIM), generator=g, device=dev)
    Q = centers[torch.randint(0, 64, (max(BATCHES),), generator=g, device=dev)] + 0.6 * torch.randn((max(BATCHES), DIM), generator=g, device=dev)
    idx = engine.Index(base, "cosine", 0)
    del base
    idx.pcaf_build(T, 42)
    W = (n + 31) // 32

    def words(rate, rows, seed):  # [rows][W] int32 on the device, bits at positions >= n clear
        gm = torch.Generator(device=dev).manual_seed(seed)
        bits = torch.rand((rows, W * 32), generator=gm, device=dev) < rate
        bits[:, n:] = False
        weights = (1 << torch.arange(32, device=dev, dtype=torch.int64))
        return (bits.view(rows, W, 32).to(torch.int64) * weights).sum(dim=2).to(torch.int32).contiguous()

    one = {rate: words(rate, 1, 7)[0].contiguous() for rate in (1.0, 0.1, 0.01)}
    lines = ["P-HNSW search, %d x %d rows, n_components %d, k %d, k_filter %d; ms per call, median (min - max) of %d windows of %d calls"
             % (n, DIM, T, K, KF, reps, calls),
             "%6s  %-34s  %30s  %10s  %10s" % ("nq", "entry", "ms per call", "/ no mask", "/ 100 %")]
    for nq in BATCHES:
        q = Q[:nq].contiguous()
        outs = (torch.empty((nq, K), dtype=torch.int32, device=dev), torch.empty((nq, K), dtype=torch.float32, device=dev))
        same = one[0.1].repeat(nq, 1).contiguous()
        distinct = torch.cat([words(0.1, min(64, nq - r), 100 + r) for r in range(0, nq, 64)]).contiguous()
        rows = [("no mask", lambda: idx.pcaf_search_dev(q, K, KF, out=outs))]
        rows += [("one mask, %g %% pass" % (100 * rate), lambda m=m: idx.pcaf_search_filtered_dev(q, K, m, KF, out=outs))
                 for rate, m in one.items()]
        rows += [("mask per query, 1 distinct, 10 %", lambda: idx.pcaf_search_filtered_each_dev(q, K, same, KF, out=outs)),
                 ("mask per query, all distinct, 10 %", lambda: idx.pcaf_search_filtered_each_dev(q, K, distinct, KF, out=outs))]
        res = {}
        for name, fn in rows:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            res[name] = (outs[0].cpu().numpy().copy(), outs[1].cpu().numpy().copy())
        assert np.array_equal(res["no mask"][0], res["one mask, 100 % pass"][0])
        assert np.array_equal(res["no mask"][1].view(np.uint32), res["one mask, 100 % pass"][1].view(np.uint32))
        m10 = one[0.1].cpu().numpy().view(np.uint32)
        for name in ("one mask, 10 % pass", "mask per query, 1 distinct, 10 %"):
            ids = res[name][0]
            assert (ids >= 0).all() and ((m10[ids >> 5] >> (ids & 31)) & 1).all(), name
        assert np.array_equal(res["one mask, 10 % pass"][0], res["mask per query, 1 distinct, 10 %"][0])
        ms = {name: [] for name, _ in rows}
        for _ in range(reps):
            for name, fn in rows:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / calls)
        med = {name: float(np.median(v)) for name, v in ms.items()}
        for name, _ in rows:
            v = ms[name]
            lines.append("%6d  %-34s  %9.4f (%8.4f - %8.4f)  %10.2f  %10.2f"
                         % (nq, name, med[name], min(v), max(v), med[name] / med["no mask"], med[name] / med["one mask, 100 % pass"]))
            print(lines[-1], flush=True)
    idx.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcaf_filtered.txt"))
    a = ap.parse_args()
    main(a.n, a.reps, a.calls, a.out)
