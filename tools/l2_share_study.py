"""Developer study (CPU, oracle): what would serving neighbouring queries on one XCD buy the wave traversal's L2 hit rate?

The headline launch (10,000 queries, 31,173 x 768 clustered, ef 640) is bound by the bytes that leave the XCD L2s, and its L2 hit
rate is about 8 %: query qi runs in workgroup qi, workgroups are dealt round-robin over the 8 XCDs, so queries that read the same
rows meet in one L2 at one time only by chance.  This models ONE XCD under an order of the batch given by a per-query KEY:

  * data: bench.py's own (hnsw_clj_amd.datagen through bench.make_31k, seeds 42 / 43); graph: the oracle's heuristic builder;
  * traversal: the upper layers' greedy descent, then layer 0 best-first at ef, recording per hop the fresh neighbours (an int8
    row each, 784 B) and the admitted ones (an f32 row each, 3,136 B with its norm line);
  * order: the queries sorted by (key, index); XCD x serves the x-th eighth of it front to back (order_kernels.hpp), "dealt" =
    today's launch (XCD 0 serves queries 0, 8, 16, ...);
  * the XCD: 512 resident queries (16 waves x 32 CUs), every resident query advances one hop per time step, a finished query is
    replaced by the XCD's next; an LRU cache of 4 MiB.  The first `--sim` queries of XCD 0's share are simulated.

Keys: dealt | centre (the generating centre: the ideal, not available to the library) | pivot:P (nearest of P base rows at stride
n // P, exact cosine) | pivot8:P (the same judged on int8 rows: what the key pass computes) | level:L (nearest node of level >= L)
| descent:L (the node the greedy descent reaches at level L) | all.  Beside the hit rate: the XCDs' load imbalance under the order
(evaluations per XCD from the oracle's search of the whole batch, max / mean).

usage: python tools/l2_share_study.py [--key all] [--sim 640] [--nq 10000] [--ef 640]      (no GPU, nothing outside the repository)"""
import argparse
import heapq
import os
import sys
import time
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from hnsw_clj_amd import datagen  # noqa: E402
from oracle import oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--key", default="all")
ap.add_argument("--sim", type=int, default=640)
ap.add_argument("--nq", type=int, default=10000)
ap.add_argument("--ef", type=int, default=640)
ap.add_argument("--resident", type=int, default=512)
ap.add_argument("--cache-mib", type=float, default=4.0)
args = ap.parse_args()

n, dim = bench.N31K, bench.DIM
INT8_ROW, F32_ROW = 256 * ((dim + 255) // 256) + 16, 4 * dim + 64
t0 = time.time()
base = bench.make_31k("clustered", 42, n)
Q = bench.make_31k("clustered", 43, args.nq)
g = O.hnsw_build_ex(base, O.COSINE, M=bench.M, ef_construction=bench.EFC, flags=O.BUILD_HEURISTIC, mode=O.MODE_FAST)
up = g.up_adj.reshape(-1, g.M)
lvl_count = {l: int((g.levels >= l).sum()) for l in range(1, g.max_level + 1)}
print("data + graph %.0f s: n=%d entry=%d max_level=%d, nodes of level >= l: %s" % (time.time() - t0, n, g.entry, g.max_level, lvl_count),
      flush=True)
norms = np.linalg.norm(base.astype(np.float64), axis=1).astype(np.float32)
unit = base / norms[:, None]


def descend(q, stop):
    """Greedy descent from the entry point through the layers above `stop`; returns the node reached at level `stop` + 1."""
    cur = g.entry
    curd = 1.0 - float(unit[cur] @ q)
    for level in range(g.max_level, stop, -1):
        improved = True
        while improved:
            improved = False
            a = up[g.up_off[cur] + level - 1]
            a = a[a >= 0]
            if len(a) == 0:
                break
            d = 1.0 - unit[a] @ q
            j = int(np.argmin(d))
            if d[j] < curd:
                cur, curd, improved = int(a[j]), float(d[j]), True
    return cur, curd


_traces = {}


def trace(qi):
    """Layer-0 best-first search at ef: per hop (fresh neighbour ids, admitted mask)."""
    if qi in _traces:
        return _traces[qi]
    q = Q[qi] / np.linalg.norm(Q[qi])
    cur, curd = descend(q, 0)
    vis = np.zeros(n, np.bool_)
    vis[cur] = True
    cand, near, hops = [(curd, cur)], [(-curd, cur)], []
    while cand:
        d0, c = heapq.heappop(cand)
        if len(near) >= args.ef and d0 > -near[0][0]:
            break
        a = g.l0_adj[c]
        a = a[a >= 0]
        a = a[~vis[a]]
        vis[a] = True
        if len(a) == 0:
            hops.append((a, np.zeros(0, np.bool_)))
            continue
        d = 1.0 - unit[a] @ q
        adm = np.zeros(len(a), np.bool_)
        for j in range(len(a)):
            if len(near) < args.ef or d[j] < -near[0][0]:
                adm[j] = True
                heapq.heappush(cand, (float(d[j]), int(a[j])))
                heapq.heappush(near, (-float(d[j]), int(a[j])))
                if len(near) > args.ef:
                    heapq.heappop(near)
        hops.append((a, adm))
    _traces[qi] = hops
    return hops


def simulate(share):
    """One XCD serving `share` (query indices in service order): bytes requested, bytes past the LRU cache, hops, evaluations."""
    cap = int(args.cache_mib * (1 << 20))
    lru, used = OrderedDict(), 0
    req = miss = hops = evals = 0
    todo = list(share)[::-1]
    live = []
    while todo or live:
        while todo and len(live) < args.resident:
            live.append([trace(todo.pop()), 0])
        for st in live:
            a, adm = st[0][st[1]]
            st[1] += 1
            hops += 1
            evals += len(a)
            for obj, size in [(int(v), INT8_ROW) for v in a] + [(n + int(v), F32_ROW) for v in a[adm]]:
                req += size
                if obj in lru:
                    lru.move_to_end(obj)
                else:
                    miss += size
                    lru[obj] = size
                    used += size
                    while used > cap:
                        used -= lru.popitem(last=False)[1]
        live = [st for st in live if st[1] < len(st[0])]
    return req, miss, hops, evals


def nearest(rows_unit, qs_unit):
    return np.argmax(qs_unit @ rows_unit.T, axis=1).astype(np.int64)


Qu = Q / np.linalg.norm(Q, axis=1, keepdims=True)


def keys_of(name):
    kind, _, arg = name.partition(":")
    if kind == "dealt":
        return None
    if kind == "centre":     # datagen's clustered set: the centres are the first 256 x dim gaussians of the seed's stream
        cen = datagen.JavaRandom(43).next_gaussians(256 * dim).reshape(256, dim)
        return nearest((cen / np.linalg.norm(cen, axis=1, keepdims=True)).astype(np.float32), Qu)
    if kind in ("pivot", "pivot8"):
        P = min(int(arg), n)
        rows = unit[np.arange(P) * (n // P)]
        if kind == "pivot8":     # int8 rows (scale max|v| / 127) against the exact query: the 16-bit query code's error is 1 / 128 of the row's
            rows = base[np.arange(P) * (n // P)]
            s = np.abs(rows).max(axis=1, keepdims=True) / 127.0
            rows = np.rint(rows / s) * s / norms[np.arange(P) * (n // P), None]
        return nearest(rows.astype(np.float32), Qu)
    if kind == "level":
        ids = np.nonzero(g.levels >= int(arg))[0]
        return ids[nearest(unit[ids], Qu)]
    if kind == "descent":
        return np.array([descend(Qu[i], int(arg) - 1)[0] for i in range(args.nq)], np.int64)
    raise SystemExit("unknown key %r" % name)


if args.key == "all":
    names = ["dealt", "centre", "pivot:256", "pivot8:256"]
    names += ["level:%d" % l for l in (6, 7, 8) if l <= g.max_level] + ["descent:%d" % l for l in (5, 7, 9) if l <= g.max_level]
else:
    names = args.key.split(",")

t0 = time.time()
_, _, stats, _ = O.hnsw_search(base, g, Q, bench.K, ef=args.ef, nthreads=min(16, os.cpu_count() or 1))
print("oracle search of the batch %.0f s: %.1f evaluations, %.1f hops per query" % (time.time() - t0, stats[:, 0].mean(), stats[:, 1].mean()),
      flush=True)
per8 = (args.nq + 7) // 8
print("order of the XCD's queries (%d simulated, %d resident, %.0f MiB LRU) | bins | MB per query requested | past L2 | hit rate | "
      "hops | evaluations per query | XCD load max / mean" % (args.sim, args.resident, args.cache_mib))
for name in names:
    t0 = time.time()
    k = keys_of(name)
    if k is None:
        shares = [np.arange(x, args.nq, 8) for x in range(8)]
        bins = 0
    else:
        order = np.argsort(k, kind="stable")
        shares = [order[x * per8:(x + 1) * per8] for x in range(8)]
        bins = len(np.unique(k))
    load = np.array([stats[s, 0].sum() for s in shares], np.float64)
    req, miss, hops, evals = simulate(shares[0][:args.sim])
    m = min(args.sim, len(shares[0]))
    print("%-12s | %4d | %.2f | %.2f | %.3f | %.0f | %.0f | %.4f   (%.0f s)" % (
        name, bins, req / m / 1e6, miss / m / 1e6, 1.0 - miss / req, hops / m, evals / m, load.max() / load.mean(), time.time() - t0), flush=True)
