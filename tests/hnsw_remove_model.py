"""numpy statement of what hnswgpu_hnsw_remove leaves of a graph, independent of the library -- the one specification of the
repair rule (include/hnswgpu.h).  The numbering is lsh_remove_model's (kept / rank); distances are oracle.c's bit-mimic of the
traversal's arithmetic (orc_dist_dev on cached device-order norms: what oracle.distance_dev computes).

A list of a kept node that loses no member keeps its members in their order under their new ids.  A list that loses one is
selected again from the OLD graph alone: the kept old members joined with the kept members of the same-layer lists of the
members that left, without the node itself, each once; ascending by (d(u, c), id); then the first min(w, C) (closest), or
get-neighbors-heuristic without extend-candidates (graph.clj:162-198 as prune-connections :208-232 uses it): a candidate is
taken unless it is closer to an already taken one than to u, until w are taken.  No back edges, no second hop."""
import ctypes as C

import numpy as np

import lsh_remove_model as LR


class Distances:
    """d(a, b) between rows of `base` by the device's arithmetic; the norms are computed once."""

    def __init__(self, O, base, metric):
        self.base = np.ascontiguousarray(base, np.float32)
        self.metric = int(metric)
        self.dim = self.base.shape[1]
        self._fn = O.lib().orc_dist_dev
        self._ptr = self.base.ctypes.data
        self._stride = self.base.strides[0]
        self.norms = [O.norm_dev(v) for v in self.base]
        self._memo = {}

    def __call__(self, a, b):
        """a is the left operand (the list's node, or the candidate against a taken row)."""
        key = (a, b)
        d = self._memo.get(key)
        if d is None:
            d = self._fn(self.metric, C.c_void_p(self._ptr + a * self._stride), C.c_void_p(self._ptr + b * self._stride), self.dim,
                         C.c_float(self.norms[a]), C.c_float(self.norms[b]))
            self._memo[key] = d
        return d


def old_list(g, v, lc):
    """Node v's members on layer lc of graph g in their order (without the -1 padding), or None where v is below lc."""
    if lc == 0:
        row = g.l0_adj.reshape(g.n, -1)[v]
    elif g.levels[v] >= lc:
        row = g.up_adj.reshape(-1, g.M)[g.up_off[v] + lc - 1]
    else:
        return None
    return [int(x) for x in row if x >= 0]


def candidates(g, keep, u, lc):
    """(kept members, members that left, the candidate set) of u's list on layer lc."""
    members = old_list(g, u, lc)
    stay = [x for x in members if keep[x]]
    left = [x for x in members if not keep[x]]
    cand = set(x for x in stay if x != u)
    for v in left:
        cand.update(x for x in (old_list(g, v, lc) or []) if x != u and keep[x])
    return stay, left, cand


def select(d, u, cand, w, heuristic):
    """The repaired list of u from its candidate set, OLD ids in selection order."""
    order = sorted(cand, key=lambda c: (d(u, c), c))
    if not heuristic:
        return order[:w]
    res = []
    for c in order:
        if len(res) >= w:
            break
        dc = d(u, c)
        if any(d(c, r) < dc for r in res):
            continue
        res.append(c)
    return res


def remove(O, base, metric, g, rows, heuristic, repair=True, d=None):
    """The oracle.Graph hnswgpu_hnsw_remove(rows) leaves of graph g over `base`.  heuristic: the handle's builder carries
    HNSWGPU_BUILD_HEURISTIC.  repair=False: the graph merely compacted -- every list keeps its kept members and nothing else.
    d: a Distances over `base` to share between calls."""
    n0, M, M0 = g.n, g.M, g.M0
    keep = np.ones(n0, np.bool_)
    keep[np.asarray(rows, np.int64).reshape(-1)] = False
    kept, new_id = LR.kept(n0, rows), LR.rank(n0, rows)
    n1 = len(kept)
    if d is None and repair:
        d = Distances(O, base, metric)
    levels = g.levels[kept].astype(np.int32)
    up_off = np.zeros(n1 + 1, np.int64)
    up_off[1:] = np.cumsum(levels)
    l0 = np.full((n1, M0), -1, np.int32)
    up = np.full((int(up_off[n1]), M), -1, np.int32)
    for u in kept:
        u = int(u)
        for lc in range(int(g.levels[u]) + 1):
            w = M0 if lc == 0 else M
            stay, left, cand = candidates(g, keep, u, lc)
            out = select(d, u, cand, w, heuristic) if (left and repair) else stay
            dst = l0[new_id[u]] if lc == 0 else up[up_off[new_id[u]] + lc - 1]
            dst[:len(out)] = new_id[out]
    if n1 == 0:
        entry, top = -1, 0
    elif keep[g.entry]:
        entry, top = int(new_id[g.entry]), g.max_level
    else:
        entry = int(np.argmax(levels))            # the first of the highest: the lowest old id among equals
        top = int(levels[entry])
    return O.Graph(levels, l0, up_off, up.reshape(-1), M, entry, top)
