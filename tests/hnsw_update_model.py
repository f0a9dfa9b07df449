"""numpy statement of what hnswgpu_hnsw_update leaves of a graph, independent of the library -- the one specification of the
rule (include/hnswgpu.h).  Let U be the ids of a call.

UNLINK is hnswgpu_hnsw_remove's repair (hnsw_remove_model: candidates / select) with U as the rows that left and nothing
renumbered: a list of a node outside U that holds no member of U stays, a list that holds one is selected again from the OLD
graph alone, every list of a row of U becomes empty.

RE-INSERT restates the batched insertion (hnsw.hip: insert_batches; oracle.c: orc_hnsw_build_batched is the project's own
statement of that loop, but draws levels by position and so cannot be called for ids that are not the last) for GIVEN ids and
GIVEN levels: per batch every row is searched against the graph as it stood when the batch began -- ef 1 from the top down to
layer 1, the single nearest node of each layer min(level, top) .. 1 kept, then ef_construction at layer 0 --, the batch is
linked in row order (a row's layers top down, a layer's links in selection order: own link, then reverse link), over-full lists
are pruned as the builder prunes, and entry point and top move behind the batch.  The batch sizes are
hnsw_build_model.batch_schedule(n, n - m).

Distances are oracle.c's bit-mimic of the traversal's arithmetic (orc_dist_dev on device-order norms: hnsw_remove_model's
Distances, what oracle.distance_dev computes)."""
import heapq

import numpy as np

import hnsw_build_model as B
import hnsw_remove_model as R

SEL_MAX_CAND = 4096          # build_kernels.hpp: kSelMaxCand

# counters of update()
REPAIRED_UPPER, EMPTIED_THEN_LINKED, PRUNED, BATCHES, ENTRY_IN_U, ENTRY_TAKEN_BACK = range(6)


def unlink(g, d, ids, heuristic, counters=None):
    """(l0, up): the lists of graph g after step 1, under the old ids.  d: Distances over the old OR the new base -- no row of U
    takes part in any distance of this step."""
    keep = np.ones(g.n, np.bool_)
    keep[np.asarray(ids, np.int64).reshape(-1)] = False
    l0 = [[] for _ in range(g.n)]
    up = [[] for _ in range(int(g.up_off[g.n]))]
    for u in range(g.n):
        if not keep[u]:
            continue
        for lc in range(int(g.levels[u]) + 1):
            w = g.M0 if lc == 0 else g.M
            stay, left, cand = R.candidates(g, keep, u, lc)
            out = R.select(d, u, cand, w, heuristic) if left else stay
            if left and lc > 0 and counters is not None:
                counters[REPAIRED_UPPER] += 1
            if lc == 0:
                l0[u] = list(out)
            else:
                up[int(g.up_off[u]) + lc - 1] = list(out)
    return l0, up


class _Lists:
    """HostGraph (hnsw.hip): every list as [(stored edge distance, id)] in its order.  Adopted from the unlinked graph with
    d(owner, neighbour), as hnswgpu_hnsw_add adopts an installed graph."""

    def __init__(self, g, l0, up, d):
        self.g = g
        self.l0 = [[(d(u, x), x) for x in lst] for u, lst in enumerate(l0)]
        owner = np.repeat(np.arange(g.n), g.levels)
        self.up = [[(d(int(owner[b]), x), x) for x in lst] for b, lst in enumerate(up)]

    def at(self, node, lc):
        if lc == 0:
            return self.l0[node], self.g.M0
        return self.up[int(self.g.up_off[node]) + lc - 1], self.g.M

    def ids(self, node, lc):
        return [x for _, x in self.at(node, lc)[0]]

    def add_edge(self, frm, to, lc, dist):
        """HostGraph::add_edge: a duplicate is ignored; an over-full list keeps its m closest by a stable sort on the stored
        distances.  True if the list was pruned."""
        lst, m = self.at(frm, lc)
        if any(x == to for _, x in lst):
            return False
        lst.append((dist, to))
        if len(lst) <= m:
            return False
        order = sorted(range(len(lst)), key=lambda i: (lst[i][0], i))
        lst[:] = [lst[i] for i in order[:m]]
        return True

    def append_edge(self, frm, to, lc, dist):
        """HostGraph::append_edge: False = the list is full, the edge is pending."""
        lst, m = self.at(frm, lc)
        if any(x == to for _, x in lst):
            return True
        if len(lst) >= m:
            return False
        lst.append((dist, to))
        return True

    def remove_edge(self, frm, to, lc):
        lst, _ = self.at(frm, lc)
        for i, (_, x) in enumerate(lst):
            if x == to:
                del lst[i]
                return True
        return False


def search_layer(lists, levels, d, q, ep, ep_d, ef, lc):
    """search-layer-ultra as oracle.c restates it: expand iff |nearest| < ef or c.dist <= worst, admit iff |nearest| < ef or
    d < worst; neighbours in list order; ties by admission order.  Returns [(dist, id)] ascending by (dist, admission)."""
    if ep_d is None:
        ep_d = d(q, ep)
    seq = 1
    visited = {ep}
    cand = [(ep_d, 0, ep)]                       # min-heap
    near = [(-ep_d, 0, ep)]                      # max-heap by (dist, seq): keys negated
    while cand:
        cd, _, cur = heapq.heappop(cand)
        worst = -near[0][0] if near else float("inf")
        if not (len(near) < ef or cd <= worst):
            continue
        if levels[cur] < lc:
            continue
        for nb in lists.ids(cur, lc):
            if nb in visited:
                continue
            visited.add(nb)
            dn = d(q, nb)
            w = -near[0][0] if near else float("inf")
            if len(near) < ef or dn < w:
                heapq.heappush(cand, (dn, seq, nb))
                heapq.heappush(near, (-dn, -seq, nb))
                seq += 1
                if len(near) > ef:
                    heapq.heappop(near)
    return sorted(((-nd, -ns, x) for nd, ns, x in near))


def select_heuristic(d, cand, m, extend):
    """get-neighbors-heuristic (graph.clj:162-198): cand [(dist, id)]; ascending by (dist, id); a candidate is taken unless it is
    closer to an already taken one than to the base node, until m are taken; extend: the discarded ones fill up in their order."""
    res, disc = [], []
    for dc, c in sorted(cand):
        if len(res) >= m:
            break
        if any(d(c, r) < dc for _, r in res):
            disc.append((dc, c))
        else:
            res.append((dc, c))
    if extend:
        res.extend(disc[:max(0, m - len(res))])
    return res


def update(O, new_base, metric, g, ids, efc, flags=0, d=None, max_batch=B.DEFAULT_MAX_BATCH):
    """(graph, counters): the oracle.Graph hnswgpu_hnsw_update(ids, rows) leaves of graph g when `new_base` is the base with the
    new values in place.  flags: the oracle's BUILD_* bits of the handle's builder (0: closest-m, a graph from set_graph).
    d: a Distances over new_base to share."""
    heur = bool(flags & O.BUILD_HEURISTIC)
    sym = heur and bool(flags & O.BUILD_SYMMETRIC)
    extend = bool(flags & O.BUILD_EXTEND)
    n, M, M0 = g.n, g.M, g.M0
    uid = sorted(int(x) for x in np.asarray(ids).reshape(-1))
    assert len(set(uid)) == len(uid) and (not uid or (uid[0] >= 0 and uid[-1] < n))
    m = len(uid)
    counters = [0] * 6
    if d is None:
        d = R.Distances(O, new_base, metric)
    levels = [int(x) for x in g.levels]
    in_u = np.zeros(n, np.bool_)
    in_u[uid] = True
    # ---- 1. unlink, 2. values (d is over the new base)
    l0, up = unlink(g, d, uid, heur, counters)
    emptied = set()
    for u in range(n):
        if in_u[u]:
            continue
        for lc in range(levels[u] + 1):
            had = R.old_list(g, u, lc)
            now = l0[u] if lc == 0 else up[int(g.up_off[u]) + lc - 1]
            if had and not now:
                emptied.add((u, lc))
    L = _Lists(g, l0, up, d)
    # ---- 3. the entry point the insertion starts from
    entry, top = int(g.entry), int(g.max_level)
    todo = list(uid)
    if m == n:
        entry, top = uid[0], levels[uid[0]]
        todo = uid[1:]
    elif in_u[entry]:
        counters[ENTRY_IN_U] += 1
        outside = [u for u in range(n) if not in_u[u]]
        entry = max(outside, key=lambda u: (levels[u], -u))
        top = levels[entry]
    # ---- 4. re-insert
    done = n - len(todo)
    pos = 0
    for bsz in B.batch_schedule(n, done, max_batch):
        batch = todo[pos:pos + bsz]
        pos += bsz
        counters[BATCHES] += 1
        top_at_start = top
        found = []
        for q in batch:                         # phase 1: the searches, against the graph as the batch found it
            ep, epd = entry, None
            upl = {}
            for lc in range(top, 0, -1):
                res = search_layer(L, levels, d, q, ep, epd, 1, lc)
                if res:
                    epd, _, ep = res[0]
                if lc <= levels[q]:
                    upl[lc] = (ep if res else -1, epd)
            res = search_layer(L, levels, d, q, ep, epd, efc, 0)
            cands = [(dd, x) for dd, _, x in res]
            sel = select_heuristic(d, cands, M0, extend) if heur else cands[:M0]
            found.append((upl, sel))
        pend = []                                # phase 2: link in row order
        seq = 0
        for q, (upl, sel) in zip(batch, found):
            for lc in range(min(levels[q], top_at_start), -1, -1):
                links = sel if lc == 0 else [(upl[lc][1], upl[lc][0])]
                for dist, nb in links:
                    seq += 1
                    if nb < 0 or nb == q:
                        continue
                    L.add_edge(q, nb, lc, dist)
                    if (nb, lc) in emptied:      # a list the unlink left empty receives a reverse edge
                        counters[EMPTIED_THEN_LINKED] += 1
                    if not heur:
                        if L.add_edge(nb, q, lc, dist):
                            counters[PRUNED] += 1
                    elif not L.append_edge(nb, q, lc, dist):
                        pend.append((nb, lc, seq, dist, q))
        if heur and pend:                        # Pruner::run_batched
            pend.sort()
            removals = []
            i = 0
            while i < len(pend):
                j = i
                while j < len(pend) and pend[j][:2] == pend[i][:2]:
                    j += 1
                target, lc = pend[i][:2]
                lst, w = L.at(target, lc)
                tc = sorted(lst + [(p[3], p[4]) for p in pend[i:j]])[:SEL_MAX_CAND]
                counters[PRUNED] += 1
                keep = select_heuristic(d, tc, w, False)
                if sym:
                    kept = set(x for _, x in keep)
                    removals.extend((x, target, lc) for _, x in tc if x not in kept)
                lst[:] = keep
                i = j
            for frm, to, lc in removals:
                L.remove_edge(frm, to, lc)
        for q in batch:                          # entry point and top: only now, row by row
            if levels[q] > top:
                if in_u[int(g.entry)] and m != n:
                    counters[ENTRY_TAKEN_BACK] += 1
                entry, top = q, levels[q]
        done += len(batch)
    assert pos == len(todo) and done == n
    out0 = np.full((n, M0), -1, np.int32)
    for u in range(n):
        x = L.ids(u, 0)
        out0[u, :len(x)] = x
    outu = np.full((int(g.up_off[n]), M), -1, np.int32)
    for b, lst in enumerate(L.up):
        outu[b, :len(lst)] = [x for _, x in lst]
    return O.Graph(g.levels.copy(), out0, g.up_off.copy(), outu.reshape(-1), M, entry, max(top, 0)), counters


# ---- the data of the GPU tests (test_hnsw_update_gpu.py), with the conditions test_hnsw_update_host.py asserts of them -------------
N0, M, EFC, SEED = 600 + 7, 8, 48, 42      # test_hnsw_remove_gpu.py's shapes: 607 rows, 19 mask words, the last of 31 rows
DIMS = [40, 1100]
_ROWS = {}


def rows(O, dim):
    """(base f32 [N0, dim], pool f32 [300, dim], queries f32 [32, dim]): hnsw_build_model.paths_data (10 clusters whose centres are
    rows, 20 duplicated pairs (100 + i, 300 + i)) + 7 rows of the same clusters, one of them equal to row 41; `pool` holds new
    values of the same clusters, all distinct and none equal to a row of base; made once per dim."""
    if dim not in _ROWS:
        base = B.paths_data(O, dim)
        rs = np.random.RandomState(7 + dim)
        more = base[rs.randint(0, len(base), 7 + 300 + 32)] + 0.2 * rs.randn(7 + 300 + 32, dim).astype(np.float32)
        more[5] = base[41]                                   # one more duplicated pair, across the 600-row border
        parts = (np.concatenate([base, more[:7]]), more[7:307], more[307:])
        _ROWS[dim] = tuple(np.ascontiguousarray(p, np.float32) for p in parts)
    return _ROWS[dim]


def main_ids(g):
    """About 150 ids, unsorted: the last row, the entry point and every other row of the top level (so a re-inserted row takes the
    entry back), rows 100 .. 104 of the duplicated pairs (their twins 300 .. 304 stay outside), never row 7 (new_values)."""
    n = g.n
    must = sorted(set([n - 1, int(g.entry)] + [int(x) for x in np.flatnonzero(g.levels == g.max_level)] + list(range(100, 105))))
    free = np.setdiff1d(np.arange(n), must + [7] + list(range(300, 305)))
    rest = np.random.default_rng(31).choice(free, 150 - len(must), replace=False)
    ids = np.concatenate([rest[:70], must, rest[70:]]).astype(np.int32)
    return ids


def new_values(base, pool, ids):
    """(rows for `ids` in their order, the base with them in place): pool rows, and one new value equal to row 7, a row outside U
    that equals no other row."""
    assert len(ids) <= len(pool) and 7 not in ids
    vals = np.ascontiguousarray(pool[:len(ids)]).copy()
    vals[len(ids) // 2] = base[7]
    out = base.copy()
    out[np.asarray(ids)] = vals
    return vals, out
