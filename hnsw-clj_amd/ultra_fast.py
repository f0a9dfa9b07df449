"""Mirror of ``hnsw.ultra-fast`` (src/hnsw/ultra_fast.clj) -- also the engine behind
``hnsw.ultra-optimized`` (src/hnsw/wip/ultra_optimized.clj:124-138,282-286 delegate here).

Same names and argument meaning: ``build_index(data, M=16, ef_construction=200, distance_fn=...)``
takes a seq of ``[id, vector]`` pairs; ``search_knn(graph, query_vec, k)`` returns a list of
``{"id", "distance"}`` ascending, ``[]`` on an empty index, fewer than k when the index is smaller.
The vectors live in HBM as one float32 matrix; traversal runs in the HIP kernel.
"""
import numpy as np

from . import engine
from .engine import COSINE, L2


def cosine_distance_ultra(v1, v2, device=0):
    """ultra_fast.clj:53-95"""
    return engine.pair_distance(COSINE, v1, v2, device)


cosine_distance_ultra.metric = COSINE


def euclidean_distance_ultra(v1, v2, device=0):
    """ultra_fast.clj:43-51 (rooted)"""
    return engine.pair_distance(L2, v1, v2, device)


euclidean_distance_ultra.metric = L2


class UltraGraph:
    """What ultra_fast.clj:104-111's UltraGraph record becomes: the String-id table stays on the host,
    vectors + adjacency live on the device behind ``index``."""

    def __init__(self, index, ids, M, ef_construction, distance_fn):
        self.index = index
        self.ids = ids
        self.M = M
        self.max_M = 2 * M
        self.ef_construction = ef_construction
        self.distance_fn = distance_fn

    def close(self):
        if self.index is not None:
            self.index.close()


def _metric_of(distance_fn):
    m = getattr(distance_fn, "metric", None)
    if m is None:
        raise ValueError(
            ":distance-fn must be one of the engine's metric functions (cosine_distance_ultra, "
            "euclidean_distance_ultra, simd_optimized.cosine_distance/euclidean_distance/dot_product): an arbitrary "
            "host function cannot be evaluated inside the GPU traversal")
    return m


def _split(data):
    ids, vecs = [], []
    for item in data:
        i, v = item  # the reference destructures [id vector] (ultra_fast.clj:318)
        ids.append(i)
        vecs.append(np.asarray(v, dtype=np.float32))
    if vecs:
        dim = len(vecs[0])
        for v in vecs:
            if len(v) != dim:
                raise ValueError("vectors differ in length")
        base = np.stack(vecs).astype(np.float32, copy=False)
    else:
        base = np.zeros((0, 1), np.float32)
    return ids, base


def build_index(data, M=16, ef_construction=200, distance_fn=cosine_distance_ultra, show_progress=True, seed=42,
                device=0, graph=None, sequential=False, heuristic=False, symmetric=False, extend=False):
    """ultra_fast.clj:334-344.  ``graph`` (an engine.Graph) uploads an adjacency built elsewhere instead
    of building one on the device.  ``sequential`` = insert-single's own order and start level (:216-275; slow, the
    parity mode); ``heuristic`` / ``symmetric`` / ``extend`` = the neighbour selection of src/hnsw/graph.clj:162-232
    (what ``pure_hnsw.build_index`` asks for)."""
    metric = _metric_of(distance_fn)
    ids, base = _split(data)
    if show_progress:
        print("Inserting %d elements..." % len(ids))
    idx = engine.Index(base, metric, device)
    if graph is not None:
        idx.set_graph(graph)
    else:
        idx.hnsw_build(M, ef_construction, seed, sequential=sequential, heuristic=heuristic, symmetric=symmetric, extend=extend)
    return UltraGraph(idx, ids, M, ef_construction, distance_fn)


def remove_vectors(graph, ids):
    """The reference has no delete (pure_hnsw.clj:16 is a todo); the rule is the engine's own (hnswgpu_hnsw_remove): ``ids`` are
    the caller's ids, the form ``graph.ids`` holds; their vectors leave the base and the graph, a neighbour list that loses a
    member is selected again from its kept members and those of the members that left, and ``graph.ids`` follows.  An unknown
    id raises KeyError before the device is touched; an id of several rows removes them all.  Empty ``ids`` does nothing.
    Returns the graph."""
    ids = list(ids)
    if not ids:
        return graph
    rows_of = {}
    for row, i in enumerate(graph.ids):
        rows_of.setdefault(i, []).append(row)
    rows = []
    for i in ids:
        if i not in rows_of:
            raise KeyError(i)
        rows.extend(rows_of[i])
    kept = graph.index.hnsw_remove(np.asarray(rows, np.int32))
    graph.ids = [graph.ids[i] for i in kept]
    graph.__dict__.pop("_route", None)       # (routed_to_exact_scan's measurements were of the graph that was)
    return graph


def update_vectors(graph, data):
    """"Update existing vectors" (the open item of the reference's to-do list); the rule is the engine's own
    (hnswgpu_hnsw_update): ``data`` has the form ``build_index`` takes; the vector stored under each id takes the new values and
    keeps its id and its level -- it is unlinked as a removed vector is and inserted again as an added one, with the graph's
    ``ef_construction`` -- so ``graph.ids`` is unchanged.  An unknown id raises KeyError, an id that names several rows or
    appears twice in ``data`` raises ValueError, both before the device is touched.  Empty ``data`` does nothing.  Returns
    the graph."""
    ids, rows = _split(data)
    if not ids:
        return graph
    rows_of = {}
    for row, i in enumerate(graph.ids):
        rows_of.setdefault(i, []).append(row)
    at, seen = [], set()
    for i in ids:
        if i not in rows_of:
            raise KeyError(i)
        if len(rows_of[i]) > 1:
            raise ValueError("id %r names %d rows of the index" % (i, len(rows_of[i])))
        if i in seen:
            raise ValueError("id %r appears twice: two values for one vector have no winner" % (i,))
        seen.add(i)
        at.append(rows_of[i][0])
    graph.index.hnsw_update(np.asarray(at, np.int32), rows, graph.ef_construction)
    graph.__dict__.pop("_route", None)       # (routed_to_exact_scan's measurements were of the graph that was)
    return graph


def _format(graph, ids_row, d_row):
    return [{"id": graph.ids[i], "distance": float(d)} for i, d in zip(ids_row, d_row) if i >= 0]


def search_knn(graph, query_vec, k, ef=None):
    """ultra_fast.clj:346-374; ef defaults to (max k 50) (:355)."""
    if graph.index.n == 0:
        return []
    ids, d = graph.index.hnsw_search(query_vec, int(k), ef or 0)
    return _format(graph, ids[0], d[0])


def routed_to_exact_scan(graph, queries, k, ef=None):
    """The crossover rule of ``search_batch(route=True)``: the traversal evaluates E(ef) rows per query, gathered at random;
    the exact scan (hnswgpu_exact_knn: every row once per batch, through the matrix cores) answers at recall 1.0 -- it is the
    cheaper way to at least the same recall once E(ef) >= n / 3 (31k x 768 on one MI355X: 1.5M QPS exact against 0.78M
    through the graph at ef 640, 90k at ef 3200; bench.py: by_distribution.*.routed_qps).  E(ef) is measured once per
    (graph, k, ef) on up to 32 of the queries."""
    key = (int(k), int(ef or 0))
    cache = graph.__dict__.setdefault("_route", {})
    if key not in cache:
        _, _, st = graph.index.hnsw_search(np.asarray(queries, np.float32)[:32], int(k), ef or 0, want_stats=True)
        cache[key] = float(st[:, 0].mean()) >= graph.index.n / 3.0
    return cache[key]


def search_batch(graph, queries, k, ef=None, route=False):
    """All queries in ONE launch: the seam of BatchSearchIndex/search-batch* (api/protocol.clj:58-67).  ``route=True`` (not
    in the reference) answers by the exact scan where that is cheaper than the traversal at this ef (routed_to_exact_scan):
    the neighbours are then the exact ones -- at least as good as the graph's, not necessarily the same."""
    queries = np.asarray(queries, np.float32)
    if len(queries) == 0:
        return []
    if graph.index.n == 0:
        return [[] for _ in queries]
    if route and routed_to_exact_scan(graph, queries, k, ef):
        ids, d = graph.index.exact_knn(queries, int(k))
    else:
        ids, d = graph.index.hnsw_search(queries, int(k), ef or 0)
    return [_format(graph, ids[i], d[i]) for i in range(len(queries))]


def filtered_plan(n, p, k, ef=None):
    """How a filtered search over n rows, p of them passing, is served: ``("scan" | "graph", ef')`` -- a pure function of
    counts the reference and the engine already fix.  The reference over-fetches by 3 (protocol.clj:101), and a result list
    must hold 3k * n / p entries to expect 3k passing ones: ef_need = ceil(3 k n / p), ef' = max(ef or max(k, 50), ef_need).
    The exact scan of the passing rows serves the call when nothing passes, when ef_need exceeds the 1024 list entries the
    filtered traversal looks at, or when p <= ef' (the scan then evaluates no more rows than the list alone holds);
    otherwise the graph is walked at ef'."""
    n, p, k = int(n), int(p), int(k)
    ef0 = int(ef) if ef else max(k, 50)
    if p <= 0:
        return "scan", ef0
    ef_need = -(-3 * k * n // p)
    ef2 = max(ef0, ef_need)
    if ef_need > 1024 or p <= ef2:
        return "scan", ef2
    return "graph", ef2


def _allow_bits(graph, filter_fn):
    """The predicate on the caller's ids, evaluated once per row on the host (or a ready bool array of length n)."""
    if callable(filter_fn):
        return np.fromiter((bool(filter_fn(i)) for i in graph.ids), np.bool_, len(graph.ids))
    bits = np.asarray(filter_fn)
    if bits.dtype != np.bool_ or bits.shape != (graph.index.n,):
        raise ValueError("filter_fn must be a predicate on ids or a bool array with one entry per row")
    return bits


def search_batch_filtered(graph, queries, k, filter_fn, ef=None):
    """FilterableIndex/search-knn-filtered* (api/protocol.clj:34-41) for a batch, one predicate per call: ``filter_fn`` is
    called once per row with ``graph.ids[i]`` (or is a bool array of length n).  filtered_plan chooses the path: "graph"
    walks the graph at ef' and keeps the first k passing entries of each result list (protocol.clj:97-102 with a list
    long enough to expect 3k passing entries); "scan" (not in the reference) evaluates exactly the passing rows -- the
    neighbours are then the EXACT k nearest passing rows, at least as good as the graph's, not necessarily the same."""
    queries = np.asarray(queries, np.float32)
    if queries.ndim == 1:
        queries = queries[None, :]
    if len(queries) == 0:
        return []
    n = graph.index.n
    if n == 0:
        return [[] for _ in queries]
    bits = _allow_bits(graph, filter_fn)
    plan, ef2 = filtered_plan(n, int(bits.sum()), k, ef)
    mask = engine.pack_mask(bits, n)
    if plan == "scan":
        ids, d = graph.index.exact_knn_filtered(queries, int(k), mask)
    else:
        ids, d = graph.index.hnsw_search_filtered(queries, int(k), mask, ef2)
    return [_format(graph, ids[i], d[i]) for i in range(len(queries))]


def search_batch_filtered_each(graph, queries, k, filter_fns, ef=None):
    """search_batch_filtered with one predicate (or bool array) PER QUERY -- the reference's many threads, each with one
    query and its own filter-fn, as one batch: row q equals ``search_knn_filtered(graph, queries[q], k, filter_fns[q], ef)``.
    The same object, or equal bits, is evaluated and packed once.  filtered_plan is applied per query: the "scan" queries go
    in one exact_knn_filtered_each call, ordered so that equal masks are adjacent (a query group then shares its rows), the
    "graph" queries in one hnsw_search_filtered_each call per distinct ef' (never rounded); the original order is restored.
    A batch whose filters are all one mask takes search_batch_filtered's single-mask call."""
    queries = np.asarray(queries, np.float32)
    if queries.ndim == 1:
        queries = queries[None, :]
    if len(filter_fns) != len(queries):
        raise ValueError("one filter per query: %d filters for %d queries" % (len(filter_fns), len(queries)))
    if len(queries) == 0:
        return []
    n = graph.index.n
    if n == 0:
        return [[] for _ in queries]
    masks, by_obj, by_bits, which = [], {}, {}, []   # distinct masks: (bits, packed, p)
    for f in filter_fns:
        m = by_obj.get(id(f))
        if m is None:
            bits = _allow_bits(graph, f)
            key = bits.tobytes()
            m = by_bits.get(key)
            if m is None:
                m = by_bits[key] = len(masks)
                masks.append((bits, engine.pack_mask(bits, n), int(bits.sum())))
            by_obj[id(f)] = m
        which.append(m)
    if len(masks) == 1:
        return search_batch_filtered(graph, queries, k, masks[0][0], ef)
    plans = [filtered_plan(n, p, k, ef) for _, _, p in masks]
    calls = {}                                       # ("scan",) or ("graph", ef') -> query numbers
    for q, m in enumerate(which):
        plan, ef2 = plans[m]
        calls.setdefault(("scan",) if plan == "scan" else ("graph", ef2), []).append(q)
    ids = np.empty((len(queries), int(k)), np.int32)
    d = np.empty((len(queries), int(k)), np.float32)
    for key, qs in sorted(calls.items()):
        qs = sorted(qs, key=lambda q: (which[q], q))  # equal masks adjacent
        rows = np.stack([masks[which[q]][1] for q in qs])
        if key[0] == "scan":
            gi, gd = graph.index.exact_knn_filtered_each(queries[qs], int(k), rows)
        else:
            gi, gd = graph.index.hnsw_search_filtered_each(queries[qs], int(k), rows, key[1])
        ids[qs], d[qs] = gi, gd
    return [_format(graph, ids[i], d[i]) for i in range(len(queries))]


def search_knn_filtered(graph, query_vec, k, filter_fn, ef=None):
    """search_batch_filtered for one query: a list of ``{"id", "distance"}`` ascending, fewer than k when fewer pass."""
    if graph.index.n == 0:
        return []
    return search_batch_filtered(graph, np.asarray(query_vec, np.float32)[None, :], k, filter_fn, ef)[0]


def graph_info(graph):
    """ultra_fast.clj:378-384"""
    g = graph.index.get_graph() if graph.index.n else None
    return {"num-elements": graph.index.n, "entry-point": graph.ids[g.entry] if g is not None else None,
            "M": graph.M, "ef-construction": graph.ef_construction}
