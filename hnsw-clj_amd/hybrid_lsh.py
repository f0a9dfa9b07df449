"""Mirror of ``hnsw.ann.hash.hybrid-lsh`` (src/hnsw/ann/hash/hybrid_lsh.clj).

``build_lsh_index(data, distance_fn=...)`` draws the reference's hyperplanes (``Random(42)``, 8 tables of 64 Gaussian rows
of which the first 12 form the bucket id), hashes every row on the device and files it in its buckets;
``search_hybrid`` / ``search_hybrid_multiprobe`` / ``search_knn(index, q, k[, mode])`` probe the query's buckets and their
one-bit neighbours with the HIP bucket scan (hnswgpu_lsh_search).  Queries may be one vector or a batch.
``search_knn_filtered`` / ``search_batch_filtered`` / ``search_batch_filtered_each`` (not in the reference, whose index is served
by the protocol's post-filter) carry a predicate on the ids into the bucket scan as an allow-mask (hnswgpu_lsh_search_filtered).
``add_vectors`` / ``remove_vectors`` / ``update_vectors`` (not in the reference either) change a live index on the device
(hnswgpu_lsh_add / hnswgpu_lsh_remove / hnswgpu_lsh_update).

One difference, on purpose: the reference computes cosine whatever ``:distance-fn`` says (its ``query-norm`` is never nil,
:157-166); here the index's metric decides, as in every other mirror.
"""
import numpy as np

from . import engine
from .ultra_fast import _metric_of, _split, cosine_distance_ultra

# hybrid_lsh.clj:12-14, :80
NUM_HASH_TABLES = 8
NUM_HASH_BITS = 12
PROJECTION_DIM = 64
SEED = 42

# hybrid_lsh.clj:350-364: mode -> (num_probes, probe_radius); anything else is :balanced
MODE_CONFIGS = {
    "turbo": (2, 1),
    "fast": (4, 1),
    "balanced": (6, 2),
    "accurate": (8, 3),
    "precise": (8, 4),
}
DEFAULT_MODE = "balanced"


def mode_config(mode=None):
    """(num_probes, probe_radius) of a mode keyword; an unknown mode (and none) is :balanced (:363-364)."""
    return MODE_CONFIGS.get(mode, MODE_CONFIGS[DEFAULT_MODE])


def clamp_probes(num_probes, probe_radius, tables=NUM_HASH_TABLES, bits=NUM_HASH_BITS):
    """What a search probes: min(num-probes, tables) tables (:269), min(probe-radius, bits) flipped bits each (:321)."""
    return min(int(num_probes), int(tables)), min(int(probe_radius), int(bits))


class HybridIndex:
    """hybrid_lsh.clj:18-22: hash tables, matrices, rows and norms live on the device behind ``index``."""

    def __init__(self, index, ids, distance_fn):
        self.index = index
        self.ids = ids
        self.distance_fn = distance_fn

    def close(self):
        self.index.close()


def build_lsh_index(data, distance_fn=cosine_distance_ultra, show_progress=True, num_threads=8, device=0):
    """hybrid_lsh.clj:66-145 (``num_threads`` is the reference's pool size: the device hashes every row in one launch)"""
    metric = _metric_of(distance_fn)
    ids, base = _split(data)
    idx = engine.Index(base, metric, device)
    idx.lsh_build(NUM_HASH_TABLES, NUM_HASH_BITS, PROJECTION_DIM, SEED)
    if show_progress:
        print("LSH index built: %d vectors, %d hash tables, %d buckets per table" % (len(ids), NUM_HASH_TABLES, 1 << NUM_HASH_BITS))
    return HybridIndex(idx, ids, distance_fn)


def build_index(data, **opts):
    """hybrid_lsh.clj:345-348"""
    return build_lsh_index(data, **opts)


def add_vectors(index, data):
    """The reference's hybrid-lsh index has no add (build-lsh-index returns an immutable record); what is restated is its
    bucket order (hybrid_lsh.clj:105-129: a bucket lists its rows in insertion order): ``data`` has the form ``build_index``
    takes; every vector is hashed under the index's hyperplanes and joins its bucket of every table behind the bucket's
    present members (hnswgpu_lsh_add).  Empty ``data`` does nothing.  Returns the index."""
    ids, rows = _split(data)
    if ids:
        index.index.lsh_add(rows)
        index.ids.extend(ids)
    return index


def remove_vectors(index, ids):
    """The reference's hybrid-lsh index has no remove either (build-lsh-index returns an immutable record); what is restated
    is its bucket order (hybrid_lsh.clj:105-129: a bucket lists its rows in insertion order): ``ids`` are the caller's ids, the
    form ``index.ids`` holds; their vectors leave the base and every table's buckets, the kept members of a bucket stay in
    their order (hnswgpu_lsh_remove), and ``index.ids`` follows.  An unknown id raises KeyError before the device is touched;
    an id of several rows removes them all.  Empty ``ids`` does nothing.  Returns the index."""
    ids = list(ids)
    if not ids:
        return index
    rows_of = {}
    for row, i in enumerate(index.ids):
        rows_of.setdefault(i, []).append(row)
    rows = []
    for i in ids:
        if i not in rows_of:
            raise KeyError(i)
        rows.extend(rows_of[i])
    kept = index.index.lsh_remove(np.asarray(rows, np.int32))
    index.ids = [index.ids[i] for i in kept]
    return index


def update_vectors(index, data):
    """"Update existing vectors" (the open item of the reference's to-do list; its hybrid-lsh index is an immutable record):
    ``data`` has the form ``build_index`` takes; the vector stored under each id takes the new values, is hashed again under
    the index's hyperplanes and, in every table where its code changed, moves to its new bucket at the place its row gives it
    (hnswgpu_lsh_update).  It keeps its id: ``index.ids`` is unchanged.  An unknown id raises KeyError, an id that names
    several rows or appears twice in ``data`` raises ValueError, both before the device is touched.  Empty ``data`` does
    nothing.  Returns the index."""
    ids, rows = _split(data)
    if not ids:
        return index
    rows_of = {}
    for row, i in enumerate(index.ids):
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
    index.index.lsh_update(np.asarray(at, np.int32), rows)
    return index


def _format(index, ids_row, d_row):
    return [{"id": index.ids[i], "distance": float(d)} for i, d in zip(ids_row, d_row) if i >= 0]


def _search(index, query_vec, k, num_probes, probe_radius, take_main, take_flip):
    q = np.asarray(query_vec, np.float32)
    single = q.ndim == 1
    Q = q[None, :] if single else q
    if index.index.n == 0 or len(Q) == 0:
        out = [[] for _ in range(len(Q))]
    else:
        ids, d = index.index.lsh_search(Q, int(k), int(num_probes), int(probe_radius), int(take_main), int(take_flip))
        out = [_format(index, ids[i], d[i]) for i in range(len(Q))]
    return out[0] if single else out


def search_hybrid(index, query_vec, k, num_probes=2, parallel=True):
    """hybrid_lsh.clj:195-259: the query's own bucket in the first ``num_probes`` tables; 3 k rows of each are kept in the
    parallel form (the default), 2 k in the sequential one."""
    return _search(index, query_vec, k, num_probes, 0, (3 if parallel else 2) * int(k), int(k))


def search_hybrid_multiprobe(index, query_vec, k, num_probes=6, probe_radius=2, parallel=True):
    """hybrid_lsh.clj:261-342, in the order of its sequential branch (``parallel`` changes the order of ties only there,
    and nothing here): 2 k rows of the own bucket, k of every one-bit neighbour."""
    return _search(index, query_vec, k, num_probes, probe_radius, 2 * int(k), int(k))


def search_knn(index, query_vec, k, mode=None):
    """hybrid_lsh.clj:350-364"""
    probes, radius = mode_config(mode)
    return search_hybrid_multiprobe(index, query_vec, k, num_probes=probes, probe_radius=radius)


def search_batch(index, queries, k, mode=None):
    q = np.asarray(queries, np.float32)
    return search_knn(index, q[None, :] if q.ndim == 1 else q, k, mode)


def _allow_bits(index, filter_fn):
    """The predicate on the caller's ids, evaluated once per row on the host (or a ready bool array of length n)."""
    if callable(filter_fn):
        return np.fromiter((bool(filter_fn(i)) for i in index.ids), np.bool_, len(index.ids))
    bits = np.asarray(filter_fn)
    if bits.dtype != np.bool_ or bits.shape != (index.index.n,):
        raise ValueError("filter_fn must be a predicate on ids or a bool array with one entry per row")
    return bits


def search_batch_filtered(index, queries, k, filter_fn, mode=None):
    """FilterableIndex/search-knn-filtered* (api/protocol.clj:34-41) over the probed buckets, one predicate per call:
    ``filter_fn`` is called once per row with ``index.ids[i]`` (or is a bool array of length n) and packed into one
    allow-mask; the device tests the bit where a bucket is read and keeps the nearest 2 k / k PASSING rows of every probed
    bucket (hnswgpu_lsh_search_filtered) -- search_hybrid_multiprobe over buckets that list only the passing rows, not the
    reference's "search 3k, drop, keep k".  Modes map through mode_config."""
    queries = np.asarray(queries, np.float32)
    if queries.ndim == 1:
        queries = queries[None, :]
    if len(queries) == 0:
        return []
    probes, radius = mode_config(mode)
    bits = _allow_bits(index, filter_fn)
    if index.index.n == 0:
        return [[] for _ in range(len(queries))]
    ids, d = index.index.lsh_search_filtered(queries, int(k), engine.pack_mask(bits, index.index.n), probes, radius,
                                             2 * int(k), int(k))
    return [_format(index, ids[i], d[i]) for i in range(len(queries))]


def search_batch_filtered_each(index, queries, k, filter_fns, mode=None):
    """search_batch_filtered with one predicate (or bool array) PER QUERY: row q equals
    ``search_knn_filtered(index, queries[q], k, filter_fns[q], mode)``.  The same object, or equal bits, is evaluated and
    packed once; the batch goes through ONE hnswgpu_lsh_search_filtered_each call, equal masks adjacent (neighbouring waves
    then read the same mask words), and the original order is restored.  A batch whose filters are all one mask takes
    search_batch_filtered's single-mask call."""
    queries = np.asarray(queries, np.float32)
    if queries.ndim == 1:
        queries = queries[None, :]
    if len(filter_fns) != len(queries):
        raise ValueError("one filter per query: %d filters for %d queries" % (len(filter_fns), len(queries)))
    if len(queries) == 0:
        return []
    n = index.index.n
    masks, by_obj, by_bits, which = [], {}, {}, []   # distinct masks: (bits, packed)
    for f in filter_fns:
        m = by_obj.get(id(f))
        if m is None:
            bits = _allow_bits(index, f)
            key = bits.tobytes()
            m = by_bits.get(key)
            if m is None:
                m = by_bits[key] = len(masks)
                masks.append((bits, engine.pack_mask(bits, n)))
            by_obj[id(f)] = m
        which.append(m)
    if len(masks) == 1:
        return search_batch_filtered(index, queries, k, masks[0][0], mode)
    if n == 0:
        return [[] for _ in range(len(queries))]
    probes, radius = mode_config(mode)
    qs = sorted(range(len(queries)), key=lambda q: (which[q], q))   # equal masks adjacent
    rows = np.stack([masks[which[q]][1] for q in qs])
    gi, gd = index.index.lsh_search_filtered_each(queries[qs], int(k), rows, probes, radius, 2 * int(k), int(k))
    ids = np.empty((len(queries), int(k)), np.int32)
    d = np.empty((len(queries), int(k)), np.float32)
    ids[qs], d[qs] = gi, gd
    return [_format(index, ids[i], d[i]) for i in range(len(queries))]


def search_knn_filtered(index, query_vec, k, filter_fn, mode=None):
    """search_batch_filtered for one query: a list of ``{"id", "distance"}`` ascending, fewer than k when fewer are found."""
    return search_batch_filtered(index, np.asarray(query_vec, np.float32)[None, :], k, filter_fn, mode)[0]


def index_info(index):
    """hybrid_lsh.clj:366-379: total-buckets counts the non-empty buckets of all tables, as the reference's maps do"""
    n = index.index.n
    tables, bits = index.index.lsh_sizes()
    _, _, off, _ = index.index.lsh_get()
    total = int((np.diff(off, axis=1) > 0).sum())
    return {"type": "Hybrid LSH Index", "vectors": n, "hash-tables": tables, "buckets-per-table": 1 << bits,
            "total-buckets": total, "avg-bucket-size": n / total if total > 0 else 0}
