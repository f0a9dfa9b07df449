"""Mirror of ``hnsw.ann.partition.ivf-flat`` (src/hnsw/ann/partition/ivf_flat.clj).

``build_index(data, num_partitions=24, distance_fn=..., max_iterations=10)`` runs k-means++ /
Lloyd on the device; ``search_knn(index, q, k, mode)`` / ``search_ivf_flat(index, q, k, mode=...,
num_probes=...)`` scan the probed lists with the HIP scan kernel;
``add_vectors(index, data)`` grows a built index, ``remove_vectors(index, ids)`` shrinks it, ``update_vectors(index, data)``
gives stored vectors new values under their ids; ``search_knn_filtered`` / ``search_batch_filtered`` (not in the reference, whose IVF index has no
FilterableIndex) scan only the rows of the probed lists that pass a predicate; ``search_batch_filtered_each`` takes one
predicate per query.
"""
import random

import numpy as np

from . import engine
from .ultra_fast import _metric_of, _split, cosine_distance_ultra

# ivf_flat.clj:243-247
MODE_CONFIGS = {
    "turbo": {"num_probes": 1, "use_centroids": False},
    "fast": {"num_probes": 2, "use_centroids": True},
    "balanced": {"num_probes": 4, "use_centroids": True},
    "accurate": {"num_probes": 8, "use_centroids": True},
    "precise": {"num_probes": 12, "use_centroids": True},
}


class IVFFlatIndex:
    """ivf_flat.clj:22-27: partitions / centroids / norms live on the device behind ``index``."""

    def __init__(self, index, ids, distance_fn, num_partitions):
        self.index = index
        self.ids = ids
        self.distance_fn = distance_fn
        self.num_partitions = num_partitions

    def close(self):
        self.index.close()


def build_ivf_flat_index(data, num_partitions=24, distance_fn=cosine_distance_ultra, show_progress=True,
                         partition_method="kmeans", max_iterations=10, seed=42, device=0):
    """ivf_flat.clj:137-211"""
    metric = _metric_of(distance_fn)
    ids, base = _split(data)
    if len(ids) == 0:
        raise ValueError("cannot partition an empty dataset")
    idx = engine.Index(base, metric, device)
    if partition_method == "kmeans":
        idx.ivf_build(num_partitions, max_iterations, seed)
    else:
        raise ValueError("unsupported :partition-method %r (only :kmeans is served by the device build)" % (partition_method,))
    return IVFFlatIndex(idx, ids, distance_fn, num_partitions)


def build_index(data, **opts):
    """ivf_flat.clj:300-303"""
    return build_ivf_flat_index(data, **opts)


def add_vectors(index, data):
    """The IVF side of add-vector! (api.clj:30-33; the reference's IVFFlatIndex itself is immutable): ``data`` has the form
    ``build_index`` takes; every vector joins its nearest partition behind the partition's present members
    (hnswgpu_ivf_add), the centroids stay.  Returns the index."""
    ids, rows = _split(data)
    if ids:
        index.index.ivf_add(rows)
        index.ids.extend(ids)
    return index


def remove_vectors(index, ids):
    """The reference's IVFFlatIndex has no remove (it is an immutable record); what is restated is its list order
    (ivf_flat.clj:137-211, "inverted lists in index order"): ``ids`` are the caller's ids, the form ``index.ids`` holds; their
    vectors leave the base and their partitions, the kept members of a partition stay in their order (hnswgpu_ivf_remove), the
    centroids stay, and ``index.ids`` follows.  An unknown id raises KeyError before the device is touched; an id of several
    rows removes them all.  Empty ``ids`` does nothing.  Returns the index."""
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
    kept = index.index.ivf_remove(np.asarray(rows, np.int32))
    index.ids = [index.ids[i] for i in kept]
    return index


def update_vectors(index, data):
    """"Update existing vectors" (the open item of the reference's to-do list; its IVFFlatIndex is an immutable record):
    ``data`` has the form ``build_index`` takes; the vector stored under each id takes the new values, moves to its nearest
    partition if that is another one (hnswgpu_ivf_update), and keeps its id: ``index.ids`` is unchanged, the centroids stay.  An
    unknown id raises KeyError, an id that names several rows or appears twice in ``data`` raises ValueError, both before the
    device is touched.  Empty ``data`` does nothing.  Returns the index."""
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
    index.index.ivf_update(np.asarray(at, np.int32), rows)
    return index


def _format(index, ids_row, d_row):
    return [{"id": index.ids[i], "distance": float(d)} for i, d in zip(ids_row, d_row) if i >= 0]


def search_ivf_flat(index, query_vec, k, mode="balanced", num_probes=None, use_centroids=None):
    """ivf_flat.clj:236-294.  A preset mode wins over num_probes exactly as in the reference (:249-251);
    pass mode=None (or any non-preset) to use num_probes."""
    cfg = MODE_CONFIGS.get(mode) or {"num_probes": num_probes or 4,
                                     "use_centroids": True if use_centroids is None else use_centroids}
    q = np.asarray(query_vec, np.float32)
    single = q.ndim == 1
    Q = q[None, :] if single else q
    npb = int(cfg["num_probes"])
    if cfg["use_centroids"]:
        ids, d = index.index.ivf_search(Q, int(k), npb)
    else:  # (take num-probes (shuffle (range num-partitions))) :271-272
        probes = np.stack([np.array(random.sample(range(index.num_partitions), min(npb, index.num_partitions)),
                                    np.int32) for _ in range(len(Q))])
        ids, d = index.index.ivf_search_lists(Q, int(k), probes)
    out = [_format(index, ids[i], d[i]) for i in range(len(Q))]
    return out[0] if single else out


def search_knn(index, query_vec, k, mode="balanced"):
    """ivf_flat.clj:305-317"""
    return search_ivf_flat(index, query_vec, k, mode=mode)


def search_batch(index, queries, k, mode="balanced", num_probes=None):
    return search_ivf_flat(index, np.asarray(queries, np.float32), k, mode=mode, num_probes=num_probes)


def _allow_bits(index, filter_fn):
    """The predicate on the caller's ids, evaluated once per row on the host (or a ready bool array of length n)."""
    if callable(filter_fn):
        return np.fromiter((bool(filter_fn(i)) for i in index.ids), np.bool_, len(index.ids))
    bits = np.asarray(filter_fn)
    if bits.dtype != np.bool_ or bits.shape != (index.index.n,):
        raise ValueError("filter_fn must be a predicate on ids or a bool array with one entry per row")
    return bits


def search_batch_filtered(index, queries, k, filter_fn, mode="balanced", num_probes=None):
    """FilterableIndex/search-knn-filtered* (api/protocol.clj:34-41) over the probed lists, one predicate per call:
    ``filter_fn`` is called once per row with ``index.ids[i]`` (or is a bool array of length n) and packed into one
    allow-mask; the device scans exactly the passing rows of the probed lists (hnswgpu_ivf_search_filtered) and returns the
    k nearest of them -- not the reference's "search 3k, drop, keep k".  Mode presets as in search_ivf_flat.  A mode without
    centroid routing (:turbo, ``use_centroids False``: random lists, :271-272) goes through the default helper's rule --
    search_ivf_flat for 3k, keep what passes, take k."""
    queries = np.asarray(queries, np.float32)
    if queries.ndim == 1:
        queries = queries[None, :]
    if len(queries) == 0:
        return []
    cfg = MODE_CONFIGS.get(mode) or {"num_probes": num_probes or 4, "use_centroids": True}
    bits = _allow_bits(index, filter_fn)
    if not cfg["use_centroids"]:
        res = search_ivf_flat(index, queries, 3 * int(k), mode=mode, num_probes=num_probes)
        passing = {i for i, b in zip(index.ids, bits) if b}
        return [[r for r in rs if r["id"] in passing][:int(k)] for rs in res]
    ids, d = index.index.ivf_search_filtered(queries, int(k), int(cfg["num_probes"]), engine.pack_mask(bits, index.index.n))
    return [_format(index, ids[i], d[i]) for i in range(len(queries))]


def search_batch_filtered_each(index, queries, k, filter_fns, mode="balanced", num_probes=None):
    """search_batch_filtered with one predicate (or bool array) PER QUERY: row q equals
    ``search_knn_filtered(index, queries[q], k, filter_fns[q], mode, num_probes)``.  The same object, or equal bits, is evaluated
    and packed once; the batch goes through ONE hnswgpu_ivf_search_filtered_each call, equal masks adjacent (neighbouring
    queries then read the same mask words), and the original order is restored.  A batch whose filters are all one mask takes
    search_batch_filtered's single-mask call; a mode without centroid routing goes through its 3k post-filter rule, per query."""
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
        return search_batch_filtered(index, queries, k, masks[0][0], mode, num_probes)
    cfg = MODE_CONFIGS.get(mode) or {"num_probes": num_probes or 4, "use_centroids": True}
    if not cfg["use_centroids"]:
        res = search_ivf_flat(index, queries, 3 * int(k), mode=mode, num_probes=num_probes)
        passing = [{i for i, b in zip(index.ids, bits) if b} for bits, _ in masks]
        return [[r for r in rs if r["id"] in passing[m]][:int(k)] for rs, m in zip(res, which)]
    qs = sorted(range(len(queries)), key=lambda q: (which[q], q))   # equal masks adjacent
    rows = np.stack([masks[which[q]][1] for q in qs])
    gi, gd = index.index.ivf_search_filtered_each(queries[qs], int(k), int(cfg["num_probes"]), rows)
    ids = np.empty((len(queries), int(k)), np.int32)
    d = np.empty((len(queries), int(k)), np.float32)
    ids[qs], d[qs] = gi, gd
    return [_format(index, ids[i], d[i]) for i in range(len(queries))]


def search_knn_filtered(index, query_vec, k, filter_fn, mode="balanced", num_probes=None):
    """search_batch_filtered for one query: a list of ``{"id", "distance"}`` ascending, fewer than k when fewer pass."""
    return search_batch_filtered(index, np.asarray(query_vec, np.float32)[None, :], k, filter_fn, mode, num_probes)[0]


def index_info(index):
    """ivf_flat.clj:319-327"""
    return {"type": "IVF-FLAT Index", "vectors": index.index.n, "partitions": index.num_partitions,
            "avg-partition-size": index.index.n / index.num_partitions, "method": "k-means++"}
