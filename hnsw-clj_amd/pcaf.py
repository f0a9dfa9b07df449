"""Mirror of ``hnsw.ann.dimreduct.pcaf`` (src/hnsw/ann/dimreduct/pcaf.clj, "P-HNSW"): a Gaussian random projection
to ``n_components`` dimensions, a brute-force cosine search in the projected space for min(k-filter, 3k)
candidates, and an exact cosine re-rank of those candidates in the original space (:196-253).

Device composition over the C ABI:
  * the projection matrix (Random(42) gaussians / sqrt(target-dim), :36-45) is an engine handle with metric DOT;
    ``hnswgpu_dense_distances`` against it IS project-vector-simd (:47-80) for a whole batch (out = -projection);
  * phase 1 is ``hnswgpu_exact_knn`` on the handle that holds the projected rows (:213-233);
  * phase 2 is ``hnswgpu_rerank`` on the handle that holds the original rows (:239-253).
The reference runs both phases in float32 through the Vector API, whose lane-reduction order is hardware
dependent; the kernels' fixed f32 orders are within the same 1e-7-relative envelope.

``one_handle=True`` keeps the same index on ONE handle instead (include/hnswgpu.h, "P-HNSW"): the projection and the projected
rows are state of the handle that holds the original rows, and a search is hnswgpu_pcaf_search(_dev) -- three launches, no
[queries][rows] intermediate.  The composition stays the default.  Only the one-handle index has the filtered searches
(search_batch_filtered / _each, search_knn_filtered): a predicate on the ids goes into phase 1 as an allow-mask
(hnswgpu_pcaf_search_filtered), so the candidates are passing rows -- not the protocol's "search 3k, drop, keep k".
Only the one-handle index is a live one too: add_vectors / remove_vectors / update_vectors (hnswgpu_pcaf_add / _remove /
_update) leave the handle what a fresh build over the rows it then holds would be.
"""
import numpy as np

from . import engine
from .datagen import JavaRandom
from .ultra_fast import _split

MODE_K_FILTER = {"turbo": 16, "fast": 24, "balanced": 32, "accurate": 48, "precise": 64}  # :283-290


def create_random_projection(original_dim, target_dim):
    """pcaf.clj:33-45 -> float32 [target_dim, original_dim]"""
    g = JavaRandom(42).next_gaussians(target_dim * original_dim)
    scale = np.float32(1.0 / np.sqrt(target_dim))
    return (scale * g.astype(np.float32)).reshape(target_dim, original_dim)


class PCAFIndex:
    """pcaf.clj:108-114"""

    def __init__(self, projection, proj_index, low_index, high_index, ids, k_filter):
        self.projection = projection      # float32 [target_dim, original_dim]
        self.proj_index = proj_index      # rows = projection matrix, metric DOT
        self.low_index = low_index        # projected rows, cosine (one handle: None, like proj_index -- high_index holds all)
        self.high_index = high_index      # original rows (float32), cosine
        self.ids = ids
        self.k_filter = k_filter
        self.dimension_reduction = projection.shape[1] / projection.shape[0]

    def close(self):
        for h in (self.proj_index, self.low_index, self.high_index):
            if h is not None:
                h.close()


def project_dev(index_or_proj, X):
    """project-vector-simd (:47-80) for every row of the CUDA tensor X."""
    proj = index_or_proj.proj_index if isinstance(index_or_proj, PCAFIndex) else index_or_proj
    if proj is None:
        raise ValueError("a one-handle index projects inside hnswgpu_pcaf_search (Index.pcaf_project for host arrays)")
    return -proj.dense_distances_dev(X)


def build_pcaf_index(data, n_components=100, k_filter=32, show_progress=False, num_threads=4, device=0, one_handle=False):
    """pcaf.clj:116-194 (``num_threads`` kept for signature parity)"""
    import torch

    ids, base = _split(data)
    dim = base.shape[1]
    if one_handle:
        high_index = engine.Index(base, engine.COSINE, device)
        high_index.pcaf_build(n_components, 42)
        if show_progress:
            print("P-HNSW: %d vectors, %d -> %d dims" % (len(ids), dim, n_components))
        return PCAFIndex(high_index.pcaf_get()[0], None, None, high_index, ids, k_filter)
    P = create_random_projection(dim, n_components)
    proj = engine.Index(P, engine.DOT, device)
    dev = torch.device("cuda", device)
    low = torch.empty((len(ids), n_components), dtype=torch.float32, device=dev)
    for i in range(0, len(ids), 65536):
        x = torch.from_numpy(base[i:i + 65536]).to(dev)
        low[i:i + 65536] = project_dev(proj, x)
    low_index = engine.Index(low, engine.COSINE, device)      # stays in HBM: device-to-device
    high_index = engine.Index(base, engine.COSINE, device)
    if show_progress:
        print("P-HNSW: %d vectors, %d -> %d dims" % (len(ids), dim, n_components))
    return PCAFIndex(P, proj, low_index, high_index, ids, k_filter)


def search_batch_dev(index, Q, k, k_filter=None):
    """Q: [nq, dim] float32 CUDA tensor -> (data positions [nq, k] int32, exact cosine distances [nq, k])."""
    if index.low_index is None:
        return index.high_index.pcaf_search_dev(Q, int(k), int(k_filter or index.k_filter))
    kf = min(int(k_filter or index.k_filter), 3 * int(k))            # :236
    kf = max(1, min(kf, index.low_index.n))
    cand, _ = index.low_index.exact_knn_dev(project_dev(index, Q), kf)
    return index.high_index.rerank_dev(Q, cand, int(k))


def search_batch(index, queries, k, mode=None):
    import torch

    queries = np.ascontiguousarray(queries, np.float32)
    if len(queries) == 0:
        return []
    if index.high_index.n == 0:
        return [[] for _ in queries]
    dev = torch.device("cuda", index.high_index.device)
    ids, d = search_batch_dev(index, torch.from_numpy(queries).to(dev), k, MODE_K_FILTER.get(mode))
    return [[{"id": index.ids[i], "distance": float(x)} for i, x in zip(ri, rd) if i >= 0]
            for ri, rd in zip(ids.cpu().tolist(), d.cpu().tolist())]


def search_pcaf_parallel(index, query_vec, k):
    """pcaf.clj:196-253"""
    return search_knn(index, query_vec, k)


def build_index(data, **opts):
    """:259-268"""
    return build_pcaf_index(data, **opts)


def search_knn(index, query_vec, k, mode=None):
    """:270-291"""
    q = np.asarray(query_vec, np.float32).reshape(1, -1)
    res = search_batch(index, q, k, mode)
    return res[0] if res else []


def _one_handle(index, what):
    if index.low_index is not None:
        raise ValueError("%s needs an index built with one_handle=True" % what)
    return index.high_index


def _rows_of(index):
    rows_of = {}
    for row, i in enumerate(index.ids):
        rows_of.setdefault(i, []).append(row)
    return rows_of


def add_vectors(index, data):
    """The reference's P-HNSW index has no add (build-pcaf-index returns an immutable record); ``data`` has the form
    ``build_index`` takes; every vector joins the original rows and, projected under the index's projection by the kernel that
    projected the old rows, the projected rows (hnswgpu_pcaf_add).  Empty ``data`` does nothing.  Returns the index."""
    handle = _one_handle(index, "add_vectors")
    ids, rows = _split(data)
    if len(ids):
        handle.pcaf_add(rows)
        index.ids = list(index.ids) + list(ids)
    return index


def remove_vectors(index, ids):
    """The reference's P-HNSW index has no remove either: ``ids`` are the caller's ids, the form ``index.ids`` holds; their
    vectors leave the original and the projected rows, the kept rows are renumbered densely in their old order
    (hnswgpu_pcaf_remove), and ``index.ids`` follows.  An unknown id raises KeyError before the device is touched; an id of
    several rows removes them all.  Empty ``ids`` does nothing.  Returns the index."""
    handle = _one_handle(index, "remove_vectors")
    ids = list(ids)
    if not ids:
        return index
    rows_of = _rows_of(index)
    rows = []
    for i in ids:
        if i not in rows_of:
            raise KeyError(i)
        rows.extend(rows_of[i])
    gone = set(rows)
    kept = [i for row, i in enumerate(index.ids) if row not in gone]
    n_after = handle.pcaf_remove(np.asarray(rows, np.int32))
    assert n_after == len(kept), "hnswgpu_pcaf_remove left %d rows, the id list %d" % (n_after, len(kept))
    index.ids = kept
    return index


def update_vectors(index, data):
    """"Update existing vectors" (the open item of the reference's to-do list): ``data`` has the form ``build_index`` takes;
    the vector stored under each id takes the new values and is projected again (hnswgpu_pcaf_update).  It keeps its id:
    ``index.ids`` is unchanged.  An unknown id raises KeyError, an id that names several rows or appears twice in ``data``
    raises ValueError, both before the device is touched.  Empty ``data`` does nothing.  Returns the index."""
    handle = _one_handle(index, "update_vectors")
    ids, rows = _split(data)
    if not len(ids):
        return index
    rows_of = _rows_of(index)
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
    handle.pcaf_update(np.asarray(at, np.int32), rows)
    return index


def _format(index, ids, d):
    return [{"id": index.ids[i], "distance": float(x)} for i, x in zip(ids.tolist(), d.tolist()) if i >= 0]


def _filtered_args(index, queries, mode):
    if index.low_index is not None:
        raise ValueError("filtered P-HNSW search needs an index built with one_handle=True")
    queries = np.asarray(queries, np.float32)
    return (queries[None, :] if queries.ndim == 1 else queries), int(MODE_K_FILTER.get(mode) or index.k_filter)


def _allow_bits(index, filter_fn):
    """The predicate on the caller's ids, evaluated once per row on the host (or a ready bool array of length n)."""
    if callable(filter_fn):
        return np.fromiter((bool(filter_fn(i)) for i in index.ids), np.bool_, len(index.ids))
    bits = np.asarray(filter_fn)
    if bits.dtype != np.bool_ or bits.shape != (index.high_index.n,):
        raise ValueError("filter_fn must be a predicate on ids or a bool array with one entry per row")
    return bits


def search_batch_filtered(index, queries, k, filter_fn, mode=None):
    """FilterableIndex/search-knn-filtered* (api/protocol.clj:34-41) through phase 1, one predicate per call: ``filter_fn`` is
    called once per row with ``index.ids[i]`` (or is a bool array of length n) and packed into one allow-mask; phase 1 picks
    its min(k-filter, 3k) candidates among the PASSING rows and fetches only those (hnswgpu_pcaf_search_filtered)."""
    queries, kf = _filtered_args(index, queries, mode)
    if len(queries) == 0:
        return []
    bits = _allow_bits(index, filter_fn)
    n = index.high_index.n
    if n == 0:
        return [[] for _ in range(len(queries))]
    ids, d = index.high_index.pcaf_search_filtered(queries, int(k), engine.pack_mask(bits, n), kf)
    return [_format(index, ids[i], d[i]) for i in range(len(queries))]


def search_batch_filtered_each(index, queries, k, filter_fns, mode=None):
    """search_batch_filtered with one predicate (or bool array) PER QUERY: row q equals
    ``search_knn_filtered(index, queries[q], k, filter_fns[q], mode)``.  The same object, or equal bits, is evaluated and
    packed once; the batch goes through ONE hnswgpu_pcaf_search_filtered_each call, equal masks adjacent (the union of a query
    block's masks, which decides what the block fetches, then is small), and the original order is restored.  A batch whose
    filters are all one mask takes search_batch_filtered's single-mask call."""
    queries, kf = _filtered_args(index, queries, mode)
    if len(filter_fns) != len(queries):
        raise ValueError("one filter per query: %d filters for %d queries" % (len(filter_fns), len(queries)))
    if len(queries) == 0:
        return []
    n = index.high_index.n
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
    qs = sorted(range(len(queries)), key=lambda q: (which[q], q))   # equal masks adjacent
    rows = np.stack([masks[which[q]][1] for q in qs])
    gi, gd = index.high_index.pcaf_search_filtered_each(queries[qs], int(k), rows, kf)
    ids = np.empty((len(queries), int(k)), np.int32)
    d = np.empty((len(queries), int(k)), np.float32)
    ids[qs], d[qs] = gi, gd
    return [_format(index, ids[i], d[i]) for i in range(len(queries))]


def search_knn_filtered(index, query_vec, k, filter_fn, mode=None):
    """search_batch_filtered for one query: a list of ``{"id", "distance"}`` ascending, fewer than k when fewer pass."""
    return search_batch_filtered(index, np.asarray(query_vec, np.float32)[None, :], k, filter_fn, mode)[0]


def index_info(index):
    """:293-302"""
    return {"type": "P-HNSW (SIMD Optimized)", "original-dim": index.projection.shape[1],
            "reduced-dim": index.projection.shape[0], "reduction-ratio": index.dimension_reduction,
            "k-filter": index.k_filter, "vectors": index.high_index.n, "optimization": "HIP"}


def cleanup(index):
    """:304-308"""
    index.close()
