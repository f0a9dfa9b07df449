"""Mirror of ``hnsw.api.protocol`` (src/hnsw/api/protocol.clj): ANNIndex, BatchSearchIndex, PersistableIndex,
FilterableIndex and the default helpers (filtered search by post-filtering, :96-101; sequential batch search, :92-95) over
the two GPU-served index types.  The HNSW index filters on the device (ultra_fast.search_knn_filtered).  GpuIvfFlatIndex is
the reference's IVF index, which has no FilterableIndex and is served by the default helper; GpuFilterableIvfFlatIndex adds
the protocol on top of it, filtering inside the list scan (ivf_flat.search_knn_filtered); GpuHybridLshIndex and
GpuFilterableHybridLshIndex are the same pair for the hybrid LSH index (hybrid_lsh.search_knn_filtered: inside the bucket scan)."""
from . import hybrid_lsh, index_io, ivf_flat, ultra_fast


class ANNIndex:
    """protocol.clj:9-28"""

    def search_knn_star(self, query, k, mode):
        raise NotImplementedError

    def index_info_star(self):
        raise NotImplementedError

    def index_type_star(self):
        raise NotImplementedError


class BatchSearchIndex:
    """protocol.clj:58-67"""

    def search_batch_star(self, queries, k, mode):
        raise NotImplementedError


class PersistableIndex:
    """protocol.clj:43-56"""

    def save_index_star(self, filepath):
        raise NotImplementedError


class FilterableIndex:
    """protocol.clj:34-41"""

    def search_knn_filtered_star(self, query, k, filter_fn, mode):
        raise NotImplementedError


def default_batch_search(index, queries, k, mode):
    """protocol.clj:92-95: one search-knn* per query (what an index without search-batch* gets)."""
    return [index.search_knn_star(q, k, mode) for q in queries]


def default_filtered_search(index, query, k, filter_fn, mode):
    """protocol.clj:96-101: search for 3k candidates, keep those whose id passes the predicate, take k."""
    return [r for r in index.search_knn_star(query, 3 * k, mode) if filter_fn(r["id"])][:k]


class GpuHnswIndex(ANNIndex, BatchSearchIndex, PersistableIndex, FilterableIndex):
    def __init__(self, graph):
        self.graph = graph

    def search_knn_filtered_star(self, query, k, filter_fn, mode=None):
        return ultra_fast.search_knn_filtered(self.graph, query, k, filter_fn)

    def search_batch_filtered(self, queries, k, filter_fns, mode=None):
        """search_knn_filtered_star for a batch, one predicate per query, in one chain of launches (not in the reference)."""
        return ultra_fast.search_batch_filtered_each(self.graph, queries, k, filter_fns)

    def save_index_star(self, filepath):
        index_io.save_index(self.graph, filepath)
        return True

    def search_knn_star(self, query, k, mode=None):
        return ultra_fast.search_knn(self.graph, query, k)  # modes are ignored by the reference too

    def search_batch_star(self, queries, k, mode=None):
        return ultra_fast.search_batch(self.graph, queries, k)

    def index_info_star(self):
        return ultra_fast.graph_info(self.graph)

    def index_type_star(self):
        return "ultra-fast"


class GpuIvfFlatIndex(ANNIndex, BatchSearchIndex, PersistableIndex):
    def __init__(self, index):
        self.index = index

    def save_index_star(self, filepath):
        index_io.save_index(self.index, filepath)
        return True

    def search_knn_star(self, query, k, mode="balanced"):
        return ivf_flat.search_knn(self.index, query, k, mode)

    def search_batch_star(self, queries, k, mode="balanced"):
        return ivf_flat.search_batch(self.index, queries, k, mode)

    def search_batch_filtered(self, queries, k, filter_fns, mode="balanced"):
        """ivf_flat.search_knn_filtered for a batch, one predicate per query, in one chain of launches (not in the reference)."""
        return ivf_flat.search_batch_filtered_each(self.index, queries, k, filter_fns, mode or "balanced")

    def index_info_star(self):
        return ivf_flat.index_info(self.index)

    def index_type_star(self):
        return "ivf-flat"


class GpuFilterableIvfFlatIndex(GpuIvfFlatIndex, FilterableIndex):
    """The IVF index with the allow-mask through its list scan: the k nearest PASSING rows of the probed lists."""

    def search_knn_filtered_star(self, query, k, filter_fn, mode="balanced"):
        return ivf_flat.search_knn_filtered(self.index, query, k, filter_fn, mode or "balanced")


class GpuHybridLshIndex(ANNIndex, BatchSearchIndex):
    """hnsw.ann.hash.hybrid-lsh behind the protocol (unified.clj's :hybrid-lsh); not persistable, as in the reference."""

    def __init__(self, index):
        self.index = index

    def search_knn_star(self, query, k, mode=None):
        return hybrid_lsh.search_knn(self.index, query, k, mode)

    def search_batch_star(self, queries, k, mode=None):
        return hybrid_lsh.search_batch(self.index, queries, k, mode)

    def index_info_star(self):
        return hybrid_lsh.index_info(self.index)

    def index_type_star(self):
        return "hybrid-lsh"


class GpuFilterableHybridLshIndex(GpuHybridLshIndex, FilterableIndex):
    """The hybrid LSH index with the allow-mask through its bucket scan: every probed bucket keeps its nearest PASSING rows."""

    def search_knn_filtered_star(self, query, k, filter_fn, mode=None):
        return hybrid_lsh.search_knn_filtered(self.index, query, k, filter_fn, mode)

    def search_batch_filtered(self, queries, k, filter_fns, mode=None):
        """search_knn_filtered_star for a batch, one predicate per query, in one chain of launches (not in the reference)."""
        return hybrid_lsh.search_batch_filtered_each(self.index, queries, k, filter_fns, mode)


def supports_filtering(index):
    """protocol.clj:73-76 (an index without it is served by default_filtered_search)"""
    return isinstance(index, FilterableIndex)


def supports_batch_search(index):
    """protocol.clj:83-86"""
    return isinstance(index, BatchSearchIndex)


def supports_persistence(index):
    """protocol.clj:78-81"""
    return isinstance(index, PersistableIndex)
