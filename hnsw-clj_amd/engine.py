"""Index handle over libhnswgpu.so -- thin, typed wrapper of the C ABI (include/hnswgpu.h).

numpy arrays go through the host-pointer entry points; torch CUDA tensors go through the ``_dev``
entry points on torch's current stream (zero copy).  Nothing here computes distances on the CPU.
"""
import ctypes as C

import numpy as np

from . import _native
from ._native import COSINE, DOT, L2, check, debug_counter, get_tuning, lib, set_tuning  # noqa: F401

METRICS = {"cosine": COSINE, "l2": L2, "euclidean": L2, "dot": DOT, COSINE: COSINE, L2: L2, DOT: DOT}
PROF_IVF_SCAN, PROF_HNSW, PROF_ASSIGN, PROF_UPDATE = 0, 1, 2, 3
BUILD_SEQUENTIAL, BUILD_HEURISTIC, BUILD_SYMMETRIC, BUILD_EXTEND = 1, 2, 4, 8     # include/hnswgpu.h: HNSWGPU_BUILD_*


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _queries(Q, dim):
    Q = _f32(Q)
    if Q.ndim == 1:
        Q = Q[None, :]
    if Q.ndim != 2 or Q.shape[1] != dim:
        raise ValueError("queries must be (nq, %d), got %s" % (dim, Q.shape))
    return Q


def pack_mask(allow, n):
    """The allow-mask of a filtered search (include/hnswgpu.h): (n + 31) // 32 uint32 words, row i passes iff bit (i & 31) of
    word i >> 5 is set (little-endian bit order, padded with zeros to whole words).  ``allow``: a bool array of length n, or
    an iterable of row ids."""
    n = int(n)
    a = np.asarray(allow if hasattr(allow, "__len__") else list(allow))
    if a.dtype == np.bool_:
        if a.shape != (n,):
            raise ValueError("a bool mask must have one entry per row (%d), got %s" % (n, a.shape))
        bits = a
    else:
        ids = a.astype(np.int64).reshape(-1)
        if len(ids) and (ids.min() < 0 or ids.max() >= n):
            raise ValueError("row ids must lie in [0, %d)" % n)
        bits = np.zeros(n, np.bool_)
        bits[ids] = True
    nwords = (n + 31) // 32
    packed = np.zeros(nwords * 4, np.uint8)
    b = np.packbits(bits, bitorder="little")
    packed[:len(b)] = b
    return packed.view("<u4").astype(np.uint32, copy=False)


def pack_masks(allows, n):
    """One allow-mask per query (the *_filtered_each calls): ``allows`` is a sequence of what pack_mask takes -- bool arrays of
    length n or iterables of row ids -- and the result is the [nq][(n + 31) // 32] uint32 array whose row q is
    pack_mask(allows[q], n)."""
    n = int(n)
    if isinstance(allows, np.ndarray) and allows.dtype == np.bool_ and allows.ndim != 2:
        raise ValueError("a bool array of masks must be (nq, %d), got %s" % (n, allows.shape))
    rows = [pack_mask(a, n) for a in allows]
    out = np.zeros((len(rows), (n + 31) // 32), np.uint32)
    for q, r in enumerate(rows):
        out[q] = r
    return out


def _mask_rows(allow_each, n, nq):
    """Packed masks (pack_masks) checked against the index size and the batch."""
    a = np.ascontiguousarray(allow_each)
    if a.dtype != np.uint32 or a.shape != (nq, (n + 31) // 32):
        raise ValueError("allow_each must be the (%d, %d) uint32 words of pack_masks(..., %d)" % (nq, (n + 31) // 32, n))
    return a


def _mask_words(allow, n):
    """A packed mask (pack_mask) checked against the index size."""
    a = np.ascontiguousarray(allow)
    if a.dtype != np.uint32 or a.ndim != 1 or len(a) != (n + 31) // 32:
        raise ValueError("allow must be the %d uint32 words of pack_mask(..., %d)" % ((n + 31) // 32, n))
    return a


def parts_layout(base, rows):
    """Per-part row lists -> what a forest handle (Index.hnsw_build_parts / set_graph_parts) is made from: (the rows of
    ``base`` grouped by part, part_off int64 [nparts + 1], the data position of every handle row int32).  Part p is the handle
    rows [part_off[p], part_off[p + 1]), in the order of ``rows[p]``; an empty list is an empty part."""
    rows = [np.asarray(r, np.int64).reshape(-1) for r in rows]
    part_off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=part_off[1:])
    pos = np.concatenate(rows + [np.empty(0, np.int64)])
    if len(pos) and (pos.min() < 0 or pos.max() >= len(base)):
        raise ValueError("row lists must hold positions in [0, %d)" % len(base))
    return np.ascontiguousarray(np.asarray(base, np.float32)[pos]), part_off, pos.astype(np.int32)


class GraphParts:
    """The part tables of a forest (include/hnswgpu.h: hnswgpu_set_graph_parts)."""

    def __init__(self, part_off, part_entry, part_max_level):
        self.part_off = np.ascontiguousarray(part_off, np.int64)
        self.part_entry = np.ascontiguousarray(part_entry, np.int32)
        self.part_max_level = np.ascontiguousarray(part_max_level, np.int32)
        self.nparts = len(self.part_entry)


class Graph:
    """Flat HNSW graph (layout documented in include/hnswgpu.h)."""

    def __init__(self, levels, l0_adj, up_off, up_adj, M, entry, max_level):
        self.levels = np.ascontiguousarray(levels, np.int32)
        self.l0_adj = np.ascontiguousarray(l0_adj, np.int32)
        self.up_off = np.ascontiguousarray(up_off, np.int64)
        self.up_adj = np.ascontiguousarray(up_adj, np.int32)
        self.M = int(M)
        self.n = len(self.levels)
        self.M0 = self.l0_adj.shape[1] if self.l0_adj.ndim == 2 else (self.l0_adj.size // max(self.n, 1))
        self.entry = int(entry)
        self.max_level = int(max_level)


class Index:
    """Base vectors resident in HBM + optional HNSW graph and IVF lists."""

    def __init__(self, base, metric="cosine", device=0):
        self.metric = METRICS[metric]
        self.device = int(device)
        self._h = C.c_void_p(None)
        if hasattr(base, "is_cuda") and base.is_cuda:  # torch tensor already in HBM
            import torch

            assert base.dtype == torch.float32 and base.dim() == 2
            base = base.contiguous()
            self.n, self.dim = int(base.shape[0]), int(base.shape[1])
            st = torch.cuda.current_stream(base.device).cuda_stream
            check(lib().hnswgpu_create_dev(base.data_ptr(), self.n, self.dim, self.dim, self.metric,
                                           base.device.index or 0, st, C.byref(self._h)))
            self.device = base.device.index or 0
        else:
            base = _f32(base)
            if base.ndim != 2:
                raise ValueError("base must be (n, dim)")
            self.n, self.dim = base.shape
            check(lib().hnswgpu_create(_p(base), self.n, self.dim, self.metric, self.device, C.byref(self._h)))

    @classmethod
    def load(cls, path, device=0):
        """hnswgpu_load: base + graph + IVF lists from one flat binary file."""
        self = cls.__new__(cls)
        self._h = C.c_void_p(None)
        self.device = int(device)
        check(lib().hnswgpu_load(str(path).encode(), self.device, C.byref(self._h)))
        n, dim, metric = C.c_int64(), C.c_int32(), C.c_int32()
        check(lib().hnswgpu_info(self._h, C.byref(n), C.byref(dim), C.byref(metric), None, None))
        self.n, self.dim, self.metric = n.value, dim.value, metric.value
        return self

    def save(self, path):
        check(lib().hnswgpu_save(self._h, str(path).encode()))

    @property
    def has_graph(self):
        g = C.c_int32()
        check(lib().hnswgpu_info(self._h, None, None, None, C.byref(g), None))
        return bool(g.value)

    # -- lifetime
    def close(self):
        if self._h:
            lib().hnswgpu_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        check(lib().hnswgpu_sync(self._h))

    # -- distance seams
    def batch_distances(self, q, ids=None, m=None):
        q = _f32(q).reshape(-1)
        if len(q) != self.dim:
            raise ValueError("query has %d elements, index dim is %d" % (len(q), self.dim))
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.int32)
            m = len(ids)
        elif m is None:
            m = self.n
        out = np.empty(m, np.float32)
        check(lib().hnswgpu_batch_distances(self._h, _p(q), _p(ids), m, _p(out)))
        return out

    def set_rejection_test(self, mode):
        """0 = off, 1 = large batches (default), 2 = every launch: int8 rejection test of the HNSW traversal."""
        check(lib().hnswgpu_set_rejection_test(self._h, int(mode)))

    def hnsw_last_order(self):
        """hnswgpu_hnsw_last_order: (order, keys) of the last ordered traversal launch on this handle -- the query indices sorted
        by (key, index) and every query's key, the index of its nearest pivot row -- or None before the first such launch."""
        nq = C.c_int32(0)
        check(lib().hnswgpu_hnsw_last_order(self._h, None, None, 0, C.byref(nq)))
        if nq.value == 0:
            return None
        order, keys = np.empty(nq.value, np.int32), np.empty(nq.value, np.int32)
        check(lib().hnswgpu_hnsw_last_order(self._h, order.ctypes.data, keys.ctypes.data, nq.value, C.byref(nq)))
        return order, keys

    def set_hnsw_dense_bounds(self, mode, budget_mb=-1):
        """hnswgpu_set_hnsw_dense_bounds: 1 = the rule (default), 0 = never, 2 = every eligible launch; budget_mb < 0 keeps it."""
        check(lib().hnswgpu_set_hnsw_dense_bounds(self._h, int(mode), int(budget_mb)))

    def hnsw_dense_bounds_state(self):
        """hnswgpu_hnsw_dense_bounds_state: (mode, budget_mb, launches that used the table, device bytes of its scratch)."""
        m, b, l, n = C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().hnswgpu_hnsw_dense_bounds_state(self._h, C.byref(m), C.byref(b), C.byref(l), C.byref(n)))
        return m.value, b.value, l.value, n.value

    def hnsw_dense_rows(self, rows=-1):
        """hnswgpu_hnsw_dense_rows: f32 rows in flight behind the table on 768-float rows, 0 = the rule (default), 2 / 4 forced,
        negative keeps the setting; returns (the setting, launches on this handle that kept four rows in flight)."""
        r, n = C.c_int32(0), C.c_int64(0)
        check(lib().hnswgpu_hnsw_dense_rows(self._h, int(rows), C.byref(r), C.byref(n)))
        return r.value, n.value

    def hnsw_dense_bounds(self, Q):
        """hnswgpu_hnsw_dense_bounds: the rejection test's lower bounds of every query of Q (may be a strided view of rows)
        against all n rows, (nq, n) float32, by the kernels in front of a launch with the dense bounds table."""
        Q = np.asarray(Q, np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dim:
            raise ValueError("Q must be (nq, %d)" % self.dim)
        if Q.strides[1] != 4 or Q.strides[0] % 4 or Q.strides[0] < 4 * self.dim:
            Q = np.ascontiguousarray(Q)
        n = C.c_int64()
        check(lib().hnswgpu_info(self._h, C.byref(n), None, None, None, None))
        out = np.empty((len(Q), n.value), np.float32)
        check(lib().hnswgpu_hnsw_dense_bounds(self._h, Q.ctypes.data, len(Q), Q.strides[0] // 4, _p(out)))
        return out

    def hnsw_rejection_state(self):
        """hnswgpu_hnsw_rejection_state: (state, off, frac) -- what rejection mode 1 has measured on this graph."""
        st, off, fr = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
        check(lib().hnswgpu_hnsw_rejection_state(self._h, C.byref(st), C.byref(off), C.byref(fr)))
        return st.value, bool(off.value), fr.value

    def rejection_stats(self, reset=True):
        """(f32 rows fetched, neighbours evaluated) by the HNSW traversals since the last reset, while profiling was on."""
        a, b = C.c_int64(0), C.c_int64(0)
        check(lib().hnswgpu_get_rejection_stats(self._h, C.byref(a), C.byref(b), 1 if reset else 0))
        return a.value, b.value

    def hnsw_rejection_bounds(self, q, ids):
        """Lower bounds of d(q, row) as the HNSW traversals' rejection test computes them: int8 rows against the 16-bit
        query code (NaN = no bound)."""
        q = _f32(q).reshape(-1)
        if len(q) != self.dim:
            raise ValueError("query has %d elements, index dim is %d" % (len(q), self.dim))
        ids = np.ascontiguousarray(ids, np.int32)
        out = np.empty(len(ids), np.float32)
        check(lib().hnswgpu_hnsw_rejection_bounds(self._h, _p(q), _p(ids), len(ids), _p(out)))
        return out

    def rejection_bounds(self, q, ids):
        """Lower bounds of d(q, row) from the int8 rows with the query in int8 as well: the lower side of distance_bounds
        (NaN = no bound).  The HNSW traversals' own bounds: hnsw_rejection_bounds."""
        q = _f32(q).reshape(-1)
        if len(q) != self.dim:
            raise ValueError("query has %d elements, index dim is %d" % (len(q), self.dim))
        ids = np.ascontiguousarray(ids, np.int32)
        out = np.empty(len(ids), np.float32)
        check(lib().hnswgpu_rejection_bounds(self._h, _p(q), _p(ids), len(ids), _p(out)))
        return out

    def distance_bounds(self, q, ids):
        """(lower, upper) bounds of d(q, row) from the int8 rows: lower <= distance <= upper, NaN = no bound."""
        q = _f32(q).reshape(-1)
        if len(q) != self.dim:
            raise ValueError("query has %d elements, index dim is %d" % (len(q), self.dim))
        ids = np.ascontiguousarray(ids, np.int32)
        lb, ub = np.empty(len(ids), np.float32), np.empty(len(ids), np.float32)
        check(lib().hnswgpu_distance_bounds(self._h, _p(q), _p(ids), len(ids), _p(lb), _p(ub)))
        return lb, ub

    def ivf_half_bounds(self, q, list_rows):
        """(lower, upper) bounds of d(q, list row) from the half-precision list rows (batches of 1.5 M candidates and more
        filter the int8 survivors with them); rows are positions in list order.  NaN = no bound."""
        q = _f32(q).reshape(-1)
        if len(q) != self.dim:
            raise ValueError("query has %d elements, index dim is %d" % (len(q), self.dim))
        rows = np.ascontiguousarray(list_rows, np.int32)
        lb, ub = np.empty(len(rows), np.float32), np.empty(len(rows), np.float32)
        check(lib().hnswgpu_ivf_half_bounds(self._h, _p(q), _p(rows), len(rows), _p(lb), _p(ub)))
        return lb, ub

    def ivf_home_bounds(self, Q, row_begin, row_end):
        """(lower, upper) bounds [nq][row_end - row_begin] of d(query, list row) from the matrix-core half-precision pass of
        large batches (ivf_home_kernel); rows are positions in list order.  NaN = no bound."""
        Q = _f32(Q).reshape(-1, self.dim)
        m = int(row_end) - int(row_begin)
        lb, ub = np.empty((len(Q), m), np.float32), np.empty((len(Q), m), np.float32)
        check(lib().hnswgpu_ivf_home_bounds(self._h, _p(Q), len(Q), int(row_begin), int(row_end), _p(lb), _p(ub)))
        return lb, ub

    def norms(self):
        out = np.empty(self.n, np.float32)
        check(lib().hnswgpu_norms(self._h, _p(out)))
        return out

    def exact_knn(self, Q, k):
        Q = _queries(Q, self.dim)
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        check(lib().hnswgpu_exact_knn(self._h, _p(Q), len(Q), k, _p(ids), _p(d)))
        return ids, d

    def exact_knn_filtered(self, Q, k, allow):
        """hnswgpu_exact_knn_filtered: the k nearest of the rows ``allow`` (pack_mask) lets pass -- exact, distances in the
        gather order at every batch size, ties to the lower row id, -1 / +inf padded when fewer than k rows pass."""
        Q = _queries(Q, self.dim)
        allow = _mask_words(allow, self.n)
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        check(lib().hnswgpu_exact_knn_filtered(self._h, _p(Q), len(Q), k, _p(allow), _p(ids), _p(d)))
        return ids, d

    def exact_knn_filtered_each(self, Q, k, allow_each):
        """hnswgpu_exact_knn_filtered_each: row q is exact_knn_filtered(Q[q:q + 1], k, allow_each[q]) -- one mask per query
        (pack_masks), one chain of launches for the batch; a group of queries fetches the union of its passing rows once."""
        Q = _queries(Q, self.dim)
        allow_each = _mask_rows(allow_each, self.n, len(Q))
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        check(lib().hnswgpu_exact_knn_filtered_each(self._h, _p(Q), len(Q), k, _p(allow_each), _p(ids), _p(d)))
        return ids, d

    def rerank(self, Q, cand, k):
        """Per query: exact distances to its candidate rows cand[q] (-1 = skip), stable sort, first k."""
        Q = _queries(Q, self.dim)
        cand = np.ascontiguousarray(cand, dtype=np.int32)
        if cand.ndim != 2 or cand.shape[0] != len(Q):
            raise ValueError("cand must be [nq, m]")
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        check(lib().hnswgpu_rerank(self._h, _p(Q), len(Q), _p(cand), cand.shape[1], k, _p(ids), _p(d)))
        return ids, d

    def dense_distances(self, Q):
        """[nq, n] distances from every query to every row."""
        Q = _queries(Q, self.dim)
        out = np.empty((len(Q), self.n), np.float32)
        check(lib().hnswgpu_dense_distances(self._h, _p(Q), len(Q), _p(out)))
        return out

    # -- HNSW
    def set_graph(self, g):
        check(lib().hnswgpu_set_graph(self._h, _p(g.levels), _p(g.l0_adj), g.M0, _p(g.up_off), _p(g.up_adj), g.M,
                                      g.entry, g.max_level))

    def hnsw_build(self, M=16, ef_construction=200, seed=42, sequential=False, heuristic=False, symmetric=False,
                   extend=False):
        """hnswgpu_hnsw_build_ex: batched closest-m insertion by default (ultra_fast.clj:216-299); sequential = the
        reference's insert-single order and start level (the CPU restatement's graph, oracle.c, edge for edge); heuristic / symmetric / extend =
        neighbour selection of src/hnsw/graph.clj:162-232."""
        flags = (BUILD_SEQUENTIAL if sequential else 0) | (BUILD_HEURISTIC if heuristic else 0) | \
                (BUILD_SYMMETRIC if symmetric else 0) | (BUILD_EXTEND if extend else 0)
        check(lib().hnswgpu_hnsw_build_ex(self._h, M, ef_construction, seed, flags))

    # -- a forest: several sub-graphs on this handle, searched in one launch (include/hnswgpu.h)
    def set_graph_parts(self, g, parts):
        """hnswgpu_set_graph_parts: ``g`` as for set_graph (its entry / max_level are not used), ``parts`` a GraphParts."""
        if len(parts.part_off) != parts.nparts + 1 or len(parts.part_max_level) != parts.nparts:
            raise ValueError("part tables of %d parts must hold %d offsets and %d levels" % (parts.nparts, parts.nparts + 1, parts.nparts))
        check(lib().hnswgpu_set_graph_parts(self._h, _p(g.levels), _p(g.l0_adj), g.M0, _p(g.up_off), _p(g.up_adj), g.M,
                                            parts.nparts, _p(parts.part_off), _p(parts.part_entry), _p(parts.part_max_level)))

    def hnsw_build_parts(self, part_off, M=16, ef_construction=200, seed=42, flags=0):
        """hnswgpu_hnsw_build_parts: every part [part_off[p], part_off[p + 1]) built as hnsw_build builds a handle over its rows
        alone (flags: BUILD_*)."""
        part_off = np.ascontiguousarray(part_off, np.int64)
        check(lib().hnswgpu_hnsw_build_parts(self._h, len(part_off) - 1, _p(part_off), M, ef_construction, seed, int(flags)))

    def graph_parts(self):
        n = C.c_int32()
        check(lib().hnswgpu_graph_parts(self._h, C.byref(n), None, None, None))
        off, ent, lv = np.zeros(n.value + 1, np.int64), np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        check(lib().hnswgpu_graph_parts(self._h, C.byref(n), _p(off), _p(ent), _p(lv)))
        return GraphParts(off, ent, lv)

    def _nprobe(self, probes, nq):
        if probes is None:
            n = C.c_int32()
            check(lib().hnswgpu_graph_parts(self._h, C.byref(n), None, None, None))
            return n.value
        assert probes.ndim == 2 and probes.shape[0] == nq, "probes must be [nq, nprobe]"
        return int(probes.shape[1])

    def hnsw_search_parts(self, Q, k_part, k, ef=0, probes=None, want_stats=False):
        """hnswgpu_hnsw_search_parts: probes [nq, nprobe] part ids (-1 = skip), None = every part; -> handle rows [nq, k]
        (-1 padded), distances; stats [nq, nprobe, 2]."""
        Q = _queries(Q, self.dim)
        if probes is not None:
            probes = np.ascontiguousarray(probes, np.int32)
        nprobe = self._nprobe(probes, len(Q))
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        stats = np.zeros((len(Q), nprobe, 2), np.int64) if want_stats else None
        check(lib().hnswgpu_hnsw_search_parts(self._h, _p(Q), len(Q), k_part, int(ef or 0), _p(probes), nprobe, k, _p(ids), _p(d),
                                              _p(stats)))
        return (ids, d, stats) if want_stats else (ids, d)

    def hnsw_search_parts_dev(self, Q, k_part, k, ef=0, probes=None, out=None, stats=None):
        """hnswgpu_hnsw_search_parts_dev on torch's current stream: probes an int32 CUDA tensor [nq, nprobe] or None; stats an
        int64 CUDA tensor [nq, nprobe, 2] or None."""
        import torch

        Q, ids, d, st = self._dev_args(Q, k, out)
        if probes is not None:
            assert probes.is_cuda and probes.dtype == torch.int32
            probes = probes.contiguous()
        nprobe = self._nprobe(probes, Q.shape[0])
        check(lib().hnswgpu_hnsw_search_parts_dev(self._h, Q.data_ptr(), Q.shape[0], k_part, int(ef or 0),
                                                  probes.data_ptr() if probes is not None else None, nprobe, k, ids.data_ptr(),
                                                  d.data_ptr(), stats.data_ptr() if stats is not None else None, st))
        return ids, d

    def hnsw_add(self, rows, ef_construction=200, seed=42):
        """insert-single on the live index (ultra_fast.clj:216-275): `rows` join the base and the installed graph; returns
        the row ids they got."""
        rows = _queries(rows, self.dim)
        first = self.n
        check(lib().hnswgpu_hnsw_add(self._h, _p(rows), len(rows), ef_construction, seed))
        self.n += len(rows)
        return np.arange(first, self.n, dtype=np.int32)

    def hnsw_remove(self, rows):
        """hnswgpu_hnsw_remove: the rows named by `rows` (row ids, any order, repeats count once) leave the base and the installed
        graph; the kept rows are renumbered densely in their old order, a list that loses no member keeps its members, a list that
        loses one is selected again from the old graph (include/hnswgpu.h).  Returns `kept`, the int64 array of the old row ids
        that remain, ascending: the row now numbered i was kept[i]."""
        rows = np.ascontiguousarray(rows, np.int32).reshape(-1)
        n_after = C.c_int64(-1)
        check(lib().hnswgpu_hnsw_remove(self._h, _p(rows), len(rows), C.byref(n_after)))
        keep = np.ones(self.n, np.bool_)
        keep[rows] = False
        kept = np.flatnonzero(keep).astype(np.int64)
        assert len(kept) == n_after.value, "hnswgpu_hnsw_remove left %d rows, the id list %d" % (n_after.value, len(kept))
        self.n = int(n_after.value)
        return kept

    def hnsw_update(self, ids, rows, ef_construction=200):
        """hnswgpu_hnsw_update: row ``ids[i]`` takes the values ``rows[i]`` (row ids in any order, none named twice); n, every
        row id and every row's level stay.  The rows are unlinked as hnswgpu_hnsw_remove unlinks rows that leave -- nothing is
        renumbered -- and inserted again in ascending id order as hnswgpu_hnsw_add inserts rows (include/hnswgpu.h)."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        rows = _queries(rows, self.dim)
        if len(rows) != len(ids):
            raise ValueError("%d ids for %d rows" % (len(ids), len(rows)))
        check(lib().hnswgpu_hnsw_update(self._h, _p(ids), _p(rows), len(ids), ef_construction))

    def get_graph(self):
        M, M0, ent, mx = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        blocks = C.c_int64()
        check(lib().hnswgpu_graph_sizes(self._h, C.byref(M), C.byref(M0), C.byref(blocks), C.byref(ent),
                                        C.byref(mx)))
        levels = np.zeros(self.n, np.int32)
        l0 = np.full((self.n, M0.value), -1, np.int32)
        up_off = np.zeros(self.n + 1, np.int64)
        up = np.full(blocks.value * M.value, -1, np.int32)
        check(lib().hnswgpu_get_graph(self._h, _p(levels), _p(l0), _p(up_off), _p(up)))
        return Graph(levels, l0, up_off, up, M.value, ent.value, mx.value)

    def hnsw_search(self, Q, k, ef=0, want_stats=False):
        Q = _queries(Q, self.dim)
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        stats = np.zeros((len(Q), 2), np.int64) if want_stats else None
        check(lib().hnswgpu_hnsw_search(self._h, _p(Q), len(Q), k, int(ef or 0), _p(ids), _p(d), _p(stats)))
        return (ids, d, stats) if want_stats else (ids, d)

    def hnsw_search_filtered(self, Q, k, allow, ef=0, want_stats=False):
        """hnswgpu_hnsw_search_filtered: hnsw_search's traversal at ef, then the first k entries of its result list (its
        first min(ef, 1024) entries) that ``allow`` (pack_mask) lets pass; stats are the unfiltered traversal's."""
        Q = _queries(Q, self.dim)
        allow = _mask_words(allow, self.n)
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        stats = np.zeros((len(Q), 2), np.int64) if want_stats else None
        check(lib().hnswgpu_hnsw_search_filtered(self._h, _p(Q), len(Q), k, int(ef or 0), _p(allow), _p(ids), _p(d),
                                                 _p(stats)))
        return (ids, d, stats) if want_stats else (ids, d)

    def hnsw_search_filtered_each(self, Q, k, allow_each, ef=0, want_stats=False):
        """hnswgpu_hnsw_search_filtered_each: hnsw_search_filtered with one mask per query (pack_masks) in one launch."""
        Q = _queries(Q, self.dim)
        allow_each = _mask_rows(allow_each, self.n, len(Q))
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        stats = np.zeros((len(Q), 2), np.int64) if want_stats else None
        check(lib().hnswgpu_hnsw_search_filtered_each(self._h, _p(Q), len(Q), k, int(ef or 0), _p(allow_each), _p(ids), _p(d),
                                                      _p(stats)))
        return (ids, d, stats) if want_stats else (ids, d)

    # -- IVF
    def ivf_build(self, nlist=24, max_iterations=10, seed=42):
        check(lib().hnswgpu_ivf_build(self._h, nlist, max_iterations, seed))

    def ivf_add(self, rows):
        """hnswgpu_ivf_add: `rows` join the base and the installed lists (each to its nearest centroid, behind the list's
        present members); returns the row ids they got."""
        rows = _queries(rows, self.dim)
        first = self.n
        check(lib().hnswgpu_ivf_add(self._h, _p(rows), len(rows)))
        self.n += len(rows)
        return np.arange(first, self.n, dtype=np.int32)

    def ivf_remove(self, rows):
        """hnswgpu_ivf_remove: the rows named by `rows` (row ids, any order, repeats count once) leave the base and the installed
        lists; the kept rows are renumbered densely in their old order, every list keeps its kept members in their order.
        Returns `kept`, the int64 array of the old row ids that remain, ascending: the row now numbered i was kept[i]."""
        rows = np.ascontiguousarray(rows, np.int32).reshape(-1)
        n_after = C.c_int64(-1)
        check(lib().hnswgpu_ivf_remove(self._h, _p(rows), len(rows), C.byref(n_after)))
        keep = np.ones(self.n, np.bool_)
        keep[rows] = False
        kept = np.flatnonzero(keep).astype(np.int64)
        assert len(kept) == n_after.value, "hnswgpu_ivf_remove left %d rows, the id list %d" % (n_after.value, len(kept))
        self.n = int(n_after.value)
        return kept

    def ivf_update(self, ids, rows):
        """hnswgpu_ivf_update: row ``ids[i]`` takes the values ``rows[i]`` (row ids in any order, none named twice); n, every
        row id and the centroids stay.  A row whose nearest centroid is still its list keeps its list position; a row that
        moves joins its new list behind the members that remain there, ascending by row id among the call's movers."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        rows = _queries(rows, self.dim)
        if len(rows) != len(ids):
            raise ValueError("%d ids for %d rows" % (len(ids), len(rows)))
        check(lib().hnswgpu_ivf_update(self._h, _p(ids), _p(rows), len(ids)))

    def set_ivf(self, centroids, list_off, list_ids):
        cen = _f32(centroids)
        off = np.ascontiguousarray(list_off, np.int64)
        ids = np.ascontiguousarray(list_ids, np.int32)
        check(lib().hnswgpu_set_ivf(self._h, _p(cen), cen.shape[0], _p(off), _p(ids)))

    def ivf_stream_state(self):
        """1 if this handle's first-search measurement switched the survivor stream off (measures now if it has not yet)."""
        off = C.c_int32(0)
        check(lib().hnswgpu_ivf_stream_state(self._h, C.byref(off)))
        return off.value

    def ivf_set_stream_state(self, off):
        """Install a verdict without measuring: the shards of one index share one (see include/hnswgpu.h)."""
        check(lib().hnswgpu_ivf_set_stream_state(self._h, 1 if off else 0))

    def set_ivf_shard(self, centroids, list_off, list_ids, global_list_len):
        """This handle holds some of the inverted lists of a larger index (see include/hnswgpu.h)."""
        cen = _f32(centroids)
        off = np.ascontiguousarray(list_off, np.int64)
        ids = np.ascontiguousarray(list_ids, np.int32)
        gl = np.ascontiguousarray(global_list_len, np.int64)
        if len(gl) != cen.shape[0] or len(off) != cen.shape[0] + 1:
            raise ValueError("need nlist global lengths and nlist + 1 offsets")
        check(lib().hnswgpu_set_ivf_shard(self._h, _p(cen), cen.shape[0], _p(off), _p(ids), _p(gl)))

    @property
    def nlist(self):
        nl = C.c_int32()
        check(lib().hnswgpu_info(self._h, None, None, None, None, C.byref(nl)))
        return nl.value

    def get_ivf(self):
        nl = self.nlist
        cen = np.empty((nl, self.dim), np.float32)
        off = np.empty(nl + 1, np.int64)
        ids = np.empty(self.n, np.int32)
        check(lib().hnswgpu_get_ivf(self._h, _p(cen), _p(off), _p(ids)))
        return cen, off, ids

    def kmeans_assign(self, centroids):
        cen = _f32(centroids)
        a = np.empty(self.n, np.int32)
        d = np.empty(self.n, np.float32)
        check(lib().hnswgpu_kmeans_assign(self._h, _p(cen), cen.shape[0], _p(a), _p(d)))
        return a, d

    def list_means(self, list_off, list_ids):
        off = np.ascontiguousarray(list_off, np.int64)
        ids = np.ascontiguousarray(list_ids, np.int32)
        out = np.empty((len(off) - 1, self.dim), np.float32)
        check(lib().hnswgpu_list_means(self._h, len(off) - 1, _p(off), _p(ids), _p(out)))
        return out

    def list_sums(self, list_off, list_ids):
        """f64 column sums of every list (compute-centroid without the division)."""
        off = np.ascontiguousarray(list_off, np.int64)
        ids = np.ascontiguousarray(list_ids, np.int32)
        out = np.empty((len(off) - 1, self.dim), np.float64)
        check(lib().hnswgpu_list_sums(self._h, len(off) - 1, _p(off), _p(ids), _p(out)))
        return out

    def kmeanspp(self, nlist, seed=42):
        out = np.empty(nlist, np.int32)
        check(lib().hnswgpu_kmeanspp(self._h, nlist, seed, _p(out)))
        return out

    def ivf_search(self, Q, k, nprobe, want_probes=False):
        Q = _queries(Q, self.dim)
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        pr = np.empty((len(Q), nprobe), np.int32) if want_probes else None
        check(lib().hnswgpu_ivf_search(self._h, _p(Q), len(Q), k, nprobe, _p(ids), _p(d), _p(pr)))
        return (ids, d, pr) if want_probes else (ids, d)

    def ivf_search_filtered(self, Q, k, nprobe, allow, want_probes=False):
        """hnswgpu_ivf_search_filtered: ivf_search's routing, then the k nearest rows of the probed lists that ``allow``
        (pack_mask, indexed by row id) lets pass -- only those rows are read; -1 / +inf where fewer than k pass."""
        Q = _queries(Q, self.dim)
        allow = _mask_words(allow, self.n)
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        pr = np.empty((len(Q), nprobe), np.int32) if want_probes else None
        check(lib().hnswgpu_ivf_search_filtered(self._h, _p(Q), len(Q), k, nprobe, _p(allow), _p(ids), _p(d), _p(pr)))
        return (ids, d, pr) if want_probes else (ids, d)

    def ivf_search_filtered_each(self, Q, k, nprobe, allow_each, want_probes=False):
        """hnswgpu_ivf_search_filtered_each: row q is ivf_search_filtered(Q[q:q + 1], k, nprobe, allow_each[q]) -- one mask per
        query (pack_masks) in one chain of launches; the bit is tested where the list is read."""
        Q = _queries(Q, self.dim)
        allow_each = _mask_rows(allow_each, self.n, len(Q))
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        pr = np.empty((len(Q), nprobe), np.int32) if want_probes else None
        check(lib().hnswgpu_ivf_search_filtered_each(self._h, _p(Q), len(Q), k, nprobe, _p(allow_each), _p(ids), _p(d), _p(pr)))
        return (ids, d, pr) if want_probes else (ids, d)

    def ivf_search_lists(self, Q, k, probes):
        Q = _queries(Q, self.dim)
        probes = np.ascontiguousarray(probes, np.int32).reshape(len(Q), -1)
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        check(lib().hnswgpu_ivf_search_lists(self._h, _p(Q), len(Q), k, probes.shape[1], _p(probes), _p(ids), _p(d)))
        return ids, d

    # -- hybrid LSH (include/hnswgpu.h: "Hybrid LSH")
    def lsh_build(self, tables=8, bits=12, proj_dim=64, seed=42):
        """hnswgpu_lsh_build: hyperplanes from java.util.Random(seed) as the reference draws them, hash, buckets."""
        check(lib().hnswgpu_lsh_build(self._h, tables, bits, proj_dim, seed))

    def set_lsh(self, planes):
        """hnswgpu_set_lsh: the caller's hyperplanes (tables, bits, dim)."""
        planes = _f32(planes)
        if planes.ndim != 3 or planes.shape[2] != self.dim:
            raise ValueError("planes must be (tables, bits, %d), got %s" % (self.dim, planes.shape))
        check(lib().hnswgpu_set_lsh(self._h, _p(planes), planes.shape[0], planes.shape[1]))

    def lsh_sizes(self):
        t, b = C.c_int32(), C.c_int32()
        check(lib().hnswgpu_lsh_sizes(self._h, C.byref(t), C.byref(b)))
        return t.value, b.value

    def lsh_get(self):
        """(planes (T, bits, dim), codes (n, T) uint16, off (T, 2^bits + 1), ids (T, n)): bucket b of table t is
        ids[t, off[t, b]:off[t, b + 1]], rows ascending."""
        t, b = self.lsh_sizes()
        planes = np.empty((t, b, self.dim), np.float32)
        codes = np.empty((self.n, t), np.uint16)
        off = np.empty((t, (1 << b) + 1), np.int64)
        ids = np.empty((t, self.n), np.int32)
        check(lib().hnswgpu_lsh_get(self._h, _p(planes), _p(codes), _p(off), _p(ids)))
        return planes, codes, off, ids

    def lsh_hash(self, Q):
        """Codes (nq, T) of arbitrary vectors under the handle's hyperplanes (the kernel that hashed the base rows)."""
        Q = _queries(Q, self.dim)
        codes = np.empty((len(Q), self.lsh_sizes()[0]), np.uint16)
        check(lib().hnswgpu_lsh_hash(self._h, _p(Q), len(Q), _p(codes)))
        return codes

    def lsh_add(self, rows):
        """hnswgpu_lsh_add: `rows` join the base and every hash table's buckets (behind a bucket's present members, in row
        order); returns the row ids they got."""
        rows = _queries(rows, self.dim)
        first = self.n
        check(lib().hnswgpu_lsh_add(self._h, _p(rows), len(rows)))
        self.n += len(rows)
        return np.arange(first, self.n, dtype=np.int32)

    def lsh_remove(self, rows):
        """hnswgpu_lsh_remove: the rows named by `rows` (row ids, any order, repeats count once) leave the base and every hash
        table's buckets; the kept rows are renumbered densely in their old order.  Returns `kept`, the int64 array of the old
        row ids that remain, ascending: the row now numbered i was kept[i]."""
        rows = np.ascontiguousarray(rows, np.int32).reshape(-1)
        n_after = C.c_int64(-1)
        check(lib().hnswgpu_lsh_remove(self._h, _p(rows), len(rows), C.byref(n_after)))
        keep = np.ones(self.n, np.bool_)
        keep[rows] = False
        kept = np.flatnonzero(keep).astype(np.int64)
        assert len(kept) == n_after.value, "hnswgpu_lsh_remove left %d rows, the id list %d" % (n_after.value, len(kept))
        self.n = int(n_after.value)
        return kept

    def lsh_update(self, ids, rows):
        """hnswgpu_lsh_update: row ``ids[i]`` takes the values ``rows[i]`` (row ids in any order, none named twice); n, every
        row id and the planes stay.  Per table a row whose code is unchanged keeps its bucket; a row whose code changed leaves
        its bucket and joins the new one at the place its row id gives it: the handle is what a fresh one over the new base is."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        rows = _queries(rows, self.dim)
        if len(rows) != len(ids):
            raise ValueError("%d ids for %d rows" % (len(ids), len(rows)))
        check(lib().hnswgpu_lsh_update(self._h, _p(ids), _p(rows), len(ids)))

    def lsh_search(self, Q, k, num_probes=6, probe_radius=2, take_main=None, take_flip=None, out=None):
        """hnswgpu_lsh_search (numpy queries) / hnswgpu_lsh_search_dev (a torch device tensor, torch's current stream):
        multi-probe search; the takes default to the reference's 2 k and k."""
        take_main = 2 * k if take_main is None else take_main
        take_flip = k if take_flip is None else take_flip
        if hasattr(Q, "is_cuda") and Q.is_cuda:
            Q, ids, d, st = self._dev_args(Q, k, out)
            check(lib().hnswgpu_lsh_search_dev(self._h, Q.data_ptr(), Q.shape[0], k, num_probes, probe_radius, take_main,
                                               take_flip, ids.data_ptr(), d.data_ptr(), st))
            return ids, d
        Q = _queries(Q, self.dim)
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        check(lib().hnswgpu_lsh_search(self._h, _p(Q), len(Q), k, num_probes, probe_radius, take_main, take_flip, _p(ids), _p(d)))
        return ids, d

    def lsh_search_filtered(self, Q, k, allow, num_probes=6, probe_radius=2, take_main=None, take_flip=None, out=None):
        """hnswgpu_lsh_search_filtered (numpy queries and pack_mask words) / _dev (torch device tensors for both, torch's
        current stream: enqueues only): lsh_search over buckets that list only the rows ``allow`` lets pass -- the bit is
        tested where the bucket is read, the takes apply to the passing rows; -1 / +inf where fewer than k are found."""
        take_main = 2 * k if take_main is None else take_main
        take_flip = k if take_flip is None else take_flip
        if hasattr(Q, "is_cuda") and Q.is_cuda:
            Q, ids, d, st = self._dev_args(Q, k, out)
            allow = self._dev_mask(allow, Q)
            check(lib().hnswgpu_lsh_search_filtered_dev(self._h, Q.data_ptr(), Q.shape[0], k, num_probes, probe_radius, take_main,
                                                        take_flip, allow.data_ptr(), ids.data_ptr(), d.data_ptr(), st))
            return ids, d
        Q = _queries(Q, self.dim)
        allow = _mask_words(allow, self.n)
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        check(lib().hnswgpu_lsh_search_filtered(self._h, _p(Q), len(Q), k, num_probes, probe_radius, take_main, take_flip,
                                                _p(allow), _p(ids), _p(d)))
        return ids, d

    def lsh_search_filtered_each(self, Q, k, allow_each, num_probes=6, probe_radius=2, take_main=None, take_flip=None, out=None):
        """hnswgpu_lsh_search_filtered_each / _dev: row q is lsh_search_filtered(Q[q:q + 1], k, allow_each[q], ...) -- one mask
        per query (pack_masks) in one chain of launches."""
        take_main = 2 * k if take_main is None else take_main
        take_flip = k if take_flip is None else take_flip
        if hasattr(Q, "is_cuda") and Q.is_cuda:
            Q, ids, d, st = self._dev_args(Q, k, out)
            allow_each = self._dev_masks(allow_each, Q)
            check(lib().hnswgpu_lsh_search_filtered_each_dev(self._h, Q.data_ptr(), Q.shape[0], k, num_probes, probe_radius,
                                                             take_main, take_flip, allow_each.data_ptr(), ids.data_ptr(),
                                                             d.data_ptr(), st))
            return ids, d
        Q = _queries(Q, self.dim)
        allow_each = _mask_rows(allow_each, self.n, len(Q))
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        check(lib().hnswgpu_lsh_search_filtered_each(self._h, _p(Q), len(Q), k, num_probes, probe_radius, take_main, take_flip,
                                                     _p(allow_each), _p(ids), _p(d)))
        return ids, d

    # -- zero-copy device entry points (torch tensors, torch's current stream)
    def _dev_args(self, Q, k, out=None):
        import torch

        assert Q.is_cuda and Q.dtype == torch.float32 and Q.dim() == 2 and Q.shape[1] == self.dim
        Q = Q.contiguous()
        if out is not None:      # caller-owned result tensors: nothing is allocated on the call path
            ids, d = out
        else:
            ids = torch.empty((Q.shape[0], k), dtype=torch.int32, device=Q.device)
            d = torch.empty((Q.shape[0], k), dtype=torch.float32, device=Q.device)
        st = torch.cuda.current_stream(Q.device).cuda_stream
        return Q, ids, d, st

    def hnsw_search_dev(self, Q, k, ef=0, out=None, stats=None):
        Q, ids, d, st = self._dev_args(Q, k, out)
        check(lib().hnswgpu_hnsw_search_dev(self._h, Q.data_ptr(), Q.shape[0], k, int(ef or 0), ids.data_ptr(),
                                            d.data_ptr(), stats.data_ptr() if stats is not None else None, st))
        return ids, d

    def ivf_search_dev(self, Q, k, nprobe, out=None):
        Q, ids, d, st = self._dev_args(Q, k, out)
        check(lib().hnswgpu_ivf_search_dev(self._h, Q.data_ptr(), Q.shape[0], k, nprobe, ids.data_ptr(),
                                           d.data_ptr(), st))
        return ids, d

    def ivf_search_shard_dev(self, Q, k, nprobe):
        """ivf_search_dev + every result's position in the candidate stream of the whole (sharded) index."""
        import torch

        Q, ids, d, st = self._dev_args(Q, k)
        order = torch.empty((Q.shape[0], k), dtype=torch.int32, device=Q.device)   # uint32 bits
        check(lib().hnswgpu_ivf_search_shard_dev(self._h, Q.data_ptr(), Q.shape[0], k, nprobe, ids.data_ptr(),
                                                 d.data_ptr(), order.data_ptr(), st))
        return ids, d, order

    def exact_knn_dev(self, Q, k, out=None):
        Q, ids, d, st = self._dev_args(Q, k, out)
        check(lib().hnswgpu_exact_knn_dev(self._h, Q.data_ptr(), Q.shape[0], k, ids.data_ptr(), d.data_ptr(), st))
        return ids, d

    def _dev_mask(self, allow, Q):
        """The packed mask as a device tensor of 32-bit words (torch.from_numpy(pack_mask(...).view(np.int32)).to(device))."""
        assert allow.is_cuda and allow.device == Q.device and allow.element_size() == 4 and allow.dim() == 1
        assert allow.numel() == (self.n + 31) // 32, "allow must hold (n + 31) // 32 words"
        return allow.contiguous()

    def exact_knn_filtered_dev(self, Q, k, allow, out=None):
        """hnswgpu_exact_knn_filtered_dev on torch's current stream (waits for it once, for the number of passing rows)."""
        Q, ids, d, st = self._dev_args(Q, k, out)
        allow = self._dev_mask(allow, Q)
        check(lib().hnswgpu_exact_knn_filtered_dev(self._h, Q.data_ptr(), Q.shape[0], k, allow.data_ptr(), ids.data_ptr(),
                                                   d.data_ptr(), st))
        return ids, d

    def hnsw_search_filtered_dev(self, Q, k, allow, ef=0, out=None, stats=None):
        Q, ids, d, st = self._dev_args(Q, k, out)
        allow = self._dev_mask(allow, Q)
        check(lib().hnswgpu_hnsw_search_filtered_dev(self._h, Q.data_ptr(), Q.shape[0], k, int(ef or 0), allow.data_ptr(),
                                                     ids.data_ptr(), d.data_ptr(),
                                                     stats.data_ptr() if stats is not None else None, st))
        return ids, d

    def _dev_masks(self, allow_each, Q):
        """Packed masks as a device tensor of [nq][(n + 31) // 32] 32-bit words (pack_masks(...).view(np.int32))."""
        assert allow_each.is_cuda and allow_each.device == Q.device and allow_each.element_size() == 4
        assert tuple(allow_each.shape) == (Q.shape[0], (self.n + 31) // 32), "allow_each must be (nq, (n + 31) // 32) words"
        return allow_each.contiguous()

    def exact_knn_filtered_each_dev(self, Q, k, allow_each, out=None):
        """hnswgpu_exact_knn_filtered_each_dev on torch's current stream (waits for it once, for the groups' passing counts)."""
        Q, ids, d, st = self._dev_args(Q, k, out)
        allow_each = self._dev_masks(allow_each, Q)
        check(lib().hnswgpu_exact_knn_filtered_each_dev(self._h, Q.data_ptr(), Q.shape[0], k, allow_each.data_ptr(),
                                                        ids.data_ptr(), d.data_ptr(), st))
        return ids, d

    def hnsw_search_filtered_each_dev(self, Q, k, allow_each, ef=0, out=None, stats=None):
        """hnswgpu_hnsw_search_filtered_each_dev on torch's current stream: enqueues only."""
        Q, ids, d, st = self._dev_args(Q, k, out)
        allow_each = self._dev_masks(allow_each, Q)
        check(lib().hnswgpu_hnsw_search_filtered_each_dev(self._h, Q.data_ptr(), Q.shape[0], k, int(ef or 0),
                                                          allow_each.data_ptr(), ids.data_ptr(), d.data_ptr(),
                                                          stats.data_ptr() if stats is not None else None, st))
        return ids, d

    def ivf_search_filtered_dev(self, Q, k, nprobe, allow, out=None):
        """hnswgpu_ivf_search_filtered_dev on torch's current stream: enqueues only, nothing is read back."""
        Q, ids, d, st = self._dev_args(Q, k, out)
        allow = self._dev_mask(allow, Q)
        check(lib().hnswgpu_ivf_search_filtered_dev(self._h, Q.data_ptr(), Q.shape[0], k, nprobe, allow.data_ptr(),
                                                    ids.data_ptr(), d.data_ptr(), st))
        return ids, d

    def ivf_search_filtered_each_dev(self, Q, k, nprobe, allow_each, out=None):
        """hnswgpu_ivf_search_filtered_each_dev on torch's current stream: enqueues only, nothing is read back."""
        Q, ids, d, st = self._dev_args(Q, k, out)
        allow_each = self._dev_masks(allow_each, Q)
        check(lib().hnswgpu_ivf_search_filtered_each_dev(self._h, Q.data_ptr(), Q.shape[0], k, nprobe, allow_each.data_ptr(),
                                                         ids.data_ptr(), d.data_ptr(), st))
        return ids, d

    def rerank_dev(self, Q, cand, k, out=None):
        import torch

        Q, ids, d, st = self._dev_args(Q, k)
        assert cand.is_cuda and cand.dtype == torch.int32 and cand.dim() == 2 and cand.shape[0] == Q.shape[0]
        cand = cand.contiguous()
        if out is not None:
            ids, d = out
        check(lib().hnswgpu_rerank_dev(self._h, Q.data_ptr(), Q.shape[0], cand.data_ptr(), cand.shape[1], k,
                                       ids.data_ptr(), d.data_ptr(), st))
        return ids, d

    def dense_distances_dev(self, Q, out=None):
        import torch

        Q, _, _, st = self._dev_args(Q, 1)
        if out is None:
            out = torch.empty((Q.shape[0], self.n), dtype=torch.float32, device=Q.device)
        check(lib().hnswgpu_dense_distances_dev(self._h, Q.data_ptr(), Q.shape[0], out.data_ptr(), st))
        return out

    # -- measurement
    def set_profiling(self, on=True):
        check(lib().hnswgpu_set_profiling(self._h, 1 if on else 0))

    def get_profile(self, which, reset=True):
        ms, cnt = C.c_double(), C.c_int64()
        check(lib().hnswgpu_get_profile(self._h, which, C.byref(ms), C.byref(cnt), 1 if reset else 0))
        return ms.value, cnt.value


def pair_distance(metric, a, b, device=0):
    """(distance-fn a b) on the device: one pair through the same kernel as everything else."""
    a, b = _f32(a).reshape(-1), _f32(b).reshape(-1)
    if len(a) != len(b):
        raise ValueError("vectors differ in length (%d vs %d)" % (len(a), len(b)))
    out = C.c_float()
    check(lib().hnswgpu_pair_distance(METRICS[metric], _p(a), _p(b), len(a), device, C.byref(out)))
    return float(out.value)


def merge_topk_dev(ids, dist, out=None):
    """[nshard][nq][k] torch CUDA tensors of global ids / distances -> merged [nq][k]."""
    import torch

    assert ids.is_cuda and ids.dtype == torch.int32 and dist.dtype == torch.float32 and ids.dim() == 3
    ids, dist = ids.contiguous(), dist.contiguous()
    ns, nq, k = ids.shape
    oi = torch.empty((nq, k), dtype=torch.int32, device=ids.device) if out is None else out[0]
    od = torch.empty((nq, k), dtype=torch.float32, device=ids.device) if out is None else out[1]
    st = torch.cuda.current_stream(ids.device).cuda_stream
    check(lib().hnswgpu_merge_topk_dev(ids.device.index or 0, ids.data_ptr(), dist.data_ptr(), ns, nq, k,
                                       oi.data_ptr(), od.data_ptr(), st))
    return oi, od


def merge_keyed_dev(ids, dist, order, out=None):
    """[nshard][nq][k] (global id, distance, order) of the shards of ONE IVF index -> [nq][k] by (distance, order)."""
    import torch

    assert ids.is_cuda and ids.dtype == torch.int32 and dist.dtype == torch.float32 and order.dtype == torch.int32
    assert ids.dim() == 3 and ids.shape == dist.shape == order.shape
    ids, dist, order = ids.contiguous(), dist.contiguous(), order.contiguous()
    ns, nq, k = ids.shape
    oi = torch.empty((nq, k), dtype=torch.int32, device=ids.device) if out is None else out[0]
    od = torch.empty((nq, k), dtype=torch.float32, device=ids.device) if out is None else out[1]
    st = torch.cuda.current_stream(ids.device).cuda_stream
    check(lib().hnswgpu_merge_keyed_dev(ids.device.index or 0, ids.data_ptr(), dist.data_ptr(), order.data_ptr(), ns, nq,
                                        k, oi.data_ptr(), od.data_ptr(), st))
    return oi, od


def merge_lists_dev(ids, dist, k, out=None):
    """[nlists][nq][k_in] torch CUDA tensors (ids -1 padded) -> the k best of every query, [nq][k];
    ties keep the lower list, then the lower rank, first (a stable sort of the concatenation)."""
    import torch

    assert ids.is_cuda and ids.dtype == torch.int32 and dist.dtype == torch.float32 and ids.dim() == 3
    ids, dist = ids.contiguous(), dist.contiguous()
    ns, nq, kin = ids.shape
    oi = torch.empty((nq, k), dtype=torch.int32, device=ids.device) if out is None else out[0]
    od = torch.empty((nq, k), dtype=torch.float32, device=ids.device) if out is None else out[1]
    st = torch.cuda.current_stream(ids.device).cuda_stream
    check(lib().hnswgpu_merge_lists_dev(ids.device.index or 0, ids.data_ptr(), dist.data_ptr(), ns, nq, kin, k,
                                        oi.data_ptr(), od.data_ptr(), st))
    return oi, od


device_count = _native.device_count


class Group:
    """ONE index over several GPUs behind the C ABI (include/hnswgpu.h: hnswgpu_group_*): whole inverted lists of an
    IVF-FLAT index dealt to the devices, or one HNSW sub-graph per device -- the reference's search-partitioned
    (partitioned_hnsw.clj:149-196) as one call.  `devices` may name a GPU several times."""

    def __init__(self, devices, dim, metric="cosine"):
        self.devices = np.ascontiguousarray(devices, np.int32)
        self.dim = int(dim)
        self.metric = METRICS[metric]
        self._h = C.c_void_p(None)
        check(lib().hnswgpu_group_create(_p(self.devices), len(self.devices), self.dim, self.metric, C.byref(self._h)))

    def close(self):
        if self._h:
            check(lib().hnswgpu_group_destroy(self._h))
            self._h = C.c_void_p(None)

    __enter__ = lambda self: self  # noqa: E731

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def info(self):
        nd, n, kind = C.c_int32(0), C.c_int64(0), C.c_int32(0)
        rows = np.zeros(len(self.devices), np.int64)
        check(lib().hnswgpu_group_info(self._h, C.byref(nd), C.byref(n), C.byref(kind), _p(rows)))
        return {"devices": nd.value, "n": n.value, "kind": {0: None, 1: "ivf", 2: "hnsw"}[kind.value], "rows_per_device": rows}

    def set_ivf(self, base, centroids, list_off, list_ids):
        base = _queries(base, self.dim)
        centroids = _queries(centroids, self.dim)
        list_off = np.ascontiguousarray(list_off, np.int64)
        list_ids = np.ascontiguousarray(list_ids, np.int32)
        if len(list_off) != len(centroids) + 1 or len(list_ids) != len(base):
            raise ValueError("list_off must have nlist + 1 entries and list_ids one per base row")
        check(lib().hnswgpu_group_set_ivf(self._h, _p(base), len(base), _p(centroids), len(centroids), _p(list_off), _p(list_ids)))

    def hnsw_build(self, base, M=16, ef_construction=200, seed=42):
        base = _queries(base, self.dim)
        check(lib().hnswgpu_group_hnsw_build(self._h, _p(base), len(base), int(M), int(ef_construction), int(seed)))

    def _search(self, fn, Q, k, param):
        Q = _queries(Q, self.dim)
        ids = np.empty((len(Q), k), np.int32)
        d = np.empty((len(Q), k), np.float32)
        check(fn(self._h, _p(Q), len(Q), int(k), int(param), _p(ids), _p(d)))
        return ids, d

    def ivf_search(self, Q, k, nprobe):
        return self._search(lib().hnswgpu_group_ivf_search, Q, k, nprobe)

    def hnsw_search(self, Q, k, ef):
        return self._search(lib().hnswgpu_group_hnsw_search, Q, k, ef)

    def member_graph(self, i):
        """The sub-graph device i holds (export: get_graph of that sub-index)."""
        h = lib().hnswgpu_group_member(self._h, int(i))
        if not h:
            raise IndexError(i)
        ix = Index.__new__(Index)
        ix._h = C.c_void_p(h)
        ix._borrowed = True
        try:
            nn, dim, metric, hg, nl = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
            check(lib().hnswgpu_info(ix._h, C.byref(nn), C.byref(dim), C.byref(metric), C.byref(hg), C.byref(nl)))
            ix.n, ix.dim, ix.metric, ix.device = nn.value, dim.value, metric.value, int(self.devices[i])
            return ix.get_graph()
        finally:
            ix._h = C.c_void_p(None)   # borrowed: never destroyed from here, whatever get_graph did
