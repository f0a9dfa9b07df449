"""No-GPU checks of the filtered search with one allow-mask per query: the four C entry points exist, are bound and validate
their arguments before any HIP call; pack_masks; the host logic of search_batch_filtered_each against a stub index; the
names of the new counter and tuning key line up with the header."""
import ctypes
import os
import re

import numpy as np
import pytest

EACH = ["hnswgpu_exact_knn_filtered_each", "hnswgpu_exact_knn_filtered_each_dev", "hnswgpu_hnsw_search_filtered_each",
        "hnswgpu_hnsw_search_filtered_each_dev"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hnswgpu.h")


def test_each_symbols_are_exported_and_bound(native_lib):
    L = ctypes.CDLL(native_lib.SO)
    for name in EACH:
        assert hasattr(L, name), "libhnswgpu.so does not export %s" % name
        assert name in native_lib.EXPORTS and name in native_lib._SIGS
        assert getattr(native_lib.lib(), name).argtypes is not None
    single = {n: native_lib._SIGS[n.replace("_each", "")] for n in EACH}
    assert all(native_lib._SIGS[n] == single[n] for n in EACH)      # the single-mask signatures, the mask argument [nq][W]


def test_each_entry_points_check_arguments_before_any_hip_call(native_lib):
    L = native_lib.lib()
    one = ctypes.c_void_p(8)           # a non-null token; never dereferenced on these paths
    assert L.hnswgpu_exact_knn_filtered_each(None, one, 1, 1, one, one, one) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_exact_knn_filtered_each_dev(None, one, 1, 1, one, one, one, None) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_hnsw_search_filtered_each(None, one, 1, 1, 0, one, one, one, None) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_hnsw_search_filtered_each_dev(None, one, 1, 1, 0, one, one, one, None, None) == -1
    assert b"idx is null" in L.hnswgpu_last_error()


def test_version_counter_and_tuning_names_line_up_with_the_header(native_lib):
    v = native_lib.lib().hnswgpu_version()
    assert v == 104
    hdr = open(HEADER).read()
    assert int(re.search(r"#define HNSWGPU_COUNT_FILTERED_EACH_GROUPS (\d+)", hdr).group(1)) == 8
    assert int(re.search(r"#define HNSWGPU_COUNT_N (\d+)", hdr).group(1)) == 9 == len(native_lib.LAUNCH_COUNTERS)
    assert native_lib.LAUNCH_COUNTERS[8] == "filtered_each_groups"
    assert int(re.search(r"#define HNSWGPU_TUNE_FILTER_EACH_MB (\d+)", hdr).group(1)) == 62
    assert int(re.search(r"#define HNSWGPU_TUNE_COUNT (\d+)", hdr).group(1)) == 63 == len(native_lib.TUNE_KEYS)
    assert native_lib.TUNE_KEYS[62] == "FILTER_EACH_MB"
    # both are plain process state: readable and settable without a device
    assert native_lib.debug_counter("filtered_each_groups") == 0
    assert native_lib.get_tuning("FILTER_EACH_MB") is None
    native_lib.set_tuning("FILTER_EACH_MB", 1)
    assert native_lib.get_tuning("FILTER_EACH_MB") == 1
    native_lib.set_tuning("FILTER_EACH_MB", None)
    assert native_lib.get_tuning("FILTER_EACH_MB") is None


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 1000])
def test_pack_masks(n):
    from hnsw_clj_amd.engine import pack_mask, pack_masks

    rng = np.random.default_rng(n)
    bits = rng.random((5, n)) < 0.4
    bits[0] = False
    bits[1] = True
    W = (n + 31) // 32
    for src in (bits, list(bits), [np.flatnonzero(b) for b in bits], [bits[0], np.flatnonzero(bits[1]), bits[2], list(np.flatnonzero(bits[3])), bits[4]]):
        m = pack_masks(src, n)
        assert m.dtype == np.uint32 and m.shape == (5, W) and m.flags["C_CONTIGUOUS"]
        for q in range(5):
            assert np.array_equal(m[q], pack_mask(bits[q], n)), (n, q)
    assert pack_masks([], n).shape == (0, W)
    with pytest.raises(ValueError):
        pack_masks([np.ones(n + 1, bool)], n)
    with pytest.raises(ValueError):
        pack_masks([[n]], n)
    with pytest.raises(ValueError):
        pack_masks(np.ones(n, bool), n)                            # one mask is not a batch of masks


class _StubIndex:
    """Records the calls of search_batch_filtered_each; answers ids = the query's tag (its first component), distance = the call number."""

    def __init__(self, n, dim):
        self.n, self.dim, self.calls = n, dim, []

    def _answer(self, name, Q, k, masks, ef):
        self.calls.append((name, np.array(Q[:, 0], np.int64), np.array(masks, copy=True), ef))
        ids = np.repeat(np.array(Q[:, 0], np.int32)[:, None], k, axis=1)
        return ids, np.full((len(Q), k), float(len(self.calls)), np.float32)

    def exact_knn_filtered_each(self, Q, k, allow_each):
        return self._answer("scan_each", Q, k, allow_each, None)

    def hnsw_search_filtered_each(self, Q, k, allow_each, ef=0):
        return self._answer("graph_each", Q, k, allow_each, ef)

    def exact_knn_filtered(self, Q, k, allow):
        return self._answer("scan", Q, k, allow[None, :], None)

    def hnsw_search_filtered(self, Q, k, allow, ef=0):
        return self._answer("graph", Q, k, allow[None, :], ef)


class _StubGraph:
    def __init__(self, n, dim):
        self.index = _StubIndex(n, dim)
        self.ids = list(range(100, 100 + n))                        # the caller's ids


def _queries(nq, dim):
    Q = np.zeros((nq, dim), np.float32)
    Q[:, 0] = np.arange(nq)
    return Q


def test_search_batch_filtered_each_groups_by_plan_and_ef():
    from hnsw_clj_amd import engine, ultra_fast

    n, k = 1000, 10
    g = _StubGraph(n, 4)
    rng = np.random.default_rng(1)
    sparse = rng.random(n) < 0.03          # scan
    half = rng.random(n) < 0.5             # graph at ef' = max(50, ceil(30000 / p))
    third = np.zeros(n, bool)
    third[:250] = True                     # graph at ef' = 120
    nothing = np.zeros(n, bool)            # scan
    evals = []

    def pred(i):                           # the same bits as `half`, as a predicate on the caller's ids: evaluated once
        evals.append(i)
        return bool(half[i - 100])

    fns = [sparse, half, third, sparse.copy(), pred, nothing, third, pred, sparse]
    plans = [ultra_fast.filtered_plan(n, int(b.sum()), k) for b in (sparse, half, third, nothing)]
    assert [p[0] for p in plans] == ["scan", "graph", "graph", "scan"] and plans[2][1] == 120 and plans[1][1] != 120
    out = ultra_fast.search_batch_filtered_each(g, _queries(len(fns), 4), k, fns)
    assert len(evals) == n and evals == g.ids                       # one evaluation per row for the two uses of `pred`
    calls = g.index.calls
    assert sorted((c[0], c[3]) for c in calls) == sorted([("scan_each", None), ("graph_each", plans[1][1]), ("graph_each", 120)])
    by = {(c[0], c[3]): c for c in calls}
    # the scan call: queries 0, 3, 8 (sparse, equal bits packed once and adjacent) and 5 (nothing), equal masks adjacent
    _, tags, masks, _ = by[("scan_each", None)]
    assert list(tags) == [0, 3, 8, 5]
    assert all(np.array_equal(masks[i], engine.pack_mask(sparse, n)) for i in range(3)) and not masks[3].any()
    _, tags, masks, _ = by[("graph_each", plans[1][1])]
    assert list(tags) == [1, 4, 7] and all(np.array_equal(m, engine.pack_mask(half, n)) for m in masks)
    _, tags, masks, _ = by[("graph_each", 120)]
    assert list(tags) == [2, 6] and all(np.array_equal(m, engine.pack_mask(third, n)) for m in masks)
    # the original order is restored: row q carries query q's tag, as the caller's id
    assert [r[0]["id"] for r in out] == [100 + q for q in range(len(fns))]
    assert all(len(r) == k for r in out)


def test_search_batch_filtered_each_all_same_takes_the_single_mask_call():
    from hnsw_clj_amd import engine, ultra_fast

    n, k = 1000, 10
    half = np.random.default_rng(2).random(n) < 0.5
    for fns, name in (([half] * 5, "graph"), ([half, half.copy(), half, lambda i: bool(half[i - 100]), half], "graph"),
                      ([np.zeros(n, bool)] * 3, "scan")):
        g = _StubGraph(n, 4)
        out = ultra_fast.search_batch_filtered_each(g, _queries(len(fns), 4), k, fns)
        assert [c[0] for c in g.index.calls] == [name] and len(g.index.calls[0][1]) == len(fns)
        assert np.array_equal(g.index.calls[0][2][0], engine.pack_mask(fns[0], n))
        assert [r[0]["id"] for r in out] == [100 + q for q in range(len(fns))]


def test_search_batch_filtered_each_edges():
    from hnsw_clj_amd import protocol, ultra_fast

    g = _StubGraph(1000, 4)
    assert ultra_fast.search_batch_filtered_each(g, np.zeros((0, 4), np.float32), 10, []) == []
    with pytest.raises(ValueError):
        ultra_fast.search_batch_filtered_each(g, _queries(2, 4), 10, [np.ones(1000, bool)])
    with pytest.raises(ValueError):
        ultra_fast.search_batch_filtered_each(g, _queries(2, 4), 10, [np.ones(999, bool), np.ones(1000, bool)])
    assert g.index.calls == []
    e = _StubGraph(0, 4)
    assert ultra_fast.search_batch_filtered_each(e, _queries(2, 4), 10, [np.ones(0, bool)] * 2) == [[], []]
    # the protocol mirror
    a, b = np.zeros(1000, bool), np.ones(1000, bool)
    a[:30] = True
    out = protocol.GpuHnswIndex(g).search_batch_filtered(_queries(2, 4), 10, [a, b])
    assert [c[0] for c in g.index.calls] == ["graph_each", "scan_each"] or [c[0] for c in g.index.calls] == ["scan_each", "graph_each"]
    assert [r[0]["id"] for r in out] == [100, 101]
