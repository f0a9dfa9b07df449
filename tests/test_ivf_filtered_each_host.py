"""No-GPU checks of the IVF-FLAT filtered search with one allow-mask per query: the two C entry points exist, are bound with the
single-mask signatures and refuse a null handle / a null mask before any HIP call; the host logic of
ivf_flat.search_batch_filtered_each against a stub index; the expectation helper of the GPU test (ivf_each_model.py) against the
single-mask rule; and the coverage conditions the GPU test's crafted inputs are chosen for, so that its coverage asserts cannot
fail for reasons of input choice."""
import ctypes

import numpy as np
import pytest

import ivf_each_model as M

EACH = ["hnswgpu_ivf_search_filtered_each", "hnswgpu_ivf_search_filtered_each_dev"]


def test_ivf_each_symbols_are_exported_and_bound(native_lib):
    L = ctypes.CDLL(native_lib.SO)
    for name in EACH:
        assert hasattr(L, name), "libhnswgpu.so does not export %s" % name
        assert name in native_lib.EXPORTS and name in native_lib._SIGS
        assert getattr(native_lib.lib(), name).argtypes is not None
        assert native_lib._SIGS[name] == native_lib._SIGS[name.replace("_each", "")]   # the single-mask signature, the mask [nq][W]
    assert native_lib.lib().hnswgpu_version() == 104


def test_ivf_each_entry_points_check_arguments_before_any_hip_call(native_lib):
    L = native_lib.lib()
    one = ctypes.c_void_p(8)           # a non-null token; never dereferenced on these paths
    assert L.hnswgpu_ivf_search_filtered_each(None, one, 1, 1, 1, one, one, one, None) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_ivf_search_filtered_each_dev(None, one, 1, 1, 1, one, one, one, None) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_ivf_search_filtered_each(one, one, 1, 1, 1, None, one, one, None) == -1
    assert b"allow is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_ivf_search_filtered_each_dev(one, one, 1, 1, 1, None, one, one, None) == -1
    assert b"allow is null" in L.hnswgpu_last_error()


# ---- ivf_flat.search_batch_filtered_each against a stub ----------------------------------------------------------------------
class _StubHandle:
    """Records the calls; answers ids = the query's tag (its first component), distance = the call number."""

    def __init__(self, n, dim):
        self.n, self.dim, self.calls = n, dim, []

    def _answer(self, name, Q, k, masks, nprobe):
        self.calls.append((name, np.array(Q[:, 0], np.int64), None if masks is None else np.array(masks, copy=True), nprobe))
        ids = np.repeat(np.array(Q[:, 0], np.int32)[:, None], k, axis=1)
        return ids, np.full((len(Q), k), float(len(self.calls)), np.float32)

    def ivf_search_filtered_each(self, Q, k, nprobe, allow_each):
        return self._answer("each", Q, k, allow_each, nprobe)

    def ivf_search_filtered(self, Q, k, nprobe, allow):
        return self._answer("single", Q, k, allow[None, :], nprobe)

    def ivf_search_lists(self, Q, k, probes):
        return self._answer("lists", Q, k, None, probes.shape[1])


def _stub(n, dim=4):
    from hnsw_clj_amd import ivf_flat
    from hnsw_clj_amd.ultra_fast import cosine_distance_ultra

    return ivf_flat.IVFFlatIndex(_StubHandle(n, dim), list(range(100, 100 + n)), cosine_distance_ultra, 8)


def _queries(nq, dim=4):
    Q = np.zeros((nq, dim), np.float32)
    Q[:, 0] = np.arange(nq)
    return Q


def test_search_batch_filtered_each_packs_equal_masks_once_and_restores_the_order():
    from hnsw_clj_amd import engine, ivf_flat

    n, k = 1000, 10
    index = _stub(n)
    rng = np.random.default_rng(1)
    sparse, half = rng.random(n) < 0.03, rng.random(n) < 0.5
    evals = []

    def pred(i):                           # the same bits as `half`, as a predicate on the caller's ids: evaluated once
        evals.append(i)
        return bool(half[i - 100])

    fns = [sparse, half, sparse.copy(), pred, np.zeros(n, bool), pred, sparse]
    out = ivf_flat.search_batch_filtered_each(index, _queries(len(fns)), k, fns, mode="accurate")
    assert len(evals) == n and evals == index.ids                   # one evaluation per row for the two uses of `pred`
    (name, tags, masks, nprobe), = index.index.calls
    assert name == "each" and nprobe == 8                           # "accurate": 8 probes
    assert list(tags) == [0, 2, 6, 1, 3, 5, 4]                      # equal masks adjacent, in the order the masks first appear
    want = [sparse] * 3 + [half] * 3 + [np.zeros(n, bool)]
    assert masks.dtype == np.uint32 and masks.shape == (7, (n + 31) // 32)
    assert all(np.array_equal(masks[i], engine.pack_mask(want[i], n)) for i in range(7))
    assert [r[0]["id"] for r in out] == [100 + q for q in range(len(fns))]   # row q carries query q's tag, as the caller's id
    assert all(len(r) == k for r in out)
    # a non-preset mode: num_probes
    index.index.calls.clear()
    ivf_flat.search_batch_filtered_each(index, _queries(2), k, [sparse, half], mode=None, num_probes=3)
    assert [(c[0], c[3]) for c in index.index.calls] == [("each", 3)]


def test_search_batch_filtered_each_all_equal_takes_the_single_mask_call():
    from hnsw_clj_amd import engine, ivf_flat

    n, k = 1000, 10
    half = np.random.default_rng(2).random(n) < 0.5
    for fns in ([half] * 5, [half, half.copy(), half, lambda i: bool(half[i - 100]), half], [np.zeros(n, bool)] * 3):
        index = _stub(n)
        out = ivf_flat.search_batch_filtered_each(index, _queries(len(fns)), k, fns)
        (name, tags, masks, nprobe), = index.index.calls
        assert name == "single" and len(tags) == len(fns) and nprobe == 4          # "balanced"
        assert np.array_equal(masks[0], engine.pack_mask(fns[0] if not callable(fns[0]) else half, n))
        assert [r[0]["id"] for r in out] == [100 + q for q in range(len(fns))]


def test_search_batch_filtered_each_without_routing_post_filters_per_query():
    from hnsw_clj_amd import ivf_flat, protocol

    n, k = 1000, 10
    index = _stub(n)
    a, b = np.zeros(n, bool), np.ones(n, bool)
    a[:3] = True                                                    # passes the tags 0, 1, 2 (ids 100 .. 102)
    out = ivf_flat.search_batch_filtered_each(index, _queries(4), k, [a, b, a, b], mode="turbo")
    (name, tags, masks, nprobe), = index.index.calls
    assert name == "lists" and list(tags) == [0, 1, 2, 3] and nprobe == 1          # search 3k ...
    assert [len(r) for r in out] == [k, k, k, k] and [r[0]["id"] for r in out] == [100, 101, 102, 103]
    out = ivf_flat.search_batch_filtered_each(index, _queries(4)[::-1].copy(), k, [a, b, a, b], mode="turbo")
    assert [len(r) for r in out] == [0, k, k, k]                    # ... keep what passes for THIS query: tag 3 fails mask a
    # edges and the protocol mirror
    assert ivf_flat.search_batch_filtered_each(index, np.zeros((0, 4), np.float32), k, []) == []
    with pytest.raises(ValueError):
        ivf_flat.search_batch_filtered_each(index, _queries(2), k, [a])
    with pytest.raises(ValueError):
        ivf_flat.search_batch_filtered_each(index, _queries(2), k, [np.ones(999, bool), b])
    index.index.calls.clear()
    res = protocol.GpuIvfFlatIndex(index).search_batch_filtered(_queries(2), k, [a, b])
    assert [c[0] for c in index.index.calls] == ["each"] and [r[0]["id"] for r in res] == [100, 101]
    assert not protocol.supports_filtering(protocol.GpuIvfFlatIndex(index))


# ---- the expectation helper against the single-mask rule ---------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_expect_each_with_one_shared_mask_is_the_single_mask_expectation(oracle, metric):
    from hnsw_clj_amd import datagen

    O = oracle
    o_metric = M.om(O, metric)
    n, dim, nlist, nprobe, k = 300, 24, 5, 3, 20
    base = datagen.generate_dataset(n, dim)
    Q = datagen.generate_dataset(9, dim, seed=43)
    cen, off, lids = M.lists(O, base, nlist, o_metric)
    bits = np.random.default_rng(3).random(n) < 0.1                 # short results for some queries
    si, sd, _ = M.expect_single(O, base, cen, off, lids, Q, bits, nprobe, o_metric, k)
    assert (si >= 0).any() and (si == -1).any()
    for masks, which in (([bits], np.zeros(9, int)), ([bits, bits.copy(), bits.copy()], M.deal(9, 3))):
        ei, ed = M.expect_each(O, base, cen, off, lids, Q, masks, which, nprobe, o_metric, k)
        assert np.array_equal(ei, si) and np.array_equal(ed, sd)
    # and with two different masks every row is its own mask's single expectation
    other = ~bits
    ei, ed = M.expect_each(O, base, cen, off, lids, Q, [bits, other], M.deal(9, 2), nprobe, o_metric, k)
    oi, od, _ = M.expect_single(O, base, cen, off, lids, Q, other, nprobe, o_metric, k)
    assert np.array_equal(ei[0::2], si[0::2]) and np.array_equal(ei[1::2], oi[1::2])
    assert np.array_equal(ed[0::2], sd[0::2]) and np.array_equal(ed[1::2], od[1::2])
    assert bits[ei[0::2][ei[0::2] >= 0]].all() and other[ei[1::2][ei[1::2] >= 0]].all()


def test_garbage_past_n_touches_only_the_bits_past_n():
    from hnsw_clj_amd.engine import pack_masks

    for n in (33, 64, 70, 1000):
        bits = np.random.default_rng(n).random((5, n)) < 0.5
        m = pack_masks(bits, n)
        g = M.garbage_past_n(m, n, 7)
        assert g.shape == m.shape and g.dtype == np.uint32
        keep = np.uint32((1 << (n & 31)) - 1) if n & 31 else np.uint32(0xFFFFFFFF)
        assert np.array_equal(g[:, :-1], m[:, :-1]) and np.array_equal(g[:, -1] & keep, m[:, -1] & keep)
        assert (n & 31 == 0) == np.array_equal(g, m)


# ---- the coverage conditions of the GPU test's crafted inputs ---------------------------------------------------------------------
def test_plan_chunks_model_on_hand_computed_cases():
    # 20000 x 32 in 2 lists, one query: the derivation in the GPU test's comment
    assert M.rb_of(32) == 8 and M.rb_of(768) == 8 and M.rb_of(1536) == 4 and M.rb_of(3072) == 2
    assert M.plan_chunks(32, 10400, 10000, 2) == (64, 163)
    # the edge lists with and without SCAN_BLOCKS = 1
    assert M.plan_chunks(32, 107, 50, 18) == (32, 4)
    assert M.plan_chunks(32, 107, 50, 18, scan_blocks=1) == (128, 1)
    assert M.plan_chunks(32, 808, 450, 2, scan_blocks=1) == (832, 1)


def test_the_edge_inputs_cover_what_the_gpu_test_relies_on():
    E = M.edge_case()
    rb = M.rb_of(E.dim)
    assert rb == 8                                                  # dim 32: one 256-float chunk per row, 8 register rows
    assert list(np.diff(E.off)) == [1, 63, 64, 65, 0, 107] and E.nprobe == E.nlist == 6   # every list probed, the empty one too
    assert sorted(E.lids.tolist()) == list(range(E.n))
    cr, nchunks = M.plan_chunks(E.dim, 107, E.n // E.nlist, len(E.which) * E.nprobe, scan_blocks=1)
    assert nchunks == 1
    seen = set()
    for bits in E.masks:
        for l in (3, 5):                                            # the 65-row and the 107-row list
            for counts in M.wave_walks(bits[E.lids[E.off[l]:E.off[l + 1]]], cr):
                seen.update(counts)
    assert {0, 1, rb - 1, rb, rb + 1, 64} <= seen, seen
    # a list that the mask empties is probed, and fewer than k rows pass: padded results
    assert any(not bits[E.lids[E.off[l]:E.off[l + 1]]].any() for bits in E.masks for l in (0, 1, 2, 3, 5))
    assert sum(int(bits.sum()) < E.k for bits in E.masks) == 2      # A and B: short results; not A fills k
    assert any(int(bits.sum()) > 64 for bits in E.masks)            # ... and more than the register list's 64 for one mask
    # neighbouring queries hold different masks
    assert all(E.which[q] != E.which[q + 1] for q in range(len(E.which) - 1))


def test_the_long_walk_inputs_carry_flush_inside_a_block_and_flush_at_the_end():
    W = M.long_walk_case()
    rb = M.rb_of(W.dim)
    cr, nchunks = M.plan_chunks(W.dim, 808, W.n // 2, len(W.which) * 2, scan_blocks=1)
    assert (cr, nchunks) == (832, 1) and list(np.diff(W.off)) == [808, 92]
    walks = M.wave_walks(W.masks[0][W.lids[W.off[0]:W.off[1]]], cr)
    assert walks[0] == [3, 0, 7, 2]                                 # wave 0: the blocks 0, 4, 8 and 12 (40 positions) of the list
    assert M.walk_events(walks[0], rb) == (1, 3, 4)                 # one step inside a block that began with leftovers, three carries, a flush of 4
    assert all(M.walk_events(w, rb)[2] > 0 for w in walks)          # every wave ends on a clamped flush
    # with the default chunks no wave walks more than one block: the same masks then run the flush-only path
    cr, nchunks = M.plan_chunks(W.dim, 808, W.n // 2, len(W.which) * 2)
    assert cr < 256 and max(len(w) for w in M.wave_walks(W.masks[0][W.lids[W.off[0]:W.off[1]]], cr)) == 1


def test_the_parity_batches_hold_complementary_neighbours_and_short_results():
    for nq in (12, 70):
        which = M.deal(nq, len(M.PARITY_MASKS))
        names = [M.PARITY_MASKS[m] for m in which]
        pairs = set(zip(names, names[1:]))
        assert ("ones", "zeros") in pairs and ("half", "not_half") in pairs     # a kernel reading mask q +- 1 returns a failing row
        assert "zeros" in names                                                    # that query's result is all padding: seen_short > 0
