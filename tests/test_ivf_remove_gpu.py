"""hnswgpu_ivf_remove on the device: a handle that shrank is indistinguishable, bit for bit, from a fresh handle over the kept rows
in their old order that was given the same centroids and the compacted lists (ivf_remove_model.compact_lists) through set_ivf --
get_ivf exactly, every search's ids and distance BITS, norms, the saved file's bytes.  And between two device paths, neither of
them the fresh handle: a removal is the permanent form of the allow-mask of the filtered search.  No tolerance anywhere."""
import ctypes
import threading

import numpy as np
import pytest

import ivf_remove_model as R
from ivf_add_model import f64_distances, merged_lists

pytestmark = pytest.mark.gpu

N0, NLIST, NQ = 3001, 16, 64   # 3001 rows: 12 chunks of 256 list positions and 94 mask words, the last of each partial
STEP_SECONDS = 60              # the time limit of one step of the threaded test
_DATA = {}


def _data(O, dim, n=N0 + 400):
    """(rows f32 [n, dim], queries f32 [NQ, dim]): clustered, from the oracle's generator; made once per shape."""
    if (dim, n) not in _DATA:
        rows = O.generate_dataset(n + NQ, dim, "clustered", num_clusters=10, noise_level=0.1, seed=7).astype(np.float32)
        _DATA[(dim, n)] = (np.ascontiguousarray(rows[:n]), np.ascontiguousarray(rows[n:]))
    return _DATA[(dim, n)]


def _bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


def _same(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=what + ": ids")
    np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]), err_msg=what + ": distance bits")


def _native_n(ix):
    """the handle's own row count (hnswgpu_info), beside engine.Index.n"""
    from hnsw_clj_amd import _native

    n = ctypes.c_int64(-1)
    assert _native.lib().hnswgpu_info(ix._h, ctypes.byref(n), None, None, None, None) == 0
    return n.value


def _device_assign(engine, tune, rows, metric, cen):
    """The nearest list of every row in the GEMV order: kmeans_assign on a fresh handle with the tile path off for that call."""
    with engine.Index(rows, metric, 0) as ix:
        tune.set("TILE", 0)
        try:
            a, _ = ix.kmeans_assign(cen)
        finally:
            tune.restore()
    return a


def _fresh(engine, rows, metric, mode, cen, off, ids, stream_state=None):
    ix = engine.Index(rows, metric, 0)
    if mode is not None:                                    # None: the mode new handles get
        ix.set_rejection_test(mode)
    ix.set_ivf(cen, off, ids)
    if stream_state is not None:
        ix.ivf_set_stream_state(stream_state)
    return ix


def _assert_same_ivf(ix, cen, off, ids, what=""):
    c, o, i = ix.get_ivf()
    np.testing.assert_array_equal(_bits(c), _bits(cen), err_msg=what + ": centroids moved")
    np.testing.assert_array_equal(o, off, err_msg=what + ": list_off")
    np.testing.assert_array_equal(i, ids, err_msg=what + ": list_ids")


def _remove(ix, gone):
    """ivf_remove, its `kept`, n and the handle's own n against the model; returns kept."""
    n = ix.n
    want = R.kept(n, gone)
    kept = ix.ivf_remove(gone)
    assert kept.dtype == np.int64
    np.testing.assert_array_equal(kept, want)
    assert ix.n == len(want) and _native_n(ix) == len(want)
    return kept


def _assert_same_answers(engine, shrunk, fresh, Q, seed=5):
    """Everything a search reads, through every entry point that reads it."""
    n1 = shrunk.n
    assert fresh.n == n1 and _native_n(shrunk) == n1
    for nq in (1, 5, 64):
        for nprobe in (1, 4, 16):
            if nprobe > shrunk.nlist:
                continue
            _same(shrunk.ivf_search(Q[:nq], 10, nprobe), fresh.ivf_search(Q[:nq], 10, nprobe), "ivf_search nq %d nprobe %d" % (nq, nprobe))
    nl = shrunk.nlist
    probes = np.array([[0, -1, nl - 1], [nl - 1, nl // 2, -1], [-1, -1, 1 % nl], [nl // 3, (nl // 3 + 1) % nl, 0],
                       [-1, -1, -1]], np.int32)
    _same(shrunk.ivf_search_lists(Q[:5], 10, probes), fresh.ivf_search_lists(Q[:5], 10, probes), "ivf_search_lists")
    rng = np.random.default_rng(seed)
    for name, bits in (("half", rng.random(n1) < 0.5), ("ones", np.ones(n1, np.bool_))):
        mask = engine.pack_mask(bits, n1)
        _same(shrunk.ivf_search_filtered(Q[:5], 10, min(4, nl), mask), fresh.ivf_search_filtered(Q[:5], 10, min(4, nl), mask),
              "ivf_search_filtered " + name)
    _same(shrunk.exact_knn(Q[:5], 10), fresh.exact_knn(Q[:5], 10), "exact_knn")
    np.testing.assert_array_equal(_bits(shrunk.norms()), _bits(fresh.norms()), err_msg="norms")
    at = np.array([n1 // 3, n1 - 1, n1 // 2, 0], np.int32)
    np.testing.assert_array_equal(_bits(shrunk.batch_distances(Q[0], ids=at)), _bits(fresh.batch_distances(Q[0], ids=at)),
                                  err_msg="batch_distances")


# ---- 1. shrunk equals fresh -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2"])
@pytest.mark.parametrize("dim", [64, 136])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_shrunken_handle_equals_fresh_handle(native_lib, oracle, tmp_path, metric, dim, mode):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, dim)
    rng = np.random.default_rng(31)
    with engine.Index(rows[:N0], metric, 0) as shrunk:
        shrunk.set_rejection_test(mode)
        shrunk.ivf_build(NLIST, 3, 42)
        cen, off, ids = shrunk.get_ivf()
        present = np.arange(N0)                              # the original row of every present row
        for m in (1, 63, 64, 65, 257, 600):
            gone = rng.choice(shrunk.n, m, replace=False).astype(np.int32)   # unsorted, in the current numbering
            if m == 65:
                gone = np.concatenate([gone, gone[:20], gone[3:4]])          # some ids named twice, one three times
            off, ids = R.compact_lists(off, ids, gone)
            present = present[_remove(shrunk, gone)]
            _assert_same_ivf(shrunk, cen, off, ids, "after m %d" % m)
        assert shrunk.n == N0 - (1 + 63 + 64 + 65 + 257 + 600)
        with _fresh(engine, rows[present], metric, mode, cen, off, ids, shrunk.ivf_stream_state()) as fresh:
            _assert_same_answers(engine, shrunk, fresh, Q)
            fa, fb = tmp_path / "shrunk.idx", tmp_path / "fresh.idx"
            shrunk.save(fa)
            fresh.save(fb)
            assert fa.read_bytes() == fb.read_bytes(), "the saved files differ"
            with engine.Index.load(fa, 0) as back:
                assert back.n == len(present)
                _assert_same_ivf(back, cen, off, ids, "loaded")
                _same(back.ivf_search(Q, 10, 4), fresh.ivf_search(Q, 10, 4), "loaded file")


# ---- 2. the permanent form of the filter ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_removal_is_the_permanent_form_of_the_filter(native_lib, oracle, metric):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, 64)
    rng = np.random.default_rng(32)
    gone = rng.choice(N0, 900, replace=False)
    new_id = R.rank(N0, gone)
    with engine.Index(rows[:N0], metric, 0) as ix:
        ix.ivf_build(NLIST, 3, 42)
        mask = engine.pack_mask(new_id >= 0, N0)
        before = [ix.ivf_search_filtered(Q[:nq], 10, 4, mask) for nq in (1, 5, 64)]
        _remove(ix, gone)
        ones = engine.pack_mask(np.ones(ix.n, np.bool_), ix.n)
        for nq, (bi, bd) in zip((1, 5, 64), before):
            ai, ad = ix.ivf_search_filtered(Q[:nq], 10, 4, ones)
            assert (bi >= 0).all()
            np.testing.assert_array_equal(ai, new_id[bi], err_msg="nq %d: ids through the rank" % nq)
            np.testing.assert_array_equal(_bits(ad), _bits(bd), err_msg="nq %d: distance bits" % nq)


# ---- 3. split independence ------------------------------------------------------------------------------------------------
def test_lists_do_not_depend_on_how_the_removal_was_split(native_lib, oracle):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, 64)
    rng = np.random.default_rng(33)
    gone = rng.choice(N0, 400, replace=False)
    with engine.Index(rows[:N0], "cosine", 0) as one, engine.Index(rows[:N0], "cosine", 0) as many:
        one.ivf_build(NLIST, 3, 42)
        cen, off0, ids0 = one.get_ivf()
        many.set_ivf(cen, off0, ids0)
        _remove(one, gone)
        present = np.arange(N0)
        for at in range(0, len(gone), 7):
            now = np.full(N0, -1, np.int64)
            now[present] = np.arange(len(present))           # original row -> its id in the current numbering
            present = present[_remove(many, now[gone[at:at + 7]])]
        c1, o1, i1 = one.get_ivf()
        _assert_same_ivf(many, c1, o1, i1)
        assert o1[-1] == N0 - 400 and sorted(i1.tolist()) == list(range(N0 - 400))
        for nq in (1, 64):
            _same(many.ivf_search(Q[:nq], 10, 4), one.ivf_search(Q[:nq], 10, 4), "split, nq %d" % nq)


# ---- 4. edges -------------------------------------------------------------------------------------------------------------
def _edge_base(seed=3, n0=200, dim=64):
    """200 x 64 over 4 centroids, lists 2 and 3 empty (the base of test_ivf_add_gpu.py's placement edges)"""
    rng = np.random.default_rng(seed)
    cen = (4.0 * rng.standard_normal((4, dim))).astype(np.float32)
    cen[2] = cen[1]                                        # two identical centroids: the lower index wins every tie
    base = (cen[rng.integers(0, 2, n0)] + 0.1 * rng.standard_normal((n0, dim))).astype(np.float32)
    a0 = f64_distances("l2", base, cen).argmin(axis=1)     # (argmin: the first minimum)
    assert set(a0.tolist()) == {0, 1}
    order = np.argsort(a0, kind="stable").astype(np.int32)
    off0 = np.zeros(5, np.int64)
    off0[1:] = np.cumsum(np.bincount(a0, minlength=4))
    return cen, base, off0, order, a0


@pytest.mark.parametrize("case", ["list0", "list1", "first_then_last", "last_word"])
def test_edges_of_the_lists(native_lib, case):
    from hnsw_clj_amd import engine

    cen, base, off0, ids0, _ = _edge_base()
    n = len(base)
    steps = {"list0": [ids0[off0[0]:off0[1]][::-1]], "list1": [ids0[off0[1]:off0[2]]],
             "first_then_last": [np.array([0]), np.array([n - 2])],          # (n - 2: the last row once row 0 has left)
             "last_word": [np.arange(192, 200)]}[case]
    with engine.Index(base, "l2", 0) as ix:
        ix.set_ivf(cen, off0, ids0)
        off, ids, present = off0, ids0, np.arange(n)
        for gone in steps:
            off, ids = R.compact_lists(off, ids, gone)
            present = present[_remove(ix, gone)]
            _assert_same_ivf(ix, cen, off, ids, case)
        if case == "list0":
            assert off[0] == off[1] == 0 and off[2] == len(present) > 0
        if case == "list1":
            assert off[1] == off[2] == off[4] == len(present) > 0
        if case == "first_then_last":
            assert present.tolist() == list(range(1, n - 1))
        with _fresh(engine, base[present], "l2", None, cen, off, ids) as fresh:
            _assert_same_answers(engine, ix, fresh, base[present][:64])


def test_to_nothing_and_back(native_lib):
    from hnsw_clj_amd import engine

    cen, base, off0, ids0, a0 = _edge_base()
    n = len(base)
    rng = np.random.default_rng(34)
    with engine.Index(base, "l2", 0) as ix:
        ix.set_ivf(cen, off0, ids0)
        kept = _remove(ix, rng.permutation(n))
        assert len(kept) == 0 and ix.n == 0 and ix.nlist == 4
        c, o, i = ix.get_ivf()
        np.testing.assert_array_equal(_bits(c), _bits(cen))
        assert o.shape == (5,) and not o.any() and i.shape == (0,)
        with _fresh(engine, np.zeros((0, 64), np.float32), "l2", None, cen, np.zeros(5, np.int64), np.zeros(0, np.int32)) as empty:
            for nq in (1, 5):
                gi, gd = ix.ivf_search(base[:nq], 10, 4)
                assert (gi == -1).all() and np.isposinf(gd).all()
                _same((gi, gd), empty.ivf_search(base[:nq], 10, 4), "the emptied handle, nq %d" % nq)
            probes = np.array([[0, 1, -1]], np.int32)
            _same(ix.ivf_search_lists(base[:1], 10, probes), empty.ivf_search_lists(base[:1], 10, probes), "emptied, given lists")
        got = ix.ivf_add(base)                               # ... and grown again
        np.testing.assert_array_equal(got, np.arange(n, dtype=np.int32))
        off, ids = merged_lists(np.zeros(5, np.int64), np.zeros(0, np.int32), a0)
        _assert_same_ivf(ix, cen, off, ids, "grown again from nothing")
        with _fresh(engine, base, "l2", None, cen, off, ids) as fresh:
            _assert_same_answers(engine, ix, fresh, base[:64])


def test_one_list(native_lib):
    from hnsw_clj_amd import engine

    rng = np.random.default_rng(2)
    base = rng.standard_normal((100, 64)).astype(np.float32)
    cen = base.mean(axis=0, keepdims=True).astype(np.float32)
    ids0 = np.arange(99, -1, -1, dtype=np.int32)
    gone = np.array([99, 0, 50, 64, 63], np.int32)
    with engine.Index(base, "cosine", 0) as ix:
        ix.set_ivf(cen, [0, 100], ids0)
        kept = _remove(ix, gone)
        off, ids = R.compact_lists([0, 100], ids0, gone)
        assert ids.tolist() == list(range(94, -1, -1)) and off.tolist() == [0, 95]
        _assert_same_ivf(ix, cen, off, ids)
        with _fresh(engine, base[kept], "cosine", None, cen, off, ids) as fresh:
            _same(ix.ivf_search(base[:5], 10, 1), fresh.ivf_search(base[:5], 10, 1), "one list")
            _same(ix.exact_knn(base[:5], 10), fresh.exact_knn(base[:5], 10), "one list, exact")


# ---- 5. a handle whose lists are its base rows in place --------------------------------------------------------------------
def test_alias_handle_stays_in_place(native_lib, oracle, tune):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, 64)
    with engine.Index(rows[:N0], "cosine", 0) as b:
        b.ivf_build(NLIST, 3, 42)
        cen, off0, ids_b = b.get_ivf()
    base = np.ascontiguousarray(rows[:N0][ids_b])           # the base in list order: identity list_ids
    ident = np.arange(N0, dtype=np.int32)
    last = int(np.flatnonzero(np.diff(off0) > 0)[-1])       # the last list with members
    rng = np.random.default_rng(4)
    tail = (cen[last][None, :] * (1.0 + 0.001 * rng.standard_normal((40, 64)))).astype(np.float32)
    gone = rng.choice(N0, 333, replace=False)
    for new, stays_identity in ((rows[N0:], False), (tail, True)):
        with engine.Index(base, "cosine", 0) as ix:
            ix.set_ivf(cen, off0, ident)
            kept = _remove(ix, gone)
            off, ids = R.compact_lists(off0, ident, gone)
            np.testing.assert_array_equal(ids, np.arange(len(kept), dtype=np.int32))
            _assert_same_ivf(ix, cen, off, ids, "alias")
            assert off[-1] == N0 - 333
            with _fresh(engine, base[kept], "cosine", None, cen, off, ids) as fresh:
                _assert_same_answers(engine, ix, fresh, Q)
            # ... and a following ivf_add: in place while the merged lists are the identity, copies of its own otherwise
            everything = np.concatenate([base[kept], new])
            assign = _device_assign(engine, tune, everything, "cosine", cen)[len(kept):]
            off2, ids2 = merged_lists(off, ids, assign)
            assert (ids2 == np.arange(len(ids2))).all() == stays_identity
            ix.ivf_add(new[:17])
            ix.ivf_add(new[17:])
            _assert_same_ivf(ix, cen, off2, ids2, "alias, grown")
            with _fresh(engine, everything, "cosine", None, cen, off2, ids2) as fresh:
                _assert_same_answers(engine, ix, fresh, Q)


# ---- 6. add and remove interleaved ----------------------------------------------------------------------------------------
def test_add_and_remove_interleaved(native_lib, oracle, tune):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, 136)
    rng = np.random.default_rng(6)
    with engine.Index(rows[:N0], "cosine", 0) as ix:
        ix.set_rejection_test(2)
        ix.ivf_build(NLIST, 3, 42)
        cen, off, ids = ix.get_ivf()
        assign = _device_assign(engine, tune, rows, "cosine", cen)
        ix.ivf_add(rows[N0:N0 + 300])
        off, ids = merged_lists(off, ids, assign[N0:N0 + 300])
        gone = np.concatenate([rng.choice(N0, 120, replace=False), N0 + rng.choice(300, 80, replace=False)])   # old and new rows
        off, ids = R.compact_lists(off, ids, gone)
        present = np.arange(N0 + 300)[_remove(ix, gone)]
        ix.ivf_add(rows[N0 + 300:N0 + 400])
        off, ids = merged_lists(off, ids, assign[N0 + 300:N0 + 400])
        present = np.concatenate([present, np.arange(N0 + 300, N0 + 400)])
        gone = np.array([len(present) - 50], np.int32)
        off, ids = R.compact_lists(off, ids, gone)
        present = present[_remove(ix, gone)]
        assert ix.n == len(present) == N0 + 400 - 201
        _assert_same_ivf(ix, cen, off, ids)
        with _fresh(engine, rows[present], "cosine", 2, cen, off, ids, ix.ivf_stream_state()) as fresh:
            _assert_same_answers(engine, ix, fresh, Q)


# ---- 7. the first-search verdict of a mode-1 handle is kept ---------------------------------------------------------------
def test_mode_1_verdict_is_kept(native_lib, oracle):
    from hnsw_clj_amd import engine

    n0 = 5000
    rows, Q = _data(oracle, 128, n0)
    rng = np.random.default_rng(7)
    with engine.Index(rows, "cosine", 0) as ix:
        ix.set_rejection_test(1)
        ix.ivf_build(NLIST, 3, 42)
        cen, off, ids = ix.get_ivf()
        verdict = ix.ivf_stream_state()
        gone = rng.choice(n0, 500, replace=False)
        off, ids = R.compact_lists(off, ids, gone)
        present = np.arange(n0)[_remove(ix, gone)]
        assert ix.ivf_stream_state() == verdict
        _assert_same_ivf(ix, cen, off, ids)
        with _fresh(engine, rows[present], "cosine", 1, cen, off, ids, verdict) as fresh:
            _assert_same_answers(engine, ix, fresh, Q)
        # ... kept, not measured again: an installed verdict that the handle's own measurement would not give survives too
        ix.ivf_set_stream_state(1 - verdict)
        gone = rng.choice(ix.n, 300, replace=False)
        off, ids = R.compact_lists(off, ids, gone)
        present = present[_remove(ix, gone)]
        assert ix.ivf_stream_state() == 1 - verdict
        with _fresh(engine, rows[present], "cosine", 1, cen, off, ids, 1 - verdict) as fresh:
            _assert_same_answers(engine, ix, fresh, Q)


# ---- 8. refusals leave the handle alone -----------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone(native_lib, oracle):
    from hnsw_clj_amd import engine

    L = native_lib.lib()
    rows, Q = _data(oracle, 64)
    base = rows[:500]

    def ids(*v):
        a = np.array(v, np.int32)
        return a, a.ctypes.data_as(ctypes.c_void_p)

    one, ptr = ids(3)

    def state(ix):
        return ix.get_ivf(), ix.ivf_search(Q[:5], 10, 4)

    def unchanged(ix, before, what):
        assert ix.n == 500 and _native_n(ix) == 500
        lists, answer = state(ix)
        assert all(np.array_equal(x, y) for x, y in zip(lists, before[0])), what
        _same(answer, before[1], what)

    def refused(ix, p, m, code, word=None, before=None):
        out = ctypes.c_int64(-7)
        assert L.hnswgpu_ivf_remove(ix._h, p, m, ctypes.byref(out)) == code
        assert out.value == (500 if code == 0 else -7)        # a refusal does not write n_after
        if word:
            assert word in L.hnswgpu_last_error().lower()
        if before is not None:                                # every refusal leaves n, the lists and a search's bits alone
            unchanged(ix, before, "after a refusal with code %d (%s)" % (code, word))

    with engine.Index(base, "cosine", 0) as bare:
        refused(bare, ptr, 1, -3, b"no ivf lists")
        refused(bare, None, 0, 0)                             # nothing to remove: nothing is looked at
        refused(bare, ptr, 0, 0)
        assert bare.n == 500 and bare.nlist == 0
    with engine.Index(base, "cosine", 0) as ix:
        ix.ivf_build(8, 2, 42)
        before = state(ix)
        cen, off, lids = before[0]
        refused(ix, None, 1, -1, b"rows is null", before)
        refused(ix, ptr, -1, -1, None, before)
        for bad in (-1, 500):
            arr, p = ids(3, 4, bad, 5)
            refused(ix, p, 4, -1, b"rows[2]", before)         # the message names the position
        refused(ix, ptr, 0, 0, None, before)                  # nothing to remove: nothing happens
        refused(ix, None, 0, 0, None, before)
        assert L.hnswgpu_ivf_remove(ix._h, None, 0, None) == 0    # n_after may be null
        out = ctypes.c_int64(-7)                              # lsh_remove still refuses a handle with lists
        ix.lsh_build(8, 6, 64, 42)
        assert L.hnswgpu_lsh_remove(ix._h, ptr, 1, ctypes.byref(out)) == -3 and out.value == -7
        assert b"ivf lists" in L.hnswgpu_last_error().lower()
        refused(ix, ptr, 1, -3, b"lsh tables", before)
    with engine.Index(base, "cosine", 0) as graph:
        graph.set_ivf(cen, off, lids)
        graph.hnsw_build(8, 40, 42)
        refused(graph, ptr, 1, -3, b"graph", before)
    with engine.Index(base, "cosine", 0) as forest:
        forest.hnsw_build_parts([0, 250, 500], 8, 40, 42)
        forest.set_ivf(cen, off, lids)
        refused(forest, ptr, 1, -3, b"forest", before)
    with engine.Index(base, "cosine", 0) as shard:
        shard.set_ivf_shard(cen, off, lids, np.diff(off) + 3)
        shard_before = state(shard)
        refused(shard, ptr, 1, -3, b"shard", shard_before)
    with engine.Index(base, "cosine", 0) as ix:               # ... and n_after null on a call that removes
        ix.set_ivf(cen, off, lids)
        assert L.hnswgpu_ivf_remove(ix._h, ptr, 1, None) == 0
        assert _native_n(ix) == 499


# ---- 9. searches beside removals ------------------------------------------------------------------------------------------
def test_searches_beside_removals_see_one_of_the_index_states(native_lib, oracle):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, 64)
    n0, step = N0, 300
    rng = np.random.default_rng(8)
    qs = [np.ascontiguousarray(Q[3 * t:3 * t + 3]) for t in range(4)]
    removals, present = [], [np.arange(n0)]                 # each removal in the numbering current at its turn
    for _ in range(3):
        removals.append(rng.choice(len(present[-1]), step, replace=False))
        present.append(present[-1][R.kept(len(present[-1]), removals[-1])])
    with engine.Index(rows[:n0], "l2", 0) as ix:
        ix.ivf_build(NLIST, 3, 42)
        cen, off, ids = ix.get_ivf()
        states = []                                         # per index state, per thread: (ids, distance bits), from fresh handles
        for s, now in enumerate(present):
            if s > 0:
                off, ids = R.compact_lists(off, ids, removals[s - 1])
            with _fresh(engine, rows[now], "l2", None, cen, off, ids) as fresh:
                states.append([(i, _bits(d)) for i, d in (fresh.ivf_search(q, 10, 4) for q in qs)])
        stop, errors, seen = threading.Event(), [], [set() for _ in range(4)]

        def matches(t, i, d):
            return [s for s in range(4) if np.array_equal(i, states[s][t][0]) and np.array_equal(_bits(d), states[s][t][1])]

        def searcher(t):
            try:
                for _ in range(20000):                      # bounded: the remover sets `stop` long before
                    if stop.is_set():
                        break
                    hit = matches(t, *ix.ivf_search(qs[t], 10, 4))
                    if not hit:
                        raise AssertionError("thread %d: an answer that belongs to none of the four index states" % t)
                    seen[t].update(hit)
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
                stop.set()

        def remover():
            try:
                for s, gone in enumerate(removals):
                    if stop.is_set():
                        return
                    ix.ivf_remove(gone)
                    for t in range(4):                      # the shrunken index is what every later search sees
                        assert s + 1 in matches(t, *ix.ivf_search(qs[t], 10, 4))
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
            finally:
                stop.set()

        threads = [threading.Thread(target=searcher, args=(t,), daemon=True) for t in range(4)]
        threads.append(threading.Thread(target=remover, daemon=True))
        for th in threads:
            th.start()
        for th in threads:
            th.join(STEP_SECONDS)
            assert not th.is_alive(), "a thread did not finish within its time limit"
        assert not errors, errors[0]
        assert ix.n == len(present[-1])
        assert all(3 in matches(t, *ix.ivf_search(qs[t], 10, 4)) for t in range(4))


# ---- 10. the Python mirror ------------------------------------------------------------------------------------------------
def test_python_mirror_remove_vectors(native_lib, oracle):
    from hnsw_clj_amd import ivf_flat

    rows, _ = _data(oracle, 64)
    n0 = 600
    index = ivf_flat.build_index([("v-%d" % i, rows[i]) for i in range(n0)], num_partitions=8, max_iterations=2)
    try:
        assert ivf_flat.search_knn(index, rows[33], 5, mode="precise")[0]["id"] == "v-33"
        assert ivf_flat.remove_vectors(index, ["v-33", "v-0", "v-599"]) is index
        assert ivf_flat.index_info(index)["vectors"] == n0 - 3 and len(index.ids) == n0 - 3
        assert all(r["id"] not in ("v-33", "v-0", "v-599") for r in ivf_flat.search_knn(index, rows[33], 10, mode="precise"))
        res = ivf_flat.search_knn(index, rows[34], 5, mode="precise")
        assert res[0]["id"] == "v-34" and abs(res[0]["distance"]) <= 1e-5
        with pytest.raises(KeyError):
            ivf_flat.remove_vectors(index, ["v-1", "v-33"])
        assert len(index.ids) == n0 - 3 and index.index.n == n0 - 3
        ivf_flat.add_vectors(index, [("w-0", rows[700])])
        assert ivf_flat.search_knn(index, rows[700], 5, mode="precise")[0]["id"] == "w-0"
    finally:
        index.close()
