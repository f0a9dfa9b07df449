"""hnswgpu_hnsw_remove on the device: the graph a removal leaves equals the numpy model (hnsw_remove_model.py) EDGE FOR EDGE, and
the shrunken handle is indistinguishable, bit for bit, from a fresh handle over the kept rows that was given the model's graph
through set_graph -- norms, distances, rejection bounds, every search's ids, distance BITS and stats.  No tolerance anywhere."""
import ctypes
import threading

import numpy as np
import pytest

import hnsw_build_model as H
import hnsw_remove_model as R
import lsh_remove_model as LR

pytestmark = pytest.mark.gpu

N0, M, EFC, SEED = 600 + 7, 8, 48, 42      # 607 rows: 19 mask words, the last of 31 rows; no multiple of 32
STEP_SECONDS = 60                          # the time limit of one step of the threaded test
_ROWS, _MODELS = {}, {}


def _rows(O, dim):
    """(rows f32 [N0 + 300, dim], queries f32 [32, dim]): hnsw_build_model.paths_data (10 clusters whose centres are rows, 20
    duplicated pairs: runs of equal distances reach the sort) + rows of the same clusters behind it; made once per dim."""
    if dim not in _ROWS:
        base = H.paths_data(O, dim)
        rs = np.random.RandomState(7 + dim)
        more = base[rs.randint(0, len(base), 307 + 32)] + 0.2 * rs.randn(307 + 32, dim).astype(np.float32)
        more[5] = base[41]                                   # one more duplicated pair, across the 600-row border
        _ROWS[dim] = (np.ascontiguousarray(np.concatenate([base, more[:307]]), np.float32), np.ascontiguousarray(more[307:], np.float32))
    return _ROWS[dim]


def _bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


def _same(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=what + ": ids")
    np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]), err_msg=what + ": distance bits")
    if len(a) > 2:
        np.testing.assert_array_equal(a[2], b[2], err_msg=what + ": stats")


def _native_n(ix):
    from hnsw_clj_amd import _native

    n = ctypes.c_int64(-1)
    assert _native.lib().hnswgpu_info(ix._h, ctypes.byref(n), None, None, None, None) == 0
    return n.value


def _sizes(ix):
    """(M, M0, up_blocks, entry, max_level) of hnswgpu_graph_sizes"""
    from hnsw_clj_amd import _native

    m, m0, ent, mx, blocks = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    assert _native.lib().hnswgpu_graph_sizes(ix._h, ctypes.byref(m), ctypes.byref(m0), ctypes.byref(blocks), ctypes.byref(ent),
                                             ctypes.byref(mx)) == 0
    return m.value, m0.value, blocks.value, ent.value, mx.value


def _remove(ix, gone):
    """hnsw_remove, its `kept`, n and the handle's own n against the numbering model; returns kept."""
    want = LR.kept(ix.n, gone)
    kept = ix.hnsw_remove(gone)
    assert kept.dtype == np.int64
    np.testing.assert_array_equal(kept, want)
    assert ix.n == len(want) and _native_n(ix) == len(want)
    return kept


def _built(engine, rows, metric, heuristic, mode=None, m=M):
    ix = engine.Index(rows, metric, 0)
    if mode is not None:
        ix.set_rejection_test(mode)
    ix.hnsw_build(m, EFC, SEED, heuristic=heuristic)
    return ix


def _fresh(engine, rows, metric, mode, g):
    ix = engine.Index(rows, metric, 0)
    if mode is not None:
        ix.set_rejection_test(mode)
    ix.set_graph(g)
    return ix


def _assert_same_answers(shrunk, fresh, Q, mode):
    n1 = shrunk.n
    assert fresh.n == n1 and _native_n(shrunk) == n1
    np.testing.assert_array_equal(_bits(shrunk.norms()), _bits(fresh.norms()), err_msg="norms")
    at = np.array([n1 // 3, n1 - 1, n1 // 2, 0], np.int32)
    np.testing.assert_array_equal(_bits(shrunk.batch_distances(Q[0], ids=at)), _bits(fresh.batch_distances(Q[0], ids=at)),
                                  err_msg="batch_distances")
    np.testing.assert_array_equal(_bits(shrunk.batch_distances(Q[1])), _bits(fresh.batch_distances(Q[1])), err_msg="all distances")
    if mode == 2:                                            # the int8 rows and their meta, through the traversal's own bound
        every = np.arange(n1, dtype=np.int32)
        np.testing.assert_array_equal(_bits(shrunk.hnsw_rejection_bounds(Q[2], every)), _bits(fresh.hnsw_rejection_bounds(Q[2], every)),
                                      err_msg="rejection bounds")
    for nq in (1, 32):
        for ef in (50, 200):
            _same(shrunk.hnsw_search(Q[:nq], 10, ef, want_stats=True), fresh.hnsw_search(Q[:nq], 10, ef, want_stats=True),
                  "hnsw_search nq %d ef %d" % (nq, ef))
    _same(shrunk.exact_knn(Q[:5], 10), fresh.exact_knn(Q[:5], 10), "exact_knn")


def _gone_main(g, n):
    """About 150 ids: unsorted, the last row, the entry point, some named twice and one three times."""
    rng = np.random.default_rng(31)
    gone = rng.choice(np.setdiff1d(np.arange(n - 1), [g.entry]), 148, replace=False).astype(np.int32)
    gone = np.concatenate([gone[:70], [n - 1, g.entry], gone[70:], gone[:20], gone[3:4], [g.entry]]).astype(np.int32)
    return gone


# ---- 1. the shrunken handle equals a fresh one ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2"])
@pytest.mark.parametrize("builder", ["closest", "heuristic"])
@pytest.mark.parametrize("dim", [40, 1100])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_shrunken_handle_equals_fresh_handle(native_lib, oracle, metric, dim, builder, mode):
    from hnsw_clj_amd import engine

    O = oracle
    rows, Q = _rows(O, dim)
    base = rows[:N0]
    code, heuristic = O.METRICS[metric], builder == "heuristic"
    with _built(engine, base, metric, heuristic, mode) as shrunk:
        g = shrunk.get_graph()
        gone = _gone_main(g, N0)
        key = (metric, dim, builder)
        if key not in _MODELS:                               # the model does not depend on the rejection mode: nor does the build
            _MODELS[key] = (g, R.remove(O, base, code, g, gone, heuristic))
        H.same_graph(g, _MODELS[key][0], "the build under mode %d" % mode)
        model = _MODELS[key][1]
        kept = _remove(shrunk, gone)
        assert len(kept) == N0 - 150
        H.same_graph(shrunk.get_graph(), model, "%s dim %d %s mode %d" % (metric, dim, builder, mode))
        assert _sizes(shrunk) == (M, 2 * M, int(model.up_off[-1]), model.entry, model.max_level)
        with _fresh(engine, base[kept], metric, mode, model) as fresh:
            _assert_same_answers(shrunk, fresh, Q, mode)


# ---- 2. edges ---------------------------------------------------------------------------------------------------------------
def _neighbours_of(g, u):
    out = set()
    for lc in range(int(g.levels[u]) + 1):
        out.update(R.old_list(g, u, lc))
    return sorted(out)


@pytest.mark.parametrize("builder", ["closest", "heuristic"])
@pytest.mark.parametrize("case", ["one", "no in-edges", "every neighbour", "top level", "last word"])
def test_edges(native_lib, oracle, case, builder):
    from hnsw_clj_amd import engine

    O = oracle
    rows, Q = _rows(O, 40)
    base = rows[:N0]
    heuristic = builder == "heuristic"
    with _built(engine, base, "l2", heuristic) as ix:
        g = ix.get_graph()
        l0 = g.l0_adj.reshape(N0, -1)
        chosen = None
        if case == "one":
            gone = [123]
        elif case == "no in-edges":
            lonely = np.setdiff1d(np.arange(N0), np.unique(np.concatenate([l0.ravel(), g.up_adj.ravel()])))
            lonely = lonely[lonely != g.entry]
            if len(lonely) == 0:
                gone = [int(np.argmin(np.bincount(l0[l0 >= 0], minlength=N0)))]      # the data has none: the least pointed at
            else:
                gone = [int(lonely[0])]
        elif case == "every neighbour":
            chosen = 77
            gone = [x for x in _neighbours_of(g, chosen) if x != chosen]
            assert len(gone) >= 2
        elif case == "top level":
            gone = np.flatnonzero(g.levels == g.max_level)
            assert g.entry in gone and g.max_level >= 1
        else:
            gone = np.arange(576, N0)[::-1]
        model = R.remove(O, base, O.L2, g, gone, heuristic)
        kept = _remove(ix, np.asarray(gone, np.int32))
        got = ix.get_graph()
        H.same_graph(got, model, case)
        if chosen is not None:                               # its list is what the model says: drawn from two-hop rows only
            new = int(LR.rank(N0, gone)[chosen])
            two_hop = set(int(kept[x]) for x in got.l0_adj.reshape(got.n, -1)[new] if x >= 0)
            assert two_hop and not two_hop & set(R.old_list(g, chosen, 0))
        if case == "top level":
            top = g.levels[kept].max()
            assert got.max_level == top < g.max_level and got.entry == np.flatnonzero(g.levels[kept] == top)[0]
        with _fresh(engine, base[kept], "l2", None, model) as fresh:
            _same(ix.hnsw_search(Q, 10, 50, want_stats=True), fresh.hnsw_search(Q, 10, 50, want_stats=True), case)


# ---- 3. two calls equal the model applied twice -------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["closest", "heuristic"])
def test_two_calls_equal_the_model_applied_twice(native_lib, oracle, builder):
    """(One call over the union does not have to equal them: each call repairs through its own removed rows only.)"""
    from hnsw_clj_amd import engine

    O = oracle
    rows, Q = _rows(O, 40)
    base = rows[:N0]
    heuristic = builder == "heuristic"
    rng = np.random.default_rng(12)
    with _built(engine, base, "cosine", heuristic) as ix:
        g, present = ix.get_graph(), np.arange(N0)
        for m in (90, 60):
            gone = rng.choice(ix.n, m, replace=False).astype(np.int32)
            g = R.remove(O, base[present], O.COSINE, g, gone, heuristic)
            present = present[_remove(ix, gone)]
            H.same_graph(ix.get_graph(), g, "after %d more" % m)
        with _fresh(engine, base[present], "cosine", None, g) as fresh:
            _assert_same_answers(ix, fresh, Q, None)


# ---- 4. to nothing and back -------------------------------------------------------------------------------------------------
def test_to_nothing_and_back(native_lib, oracle):
    from hnsw_clj_amd import engine

    O = oracle
    rows, Q = _rows(O, 40)
    base = rows[:N0]
    with _built(engine, base, "l2", True) as ix:
        kept = _remove(ix, np.random.default_rng(34).permutation(N0).astype(np.int32))
        assert len(kept) == 0 and ix.n == 0 and ix.has_graph
        assert _sizes(ix) == (M, 2 * M, 0, -1, 0)
        g = ix.get_graph()
        assert g.n == 0 and g.up_off.tolist() == [0] and g.up_adj.size == 0
        for nq in (1, 5):
            gi, gd, st = ix.hnsw_search(Q[:nq], 10, 50, want_stats=True)
            assert (gi == -1).all() and np.isposinf(gd).all() and not st.any()
        again = rows[N0:N0 + 300]                            # ... and grown again, by the builder the handle kept
        got = ix.hnsw_add(again, EFC, SEED)
        np.testing.assert_array_equal(got, np.arange(300, dtype=np.int32))
        og, _ = O.hnsw_build_batched(again, H.batch_schedule(300, 1), O.L2, M, EFC, SEED, O.BUILD_HEURISTIC, O.MODE_DEV)
        H.same_graph(ix.get_graph(), og, "grown again from nothing")
        with _fresh(engine, again, "l2", None, og) as fresh:
            _assert_same_answers(ix, fresh, Q, None)


# ---- 5. add and remove interleaved ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["closest", "heuristic"])
def test_add_and_remove_interleaved(native_lib, oracle, builder):
    from hnsw_clj_amd import engine

    O = oracle
    rows, Q = _rows(O, 40)
    heuristic = builder == "heuristic"
    flags = O.BUILD_HEURISTIC if heuristic else 0
    rng = np.random.default_rng(21)
    nxt = 400
    with _built(engine, rows[:nxt], "cosine", heuristic) as ix:
        g, present = ix.get_graph(), rows[:nxt]
        for step, m in (("remove", 70), ("add", 90), ("remove", 1), ("add", 1), ("remove", 130), ("add", 40)):
            if step == "remove":
                gone = rng.choice(ix.n, m, replace=False).astype(np.int32)
                g = R.remove(O, present, O.COSINE, g, gone, heuristic)
                present = present[_remove(ix, gone)]
            else:
                n_before = ix.n
                ids = ix.hnsw_add(rows[nxt:nxt + m], EFC, SEED)
                assert ids[0] == n_before and len(ids) == m
                present = np.ascontiguousarray(np.concatenate([present, rows[nxt:nxt + m]]))
                nxt += m
                g, _ = O.hnsw_build_batched(present, H.batch_schedule(len(present), n_before), O.COSINE, M, EFC, SEED, flags, O.MODE_DEV,
                                            start=g)
            H.same_graph(ix.get_graph(), g, "after %s %d" % (step, m))
        with _fresh(engine, present, "cosine", None, g) as fresh:
            _assert_same_answers(ix, fresh, Q, None)


# ---- 6. save, load and the builder --------------------------------------------------------------------------------------------
def test_save_load_keep_the_graph_and_the_builder(native_lib, oracle, tmp_path):
    from hnsw_clj_amd import engine

    O = oracle
    rows, Q = _rows(O, 40)
    base = rows[:N0]
    with _built(engine, base, "l2", True) as ix:
        g = ix.get_graph()
        gone = _gone_main(g, N0)
        model = R.remove(O, base, O.L2, g, gone, True)
        kept = _remove(ix, gone)
        path = tmp_path / "shrunk.idx"
        ix.save(path)
        with engine.Index.load(path, 0) as back:
            assert back.n == len(kept)
            H.same_graph(back.get_graph(), model, "loaded")
            _same(back.hnsw_search(Q, 10, 50, want_stats=True), ix.hnsw_search(Q, 10, 50, want_stats=True), "loaded")
            more = rows[N0:N0 + 50]
            present = np.ascontiguousarray(np.concatenate([base[kept], more]))
            og, _ = O.hnsw_build_batched(present, H.batch_schedule(len(present), len(kept)), O.L2, M, EFC, SEED, O.BUILD_HEURISTIC,
                                         O.MODE_DEV, start=model)
            for handle in (back, ix):                        # the heuristic builder came back with the file, and stayed on the handle
                handle.hnsw_add(more, EFC, SEED)
                H.same_graph(handle.get_graph(), og, "grown behind the removal")


# ---- 7. refusals leave the handle alone ---------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone(native_lib, oracle):
    from hnsw_clj_amd import engine

    L = native_lib.lib()
    rows, Q = _rows(oracle, 40)
    base = rows[:500]

    def ids(*v):
        a = np.array(v, np.int32)
        return a, a.ctypes.data_as(ctypes.c_void_p)

    one, ptr = ids(3)

    def state(ix):
        return ix.get_graph(), ix.hnsw_search(Q[:5], 10, 50, want_stats=True)

    def unchanged(ix, before, what):
        assert ix.n == 500 and _native_n(ix) == 500
        g, answer = state(ix)
        H.same_graph(g, before[0], what)
        _same(answer, before[1], what)

    def refused(ix, p, m, code, word=None, before=None):
        out = ctypes.c_int64(-7)
        assert L.hnswgpu_hnsw_remove(ix._h, p, m, ctypes.byref(out)) == code
        assert out.value == (500 if code == 0 else -7)        # a refusal does not write n_after
        if word:
            assert word in L.hnswgpu_last_error().lower()
        if before is not None:                                # every refusal leaves n, the graph and a search's bits alone
            unchanged(ix, before, "after a refusal with code %d (%s)" % (code, word))

    with engine.Index(base, "cosine", 0) as bare:
        refused(bare, ptr, 1, -3, b"no graph")
        refused(bare, None, 0, 0)                             # nothing to remove: nothing is looked at
        refused(bare, ptr, 0, 0)
        assert bare.n == 500 and not bare.has_graph
    with _built(engine, base, "cosine", True) as ix:
        before = state(ix)
        refused(ix, None, 1, -1, b"rows is null", before)
        refused(ix, ptr, -1, -1, None, before)
        for bad in (-1, 500):
            arr, p = ids(3, 4, bad, 5)
            refused(ix, p, 4, -1, b"rows[2]", before)         # the message names the position
        refused(ix, ptr, 0, 0, None, before)                  # nothing to remove: nothing happens
        refused(ix, None, 0, 0, None, before)
        assert L.hnswgpu_hnsw_remove(ix._h, None, 0, None) == 0   # n_after may be null
        ix.ivf_build(8, 2, 42)
        refused(ix, ptr, 1, -3, b"ivf lists", before)
        out = ctypes.c_int64(-7)                              # the other two removals still refuse a handle with a graph
        assert L.hnswgpu_ivf_remove(ix._h, ptr, 1, ctypes.byref(out)) == -3 and out.value == -7
        assert b"graph" in L.hnswgpu_last_error().lower()
    with _built(engine, base, "cosine", False) as ix:
        before = state(ix)
        ix.lsh_build(8, 6, 64, 42)
        refused(ix, ptr, 1, -3, b"lsh tables", before)
        out = ctypes.c_int64(-7)
        assert L.hnswgpu_lsh_remove(ix._h, ptr, 1, ctypes.byref(out)) == -3 and out.value == -7
    with engine.Index(base, "cosine", 0) as forest:
        forest.hnsw_build_parts([0, 250, 500], 8, 40, 42)
        g0 = forest.get_graph()
        refused(forest, ptr, 1, -3, b"forest")
        assert forest.n == 500 and _native_n(forest) == 500
        g1 = forest.get_graph()
        np.testing.assert_array_equal(g0.l0_adj, g1.l0_adj)
        np.testing.assert_array_equal(g0.up_adj, g1.up_adj)
    with _built(engine, base, "cosine", False) as ix:         # ... and n_after null on a call that removes
        assert L.hnswgpu_hnsw_remove(ix._h, ptr, 1, None) == 0
        assert _native_n(ix) == 499


# ---- 8. searches beside removals ----------------------------------------------------------------------------------------------
def test_searches_beside_removals_see_one_of_the_index_states(native_lib, oracle):
    from hnsw_clj_amd import engine

    O = oracle
    rows, Q = _rows(O, 40)
    n0, step = N0, 100
    rng = np.random.default_rng(8)
    qs = [np.ascontiguousarray(Q[3 * t:3 * t + 3]) for t in range(4)]
    removals, present = [], [np.arange(n0)]                 # each removal in the numbering current at its turn
    for _ in range(3):
        removals.append(rng.choice(len(present[-1]), step, replace=False).astype(np.int32))
        present.append(present[-1][LR.kept(len(present[-1]), removals[-1])])
    with _built(engine, rows[:n0], "l2", False) as ix:
        g = ix.get_graph()
        states = []                                         # per index state, per thread: (ids, distance bits), from fresh handles
        for s, now in enumerate(present):
            if s > 0:
                g = R.remove(O, rows[present[s - 1]], O.L2, g, removals[s - 1], False)
            with _fresh(engine, rows[now], "l2", None, g) as fresh:
                states.append([(i, _bits(d)) for i, d in (fresh.hnsw_search(q, 10, 50) for q in qs)])
        stop, errors, seen = threading.Event(), [], [set() for _ in range(4)]

        def matches(t, i, d):
            return [s for s in range(4) if np.array_equal(i, states[s][t][0]) and np.array_equal(_bits(d), states[s][t][1])]

        def searcher(t):
            try:
                for _ in range(20000):                      # bounded: the remover sets `stop` long before
                    if stop.is_set():
                        break
                    hit = matches(t, *ix.hnsw_search(qs[t], 10, 50))
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
                    ix.hnsw_remove(gone)
                    for t in range(4):                      # the shrunken index is what every later search sees
                        assert s + 1 in matches(t, *ix.hnsw_search(qs[t], 10, 50))
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
        assert all(3 in matches(t, *ix.hnsw_search(qs[t], 10, 50)) for t in range(4))


# ---- 9. the Python mirror -----------------------------------------------------------------------------------------------------
def test_python_mirror_remove_vectors(native_lib, oracle):
    from hnsw_clj_amd import ultra_fast

    rows, _ = _rows(oracle, 40)
    n0 = 600
    graph = ultra_fast.build_index([("v-%d" % i, rows[i]) for i in range(n0)], M=8, ef_construction=48, show_progress=False, heuristic=True)
    try:
        assert ultra_fast.search_knn(graph, rows[33], 5, ef=200)[0]["id"] == "v-33"
        assert ultra_fast.remove_vectors(graph, ["v-33", "v-0", "v-599"]) is graph
        assert ultra_fast.graph_info(graph)["num-elements"] == n0 - 3 and len(graph.ids) == n0 - 3
        assert all(r["id"] not in ("v-33", "v-0", "v-599") for r in ultra_fast.search_knn(graph, rows[33], 10, ef=200))
        res = ultra_fast.search_knn(graph, rows[34], 5, ef=200)
        assert res[0]["id"] == "v-34" and abs(res[0]["distance"]) <= 1e-5
        with pytest.raises(KeyError):
            ultra_fast.remove_vectors(graph, ["v-1", "v-33"])
        assert len(graph.ids) == n0 - 3 and graph.index.n == n0 - 3
    finally:
        graph.close()
