"""hnswgpu_hnsw_update on the device: the graph an update leaves equals the numpy model (hnsw_update_model.py) EDGE FOR EDGE, and the
updated handle is indistinguishable, bit for bit, from a fresh handle over the new base that was given the model's graph through
set_graph -- norms, distances, rejection bounds, every search's ids, distance BITS and stats.  No tolerance anywhere.  The data
sets and the conditions they meet: hnsw_update_model.py, asserted by test_hnsw_update_host.py."""
import ctypes
import threading

import numpy as np
import pytest

import hnsw_build_model as H
import hnsw_remove_model as R
import hnsw_update_model as U
import test_hnsw_remove_gpu as THR

pytestmark = pytest.mark.gpu

N0, M, EFC, SEED = U.N0, U.M, U.EFC, U.SEED
_MODELS = {}


def _flags(O, heuristic):
    return O.BUILD_HEURISTIC if heuristic else 0


def _update(ix, ids, vals):
    """hnsw_update; n and the handle's own n stay."""
    n = ix.n
    assert ix.hnsw_update(ids, vals, EFC) is None
    assert ix.n == n and THR._native_n(ix) == n


def _check(engine, O, ix, cur, metric, mode, model, Q, what):
    """The handle against the model's graph and against a fresh handle over `cur` that was given it."""
    H.same_graph(ix.get_graph(), model, what)
    assert THR._sizes(ix) == (model.M, model.M0, int(model.up_off[-1]), model.entry, model.max_level)
    with THR._fresh(engine, cur, metric, mode, model) as fresh:
        THR._assert_same_answers(ix, fresh, Q, mode)


# ---- 1. the updated handle equals the model and a fresh handle -------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2"])
@pytest.mark.parametrize("builder", ["closest", "heuristic"])
@pytest.mark.parametrize("dim", U.DIMS)
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_updated_handle_equals_model_and_fresh_handle(native_lib, oracle, metric, dim, builder, mode):
    from hnsw_clj_amd import engine

    O = oracle
    base, pool, Q = U.rows(O, dim)
    code, heuristic = O.METRICS[metric], builder == "heuristic"
    with THR._built(engine, base, metric, heuristic, mode) as ix:
        g = ix.get_graph()
        ids = U.main_ids(g)
        vals, cur = U.new_values(base, pool, ids)
        key = (metric, dim, builder)
        if key not in _MODELS:                               # the model does not depend on the rejection mode: nor does the build
            _MODELS[key] = (g, U.update(O, cur, code, g, ids, EFC, _flags(O, heuristic))[0])
        H.same_graph(g, _MODELS[key][0], "the build under mode %d" % mode)
        model = _MODELS[key][1]
        assert len(ids) == 150 and N0 - 1 in ids and g.entry in ids
        _update(ix, ids, vals)
        np.testing.assert_array_equal(model.levels, g.levels)
        _check(engine, O, ix, cur, metric, mode, model, Q, "%s dim %d %s mode %d" % (metric, dim, builder, mode))


# ---- 2. the tail identity, through the library itself ----------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["closest", "heuristic"])
def test_tail_update_is_remove_then_add(native_lib, oracle, builder):
    from hnsw_clj_amd import engine

    O = oracle
    base, pool, Q = U.rows(O, 40)
    heuristic = builder == "heuristic"
    tail = np.arange(N0 - 65, N0, dtype=np.int32)
    vals, cur = U.new_values(base, pool, tail)
    with THR._built(engine, base, "cosine", heuristic, 2) as ix, THR._built(engine, base, "cosine", heuristic, 2) as twin:
        _update(ix, tail[::-1].copy(), vals[::-1].copy())
        THR._remove(twin, tail)
        np.testing.assert_array_equal(twin.hnsw_add(vals, EFC, SEED), tail)
        H.same_graph(ix.get_graph(), twin.get_graph(), "update of the last 65 rows against remove + add")
        assert THR._sizes(ix) == THR._sizes(twin)
        THR._assert_same_answers(ix, twin, Q, 2)


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------
def _neighbours_of(g, u):
    out = set()
    for lc in range(int(g.levels[u]) + 1):
        out.update(R.old_list(g, u, lc))
    return sorted(out - {u})


@pytest.mark.parametrize("builder", ["closest", "heuristic"])
@pytest.mark.parametrize("case", ["one", "no in-edges", "every neighbour", "top level", "last word", "mutual", "every row", "one-row handle"])
def test_edges(native_lib, oracle, case, builder):
    from hnsw_clj_amd import engine

    O = oracle
    rows, pool, Q = U.rows(O, 40)
    base = rows[:1] if case == "one-row handle" else rows
    n = len(base)
    heuristic = builder == "heuristic"
    with THR._built(engine, base, "l2", heuristic) as ix:
        g = ix.get_graph()
        l0 = g.l0_adj.reshape(n, -1)
        if case == "one":
            ids = [123]
        elif case == "no in-edges":
            lonely = np.setdiff1d(np.arange(n), np.unique(np.concatenate([l0.ravel(), g.up_adj.ravel()])))
            lonely = lonely[lonely != g.entry]
            ids = [int(lonely[0])] if len(lonely) else [int(np.argmin(np.bincount(l0[l0 >= 0], minlength=n)))]   # none: the least pointed at
        elif case == "every neighbour":
            ids = _neighbours_of(g, 77)
            assert len(ids) >= 2
        elif case == "top level":
            ids = [g.entry]                                      # U is the entry point alone
            assert g.max_level >= 1
        elif case == "last word":
            ids = np.arange(576, n)[::-1]
        elif case == "mutual":
            a = 200
            b = next(int(x) for x in l0[a] if x >= 0 and a in l0[x])
            ids = [b, a]
        elif case == "every row":
            ids = np.random.default_rng(4).permutation(n)
        else:
            ids = [0]
        ids = np.asarray(ids, np.int32)
        if case == "every row":
            vals = np.ascontiguousarray(base[::-1][ids])         # the rows in reverse: as many equal rows as before
        else:
            vals = np.ascontiguousarray(pool[10:10 + len(ids)])
        cur = base.copy()
        cur[ids] = vals
        model, _ = U.update(O, cur, O.L2, g, ids, EFC, _flags(O, heuristic))
        _update(ix, ids, vals)
        got = ix.get_graph()
        H.same_graph(got, model, case)
        if case == "top level" and (g.levels == g.max_level).sum() == 1:   # alone on its level: it empties and is taken back
            assert (got.entry, got.max_level) == (g.entry, g.max_level)
        if case == "every row":
            assert got.entry == 0 or g.levels[got.entry] > g.levels[0]
        with THR._fresh(engine, cur, "l2", None, model) as fresh:
            THR._same(ix.hnsw_search(Q, 10, 50, want_stats=True), fresh.hnsw_search(Q, 10, 50, want_stats=True), case)
            THR._same(ix.exact_knn(Q[:5], min(10, n)), fresh.exact_knn(Q[:5], min(10, n)), case)


# ---- 4. two calls equal the model applied twice ------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["closest", "heuristic"])
def test_two_calls_equal_the_model_applied_twice(native_lib, oracle, builder):
    """... and differ from the model applied to the union: each call unlinks through its own rows only."""
    from hnsw_clj_amd import engine

    O = oracle
    base, pool, Q = U.rows(O, 40)
    heuristic = builder == "heuristic"
    flags = _flags(O, heuristic)
    picked = np.random.default_rng(12).choice(N0, 150, replace=False).astype(np.int32)
    with THR._built(engine, base, "cosine", heuristic) as ix:
        g0 = ix.get_graph()
        g, cur, at = g0, base.copy(), 0
        for part in (picked[:90], picked[90:]):
            vals = np.ascontiguousarray(pool[at:at + len(part)])
            at += len(part)
            cur = cur.copy()
            cur[part] = vals
            g, _ = U.update(O, cur, O.COSINE, g, part, EFC, flags)
            _update(ix, part, vals)
            H.same_graph(ix.get_graph(), g, "after %d more" % len(part))
        union, _ = U.update(O, cur, O.COSINE, g0, picked, EFC, flags)
        assert (union.l0_adj != g.l0_adj).any(), "the split made no difference"
        _check(engine, O, ix, cur, "cosine", None, g, Q, "two calls")


# ---- 5. interleaved with add and remove --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["closest", "heuristic"])
def test_interleaved_with_add_and_remove(native_lib, oracle, builder):
    from hnsw_clj_amd import engine

    O = oracle
    rows, pool, Q = U.rows(O, 40)
    heuristic = builder == "heuristic"
    flags = _flags(O, heuristic)
    rng = np.random.default_rng(21)
    nxt, at, removed = 400, 0, False
    with THR._built(engine, rows[:nxt], "cosine", heuristic) as ix:
        g, cur = ix.get_graph(), rows[:nxt].copy()
        for step, m in (("update", 50), ("add", 90), ("update", 1), ("remove", 30), ("update", 40), ("add", 1), ("update", 7)):
            if step == "update":
                ids = rng.choice(ix.n, m, replace=False).astype(np.int32)
                vals = np.ascontiguousarray(pool[at:at + m])
                at += m
                cur = cur.copy()
                cur[ids] = vals
                g, _ = U.update(O, cur, O.COSINE, g, ids, EFC, flags)
                _update(ix, ids, vals)
            elif step == "remove":
                gone = rng.choice(ix.n, m, replace=False).astype(np.int32)
                g = R.remove(O, cur, O.COSINE, g, gone, heuristic)
                cur = np.ascontiguousarray(cur[THR._remove(ix, gone)])
                removed = True
            else:
                n_before = ix.n
                ix.hnsw_add(rows[nxt:nxt + m], EFC, SEED)
                cur = np.ascontiguousarray(np.concatenate([cur, rows[nxt:nxt + m]]))
                nxt += m
                g, _ = O.hnsw_build_batched(cur, H.batch_schedule(len(cur), n_before), O.COSINE, M, EFC, SEED, flags, O.MODE_DEV, start=g)
            got = ix.get_graph()
            H.same_graph(got, g, "after %s %d" % (step, m))
            if not removed:                                  # the levels are the seed's draws by id still: a fresh build draws the same
                with THR._built(engine, cur, "cosine", heuristic) as again:
                    np.testing.assert_array_equal(got.levels, again.get_graph().levels, err_msg="levels after %s %d" % (step, m))
        _check(engine, O, ix, cur, "cosine", None, g, Q, "interleaved")


# ---- 6. save, load and the builder -------------------------------------------------------------------------------------------------
def test_save_load_keep_the_graph_and_the_builder(native_lib, oracle, tmp_path):
    from hnsw_clj_amd import engine

    O = oracle
    base, pool, Q = U.rows(O, 40)
    with THR._built(engine, base, "l2", True) as ix:
        g = ix.get_graph()
        ids = U.main_ids(g)
        vals, cur = U.new_values(base, pool, ids)
        model, _ = U.update(O, cur, O.L2, g, ids, EFC, O.BUILD_HEURISTIC)
        _update(ix, ids, vals)
        path = tmp_path / "updated.idx"
        ix.save(path)
        with engine.Index.load(path, 0) as back:
            H.same_graph(back.get_graph(), model, "loaded")
            THR._same(back.hnsw_search(Q, 10, 50, want_stats=True), ix.hnsw_search(Q, 10, 50, want_stats=True), "loaded")
            more = np.arange(40, 90, dtype=np.int32)
            vals2 = np.ascontiguousarray(pool[200:250])
            cur2 = cur.copy()
            cur2[more] = vals2
            model2, _ = U.update(O, cur2, O.L2, model, more, EFC, O.BUILD_HEURISTIC)
            for handle in (back, ix):                        # the heuristic builder came back with the file, and stayed on the handle
                _update(handle, more, vals2)
                H.same_graph(handle.get_graph(), model2, "updated behind the file")


# ---- 7. a graph installed by set_graph updates by closest-m ------------------------------------------------------------------------
def test_installed_graph_updates_by_closest_m(native_lib, oracle):
    from hnsw_clj_amd import engine

    O = oracle
    base, pool, Q = U.rows(O, 40)
    with THR._built(engine, base, "cosine", True) as built:
        g = built.get_graph()
    ids = U.main_ids(g)
    vals, cur = U.new_values(base, pool, ids)
    closest, _ = U.update(O, cur, O.COSINE, g, ids, EFC, 0)
    heur, _ = U.update(O, cur, O.COSINE, g, ids, EFC, O.BUILD_HEURISTIC)
    assert (closest.l0_adj != heur.l0_adj).any()
    with THR._fresh(engine, base, "cosine", None, g) as ix:
        _update(ix, ids, vals)
        _check(engine, O, ix, cur, "cosine", None, closest, Q, "a heuristic graph installed by set_graph")


# ---- 8. refusals, in their order, leave the handle alone ---------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone(native_lib, oracle):
    from hnsw_clj_amd import engine

    O = oracle
    L = native_lib.lib()
    rows, pool, Q = U.rows(O, 40)
    base = rows[:500]
    new = np.ascontiguousarray(pool[:8])
    vp = new.ctypes.data_as(ctypes.c_void_p)

    def ids(*v):
        a = np.array(v, np.int32)
        return a, a.ctypes.data_as(ctypes.c_void_p)

    one, ptr = ids(3)

    def state(ix):
        return ix.get_graph(), THR._bits(ix.norms()), ix.hnsw_search(Q[:5], 10, 50, want_stats=True)

    def refused(ix, p, v, m, efc, code, words=(), before=None):
        assert L.hnswgpu_hnsw_update(ix._h, p, v, m, efc) == code
        for word in words:
            assert word in L.hnswgpu_last_error().lower(), L.hnswgpu_last_error()
        assert ix.n == 500 and THR._native_n(ix) == 500
        if before is not None:                                # every refusal leaves the graph, the norms and a search's bits alone
            g, norms, answer = state(ix)
            what = "after a refusal with code %d %s" % (code, words)
            H.same_graph(g, before[0], what)
            np.testing.assert_array_equal(norms, before[1], err_msg=what)
            THR._same(answer, before[2], what)

    with engine.Index(base, "cosine", 0) as bare:
        refused(bare, ptr, vp, -1, EFC, -1)                   # m < 0, null arrays and ef_construction come before the handle's state
        refused(bare, None, vp, 1, EFC, -1, [b"ids is null"])
        refused(bare, ptr, None, 1, EFC, -1, [b"rows is null"])
        for efc in (0, 4097):
            refused(bare, ptr, vp, 1, efc, -5, [b"ef_construction"])
            refused(bare, None, None, 0, efc, -5, [b"ef_construction"])   # ... and before m == 0
        refused(bare, None, None, 0, EFC, 0)                  # nothing to update: nothing is looked at
        refused(bare, ptr, vp, 0, EFC, 0)
        refused(bare, ptr, vp, 1, EFC, -3, [b"no graph"])
        bad, bp = ids(777)
        refused(bare, bp, vp, 1, EFC, -3, [b"no graph"])      # the handle's state comes before the ids
        assert not bare.has_graph
    with THR._built(engine, base, "cosine", True) as ix:
        before = state(ix)
        refused(ix, None, vp, 1, EFC, -1, [b"ids is null"], before)
        refused(ix, ptr, None, 1, EFC, -1, [b"rows is null"], before)
        refused(ix, ptr, vp, -1, EFC, -1, (), before)
        refused(ix, ptr, vp, 1, 0, -5, [b"ef_construction"], before)
        refused(ix, ptr, vp, 0, EFC, 0, (), before)
        for out in (-1, 500):
            arr, p = ids(3, 4, out, 5)
            refused(ix, p, vp, 4, EFC, -1, [b"ids[2]", b"not a row"], before)
        arr, p = ids(3, 9, 4, 9, 5)
        refused(ix, p, vp, 5, EFC, -1, [b"ids[3]", b"ids[1]", b"twice"], before)     # both positions are named
        arr, p = ids(3, 9, 500, 9)
        refused(ix, p, vp, 4, EFC, -1, [b"ids[2]", b"not a row"], before)           # outside [0, n) comes before twice
        long_ids = np.arange(400, dtype=np.int32)[::-1].copy()    # a duplicate late in a long id array: nothing was enqueued
        long_ids[-1] = long_ids[5]
        long_rows = np.ascontiguousarray(np.concatenate([pool, pool])[:400])
        refused(ix, long_ids.ctypes.data_as(ctypes.c_void_p), long_rows.ctypes.data_as(ctypes.c_void_p), 400, EFC, -1,
                [b"ids[399]", b"ids[5]"], before)
        with pytest.raises(ValueError):
            ix.hnsw_update([1, 2], new[:1])
        ix.ivf_build(8, 2, 42)
        refused(ix, ptr, vp, 1, EFC, -3, [b"ivf lists"], before)
    with THR._built(engine, base, "cosine", False) as ix:
        before = state(ix)
        ix.lsh_build(8, 6, 64, 42)
        refused(ix, ptr, vp, 1, EFC, -3, [b"lsh tables"], before)
    with engine.Index(base, "cosine", 0) as forest:
        forest.hnsw_build_parts([0, 250, 500], 8, 40, 42)
        g0 = forest.get_graph()
        refused(forest, ptr, vp, 1, EFC, -3, [b"forest"])
        g1 = forest.get_graph()
        np.testing.assert_array_equal(g0.l0_adj, g1.l0_adj)
        np.testing.assert_array_equal(g0.up_adj, g1.up_adj)
    with THR._built(engine, base, "cosine", False) as built:
        g = built.get_graph()
    narrow = O.Graph(g.levels, np.ascontiguousarray(g.l0_adj.reshape(500, -1)[:, :12]), g.up_off, g.up_adj, g.M, g.entry, g.max_level)
    with THR._fresh(engine, base, "cosine", None, narrow) as ix:   # M0 = 12 over M = 8
        before = state(ix)
        refused(ix, ptr, vp, 1, EFC, -3, [b"m0 = 2 m"], before)


# ---- 9. searches beside updates ------------------------------------------------------------------------------------------------------
def test_searches_beside_updates_see_one_of_the_index_states(native_lib, oracle):
    from hnsw_clj_amd import engine

    O = oracle
    base, pool, Q = U.rows(O, 40)
    rng = np.random.default_rng(8)
    qs = [np.ascontiguousarray(Q[3 * t:3 * t + 3]) for t in range(4)]
    calls = [(rng.choice(N0, 100, replace=False).astype(np.int32), np.ascontiguousarray(pool[100 * s:100 * s + 100])) for s in range(3)]
    with THR._built(engine, base, "l2", False) as ix:
        g, cur = ix.get_graph(), base.copy()
        states = []                                         # per index state, per thread: (ids, distance bits), from fresh handles
        for s in range(4):
            if s > 0:
                cur = cur.copy()
                cur[calls[s - 1][0]] = calls[s - 1][1]
                g, _ = U.update(O, cur, O.L2, g, calls[s - 1][0], EFC, 0)
            with THR._fresh(engine, cur, "l2", None, g) as fresh:
                states.append([(i, THR._bits(d)) for i, d in (fresh.hnsw_search(q, 10, 50) for q in qs)])
        assert all(any(not np.array_equal(states[s][t][1], states[s + 1][t][1]) for t in range(4)) for s in range(3))
        stop, errors, seen = threading.Event(), [], [set() for _ in range(4)]

        def matches(t, i, d):
            return [s for s in range(4) if np.array_equal(i, states[s][t][0]) and np.array_equal(THR._bits(d), states[s][t][1])]

        def searcher(t):
            try:
                for _ in range(20000):                      # bounded: the updater sets `stop` long before
                    if stop.is_set():
                        break
                    hit = matches(t, *ix.hnsw_search(qs[t], 10, 50))
                    if not hit:
                        raise AssertionError("thread %d: an answer that belongs to none of the four index states" % t)
                    seen[t].update(hit)
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
                stop.set()

        def updater():
            try:
                for s, (ids, vals) in enumerate(calls):
                    if stop.is_set():
                        return
                    ix.hnsw_update(ids, vals, EFC)
                    for t in range(4):                      # the updated index is what every later search sees
                        assert s + 1 in matches(t, *ix.hnsw_search(qs[t], 10, 50))
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
            finally:
                stop.set()

        threads = [threading.Thread(target=searcher, args=(t,), daemon=True) for t in range(4)]
        threads.append(threading.Thread(target=updater, daemon=True))
        for th in threads:
            th.start()
        for th in threads:
            th.join(THR.STEP_SECONDS)
            assert not th.is_alive(), "a thread did not finish within its time limit"
        assert not errors, errors[0]
        H.same_graph(ix.get_graph(), g, "after the three updates")
        assert all(3 in matches(t, *ix.hnsw_search(qs[t], 10, 50)) for t in range(4))


# ---- 10. the Python mirror -----------------------------------------------------------------------------------------------------------
def test_python_mirror_update_vectors(native_lib, oracle):
    from hnsw_clj_amd import ultra_fast

    base, pool, _ = U.rows(oracle, 40)
    n0 = 600
    graph = ultra_fast.build_index([("v-%d" % i, base[i]) for i in range(n0)], M=8, ef_construction=48, show_progress=False, heuristic=True)
    try:
        assert ultra_fast.search_knn(graph, base[33], 5, ef=200)[0]["id"] == "v-33"
        assert ultra_fast.update_vectors(graph, [("v-33", pool[0]), ("v-599", pool[1]), ("v-0", pool[2])]) is graph
        assert ultra_fast.graph_info(graph)["num-elements"] == n0 and len(graph.ids) == n0
        for name, v in (("v-33", pool[0]), ("v-599", pool[1]), ("v-0", pool[2]), ("v-34", base[34])):
            res = ultra_fast.search_knn(graph, v, 5, ef=200)
            assert res[0]["id"] == name and abs(res[0]["distance"]) <= 1e-5
        got = graph.index.batch_distances(pool[1], ids=np.array([599], np.int32))
        assert abs(float(got[0])) <= 1e-5                    # the row itself took the new values
        with pytest.raises(KeyError):
            ultra_fast.update_vectors(graph, [("v-1", pool[3]), ("v-600", pool[4])])
        with pytest.raises(ValueError):
            ultra_fast.update_vectors(graph, [("v-1", pool[3]), ("v-1", pool[4])])
        assert ultra_fast.search_knn(graph, base[1], 5, ef=200)[0]["id"] == "v-1"     # neither call updated anything
    finally:
        graph.close()
