"""hnswgpu_lsh_update on the device: a handle whose rows took new values is indistinguishable, bit for bit, from a fresh handle over
the base with the new values that was given the same hyperplanes through set_lsh -- lsh_get array for array, every search's ids
and distance BITS, norms, the saved file's bytes.  The fresh handle's buckets come from the host counting sort of a build.  As
yardsticks that run none of the code under test: the numpy counting sort (lsh_model.buckets, inside _assert_same_tables) and the
numpy update applied one row at a time (lsh_update_model.merge)."""
import ctypes
import threading

import numpy as np
import pytest

import lsh_update_model as U
import test_lsh_remove_gpu as TLR
from test_lsh_remove_gpu import CONFIGS, K, N, NQ, STEP_SECONDS, _bits, _data, _fresh, _native_n, _same, _tables_equal

pytestmark = pytest.mark.gpu

TABLES, BITS = 8, 6


def _new_values(rng, base, ids):
    """New values for rows `ids`: every other one its old value with a little noise (most of its codes stay, some flip: a row that
    moves in some tables and stays in others), the rest unrelated (it moves nearly everywhere)."""
    ids = np.asarray(ids)
    rows = rng.standard_normal((len(ids), base.shape[1])).astype(np.float32)
    rows[::2] = base[ids[::2]] + 0.2 * rows[::2]
    return rows


def _update(ix, cur, ids, rows):
    """lsh_update and the bookkeeping: returns the base the handle holds now"""
    n = ix.n
    ix.lsh_update(ids, rows)
    assert ix.n == n == _native_n(ix)
    return U.apply(cur, ids, rows)


def _assert_equals_fresh(engine, ix, cur, metric, planes, mode, Q=None, tmp_path=None, what=""):
    """The tables array for array (and against the numpy counting sort), the norms; with Q every search, and with tmp_path the file"""
    with _fresh(engine, cur, metric, planes, mode) as fresh:
        tables = TLR._assert_same_tables(ix, fresh, what)
        np.testing.assert_array_equal(_bits(ix.norms()), _bits(fresh.norms()), err_msg=what + ": norms")
        if Q is not None:
            n = ix.n
            np.testing.assert_array_equal(ix.lsh_hash(cur), tables[1], err_msg=what + ": a row's code depends on how the handle came")
            for cfg in CONFIGS:
                for nq in (1, len(Q)):
                    _same(ix.lsh_search(Q[:nq], K, *cfg), fresh.lsh_search(Q[:nq], K, *cfg), "%s lsh_search %s nq %d" % (what, cfg, nq))
            keep = np.arange(n) % 3 != 1
            cfg = CONFIGS[2]
            one = engine.pack_mask(keep, n)
            _same(ix.lsh_search_filtered(Q, K, one, *cfg), fresh.lsh_search_filtered(Q, K, one, *cfg), what + " lsh_search_filtered")
            each = engine.pack_masks([np.arange(n) % 5 != q % 5 for q in range(len(Q))], n)
            _same(ix.lsh_search_filtered_each(Q, K, each, *cfg), fresh.lsh_search_filtered_each(Q, K, each, *cfg),
                  what + " lsh_search_filtered_each")
            _same(ix.exact_knn(Q[:5], K), fresh.exact_knn(Q[:5], K), what + " exact_knn")
            pick = np.unique(np.minimum([0, n - 1, n // 2, 31, 32], n - 1)).astype(np.int32)
            np.testing.assert_array_equal(_bits(ix.batch_distances(Q[0], ids=pick)), _bits(fresh.batch_distances(Q[0], ids=pick)),
                                          err_msg=what + ": batch_distances")
        if tmp_path is not None:
            fa, fb = tmp_path / "updated.idx", tmp_path / "fresh.idx"
            ix.save(fa)
            fresh.save(fb)
            assert fa.read_bytes() == fb.read_bytes(), what + ": the saved files differ"
    return tables


def _touch(ix, Q):
    """the base-order int8 rows of a handle without a graph come with the first bounds call: the update then remakes them"""
    from hnsw_clj_amd._native import HnswGpuError

    try:
        ix.distance_bounds(Q[0], np.arange(ix.n, dtype=np.int32))
    except HnswGpuError:
        pass                                                # (a handle that makes no int8 rows)


def _mode_of(dim):
    return 2 if dim == 257 else None                        # None: the mode new handles get


def _built(engine, rows, metric, dim, Q):
    ix = engine.Index(rows, metric, 0)
    if _mode_of(dim) is not None:
        ix.set_rejection_test(_mode_of(dim))
    ix.lsh_build(TABLES, BITS, 64, 42)
    _touch(ix, Q)
    return ix


CASES = [(metric, dim) for dim in (64, 257) for metric in ("cosine", "l2", "dot")]
CASE_IDS = ["%s-dim%d" % c for c in CASES]


# ---- 1. scripted planes -----------------------------------------------------------------------------------------------------
SCRIPT_N = 24
SCRIPT_PLANES = np.eye(8, dtype=np.float32)[:4].reshape(2, 2, 8)   # table 0: bits = signs of x0, x1; table 1: signs of x2, x3


def _scripted_row(r, c0, c1):
    """A row of dim 8 whose signs choose bucket c0 of table 0 and c1 of table 1; the magnitudes differ from row to row"""
    v = np.full(8, 1.0 + r / 64.0, np.float32)
    for j, bit in enumerate(((c0 & 1), (c0 >> 1), (c1 & 1), (c1 >> 1))):
        v[j] = v[j] if bit else -v[j]
    return v


def test_scripted_moves(native_lib, tmp_path):
    from hnsw_clj_amd import engine

    codes = np.full((SCRIPT_N, 2), 3, np.uint16)
    codes[[3, 10, 17], 0] = 1
    codes[5, 0] = 2
    codes[2, 1] = 2
    base = np.stack([_scripted_row(r, *codes[r]) for r in range(SCRIPT_N)])
    Q = base[:5] + np.float32(0.01)

    def bucket(tables, t, b):
        return tables[3][t, tables[2][t, b]:tables[2][t, b + 1]].tolist()

    steps = [
        # (what, {row: (code in table 0, code in table 1)}, [(table, bucket, its members afterwards)])
        ("a row that moves in table 0 only", {7: (1, 3)}, [(0, 1, [3, 7, 10, 17]), (1, 2, [2])]),
        ("a row that moves in both tables", {12: (1, 2)}, [(0, 1, [3, 7, 10, 12, 17]), (1, 2, [2, 12])]),
        ("a bucket emptied and an empty bucket filled", {5: (0, 3)}, [(0, 2, []), (0, 0, [5])]),
        ("two rows that swap buckets", {3: (3, 3), 4: (1, 3)}, [(0, 1, [4, 7, 10, 12, 17])]),
        ("joiners before, between and behind the kept members, beside a leaver", {20: (1, 3), 1: (1, 3), 10: (3, 3), 8: (1, 3)},
         [(0, 1, [1, 4, 7, 8, 12, 17, 20])]),
        ("row 0 and row n - 1", {0: (2, 0), SCRIPT_N - 1: (2, 0)}, [(0, 2, [0, SCRIPT_N - 1]), (1, 0, [0, SCRIPT_N - 1])]),
    ]
    with engine.Index(base, "l2", 0) as ix:
        ix.set_lsh(SCRIPT_PLANES)
        model = ix.lsh_get()[1:]
        np.testing.assert_array_equal(model[0], codes)
        cur = base
        for what, moves, expect in steps:
            ids = np.array(list(moves), np.int32)
            rows = np.stack([_scripted_row(r, *moves[r]) for r in ids])
            before = ix.lsh_get()
            cur = _update(ix, cur, ids, rows)
            model = U.merge(*model, ids, np.array([moves[r] for r in ids], np.uint16))
            tables = _assert_equals_fresh(engine, ix, cur, "l2", SCRIPT_PLANES, None, Q, tmp_path, what)
            for got, want, name in zip(tables[1:], model, ("codes", "off", "ids")):
                np.testing.assert_array_equal(got, want, err_msg="%s: %s against the model" % (what, name))
            for t, b, members in expect:
                assert bucket(tables, t, b) == members, "%s: bucket %d of table %d" % (what, b, t)
            for t in range(2):                              # a table in which no row of the call moved is what it was
                if all(moves[r][t] == before[1][r, t] for r in ids):
                    np.testing.assert_array_equal(tables[2][t], before[2][t], err_msg=what)
                    np.testing.assert_array_equal(tables[3][t], before[3][t], err_msg=what)


# ---- 2. updated equals fresh ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,dim", CASES, ids=CASE_IDS)
def test_updated_handle_equals_fresh_handle(native_lib, tmp_path, metric, dim):
    from hnsw_clj_amd import engine

    rows, Q = _data(dim)
    rng = np.random.default_rng(11 * dim)
    with _built(engine, rows, metric, dim, Q) as ix:
        planes, codes0, off0, ids0 = ix.lsh_get()
        cur, model = rows, (codes0, off0, ids0)
        for m in (1, 63, 64, 65, 257):                      # scattered rows
            ids = rng.choice(N, m, replace=False).astype(np.int32)
            new = _new_values(rng, cur, ids)
            cur = _update(ix, cur, ids, new)
            tables = _assert_equals_fresh(engine, ix, cur, metric, planes, _mode_of(dim), what="m %d" % m)
            model = U.merge(*model, ids, tables[1][ids])    # (the codes are the device's; the buckets are the model's)
            for got, want, name in zip(tables[1:], model, ("codes", "off", "ids")):
                np.testing.assert_array_equal(got, want, err_msg="m %d: %s against the model" % (m, name))
            stay = tables[1][ids] == codes0[ids]
            assert m < 63 or (stay.any() and not stay.all()), "m %d: the call has no stayers or no movers" % m
            codes0 = tables[1]
        _assert_equals_fresh(engine, ix, cur, metric, planes, _mode_of(dim), Q, tmp_path, "scattered calls")
        ids = np.arange(N, dtype=np.int32)                  # m = n
        cur = _update(ix, cur, ids, _new_values(rng, cur, ids))
        _assert_equals_fresh(engine, ix, cur, metric, planes, _mode_of(dim), Q, tmp_path, "m = n")


@pytest.mark.parametrize("metric,dim", CASES, ids=CASE_IDS)
def test_the_same_values_again_change_nothing(native_lib, metric, dim):
    from hnsw_clj_amd import engine

    rows, Q = _data(dim)
    rng = np.random.default_rng(12 * dim)
    with _built(engine, rows, metric, dim, Q) as ix:
        planes = ix.lsh_get()[0]
        ids = rng.choice(N, 300, replace=False).astype(np.int32)
        cur = _update(ix, rows, ids, _new_values(rng, rows, ids))
        before, norms = ix.lsh_get(), ix.norms()
        answer = ix.lsh_search(Q, K)
        again = rng.choice(N, 257, replace=False).astype(np.int32)
        for pick in (ids, again, np.arange(N, dtype=np.int32)):
            _update(ix, cur, pick, cur[pick])
            assert _tables_equal(ix.lsh_get(), before)
            np.testing.assert_array_equal(_bits(ix.norms()), _bits(norms))
            _same(ix.lsh_search(Q, K), answer, "the same values again")
        _assert_equals_fresh(engine, ix, cur, metric, planes, _mode_of(dim))


@pytest.mark.parametrize("metric,dim", CASES, ids=CASE_IDS)
def test_one_bucket_per_table_receives_every_row_of_the_call(native_lib, metric, dim):
    from hnsw_clj_amd import engine

    rows, Q = _data(dim)
    rng = np.random.default_rng(13 * dim)
    value = rng.standard_normal(dim).astype(np.float32)
    with _built(engine, rows, metric, dim, Q) as ix:
        planes = ix.lsh_get()[0]
        cur = rows
        for m in (65, 700):                                 # the second call's joiners land between the first call's
            ids = rng.choice(N, m, replace=False).astype(np.int32)
            cur = _update(ix, cur, ids, np.repeat(value[None, :], m, axis=0))
            _, codes, off, bids = _assert_equals_fresh(engine, ix, cur, metric, planes, _mode_of(dim), Q[:3], what="m %d" % m)
            code = ix.lsh_hash(value)[0]
            for t in range(TABLES):
                members = bids[t, off[t, code[t]]:off[t, code[t] + 1]]
                assert np.isin(ids, members).all() and (np.diff(members) > 0).all()


@pytest.mark.parametrize("metric,dim", CASES, ids=CASE_IDS)
def test_the_handle_does_not_depend_on_order_or_split(native_lib, metric, dim):
    from hnsw_clj_amd import engine

    rows, Q = _data(dim)
    rng = np.random.default_rng(14 * dim)
    ids = np.sort(rng.choice(N, 400, replace=False)).astype(np.int32)
    new = _new_values(rng, rows, ids)
    want = U.apply(rows, ids, new)
    perm = rng.permutation(len(ids))
    with _built(engine, rows, metric, dim, Q) as one:
        planes = one.lsh_get()[0]
        _update(one, rows, ids, new)
        expect = _assert_equals_fresh(engine, one, want, metric, planes, _mode_of(dim), Q, what="one call, ascending ids")
        norms, answer = one.norms(), one.lsh_search(Q, K)
    orders = {"descending ids": [np.arange(len(ids))[::-1]], "shuffled ids": [perm],
              "three calls": [perm[:1], perm[1:130], perm[130:]]}
    for what, calls in orders.items():
        with _built(engine, rows, metric, dim, Q) as ix:
            cur = rows
            for at in calls:
                cur = _update(ix, cur, ids[at], new[at])
            np.testing.assert_array_equal(_bits(cur), _bits(want))
            assert _tables_equal(ix.lsh_get(), expect), what
            np.testing.assert_array_equal(_bits(ix.norms()), _bits(norms), err_msg=what)
            _same(ix.lsh_search(Q, K), answer, what)


# ---- 3. more buckets than the cursors in LDS hold ---------------------------------------------------------------------------
def test_bits_13_the_cursors_in_global_memory(native_lib):
    from hnsw_clj_amd import engine

    n, dim = 700, 20
    rng = np.random.default_rng(1300)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    planes = rng.standard_normal((2, 13, dim)).astype(np.float32)
    with engine.Index(rows, "dot", 0) as ix:
        ix.set_lsh(planes)
        model = ix.lsh_get()[1:]
        cur = rows
        for m in (1, 65, 300, n):
            ids = rng.choice(n, m, replace=False).astype(np.int32)
            new = _new_values(rng, cur, ids)
            if m == 300:
                new[100:] = new[0]                          # 200 rows of one bucket: several steps of the walk move one cursor
            cur = _update(ix, cur, ids, new)
            tables = _assert_equals_fresh(engine, ix, cur, "dot", planes, None, what="bits 13, m %d" % m)
            model = U.merge(*model, ids, tables[1][ids])
            for got, want, name in zip(tables[1:], model, ("codes", "off", "ids")):
                np.testing.assert_array_equal(got, want, err_msg="bits 13, m %d: %s against the model" % (m, name))


# ---- 4. a zero row and a NaN row --------------------------------------------------------------------------------------------
def test_a_zero_row_and_a_nan_row(native_lib):
    from hnsw_clj_amd import engine

    rows, _ = _data(20)
    base = rows[:600]
    new = np.zeros((3, 20), np.float32)
    new[1] = np.nan
    new[2] = base[7]
    new[2, 3] = np.nan
    ids = np.array([599, 0, 300], np.int32)
    with engine.Index(base, "cosine", 0) as ix:
        ix.lsh_build(TABLES, BITS, 64, 42)
        planes = ix.lsh_get()[0]
        cur = _update(ix, base, ids, new)
        _, codes, _, _ = _assert_equals_fresh(engine, ix, cur, "cosine", planes, None, what="zero and NaN rows")
        assert (codes[599] == (1 << BITS) - 1).all(), "0.0 >= 0.0: every bit of the zero row is set"
        assert (codes[0] == 0).all(), "NaN >= 0.0 is false: no bit of the NaN row is set"
        norms = ix.norms()
        assert norms[599] == 0 and np.isnan(norms[0]) and np.isnan(norms[300])
        cur = _update(ix, cur, ids, base[ids])              # ... and back
        tables = _assert_equals_fresh(engine, ix, cur, "cosine", planes, None, what="back from zero and NaN rows")
        with _fresh(engine, base, "cosine", planes) as fresh:
            assert _tables_equal(tables, fresh.lsh_get())


# ---- 5. a chain of mutations ------------------------------------------------------------------------------------------------
def test_add_update_remove_update(native_lib, tmp_path):
    from hnsw_clj_amd import engine

    rows, Q = _data(136)
    n0 = 1000
    rng = np.random.default_rng(5)
    with engine.Index(rows[:n0], "l2", 0) as ix:
        ix.set_rejection_test(2)
        ix.lsh_build(TABLES, BITS, 64, 42)
        _touch(ix, Q)
        planes = ix.lsh_get()[0]
        ix.lsh_add(rows[n0:n0 + 257])
        cur = rows[:n0 + 257]
        ids = np.concatenate([rng.choice(n0, 100, replace=False), n0 + rng.choice(257, 50, replace=False)]).astype(np.int32)
        cur = _update(ix, cur, ids, _new_values(rng, cur, ids))
        gone = np.concatenate([ids[:40], rng.choice(n0 + 257, 60, replace=False)])
        cur = cur[TLR._remove(ix, gone)]
        ids = rng.choice(len(cur), 129, replace=False).astype(np.int32)       # in the numbering that is current now
        new = _new_values(rng, cur, ids)
        cur = _update(ix, cur, ids, new)
        _assert_equals_fresh(engine, ix, cur, "l2", planes, 2, Q, tmp_path, "add, update, remove, update")
        # under a mask that lets only the updated rows pass, a row's new value finds the row itself
        allow = engine.pack_mask(np.isin(np.arange(len(cur)), ids), len(cur))
        gi, gd = ix.lsh_search_filtered(new[:NQ], K, allow, TABLES, 0, 2 * K, K)
        np.testing.assert_array_equal(gi[:, 0], ids[:NQ])
        assert np.isin(gi[gi >= 0], ids).all()


# ---- 6. refusals, their order, and the handle afterwards --------------------------------------------------------------------
def test_refusals_leave_the_handle_alone(native_lib):
    from hnsw_clj_amd import engine

    L = native_lib.lib()
    rows, Q = _data(20)
    base = rows[:500]
    value = np.ascontiguousarray(rows[600:604])
    vptr = value.ctypes.data_as(ctypes.c_void_p)

    def ids(*v):
        a = np.array(v, np.int32)
        return a, a.ctypes.data_as(ctypes.c_void_p)

    one, ptr = ids(3)

    def state(ix):
        return ix.lsh_get(), ix.lsh_search(Q[:5], K), ix.norms()

    def refused(ix, p, v, m, code, word=None, before=None):
        assert L.hnswgpu_lsh_update(ix._h, p, v, m) == code
        if word:
            assert word in L.hnswgpu_last_error().lower(), L.hnswgpu_last_error()
        if before is not None:                                # every refusal leaves n, the tables, the norms and a search's bits alone
            what = "after a refusal with code %d (%s)" % (code, word)
            assert ix.n == 500 and _native_n(ix) == 500
            tables, answer, norms = state(ix)
            assert _tables_equal(tables, before[0]), what
            _same(answer, before[1], what)
            np.testing.assert_array_equal(_bits(norms), _bits(before[2]), err_msg=what)

    with engine.Index(base, "cosine", 0) as bare:
        refused(bare, None, vptr, 1, -1, b"ids is null")      # the arguments come before the state of the handle
        refused(bare, ptr, vptr, 0, 0)                        # nothing to update: nothing is looked at
        refused(bare, ptr, vptr, 1, -3, b"no lsh tables")
        _, p = ids(3, 777)
        refused(bare, p, vptr, 2, -3, b"no lsh tables")       # ... and the state before the ids
        assert bare.n == 500 and bare.lsh_sizes() == (0, 0)
    with engine.Index(base, "cosine", 0) as ix:
        ix.lsh_build(TABLES, BITS, 64, 42)
        before = state(ix)
        refused(ix, None, vptr, 1, -1, b"ids is null", before)
        refused(ix, ptr, None, 1, -1, b"rows is null", before)
        refused(ix, ptr, vptr, -1, -1, None, before)
        for bad in (-1, 500):
            _, p = ids(3, 4, bad, 5)
            refused(ix, p, vptr, 4, -1, b"not a row", before)
        _, p = ids(3, 4, 5, 4)
        refused(ix, p, vptr, 4, -1, b"named twice", before)
        _, p = ids(4, 4, 500)
        refused(ix, p, vptr, 3, -1, b"not a row", before)     # the range before the repeats
        refused(ix, ptr, vptr, 0, 0, None, before)            # nothing to update: nothing happens
        refused(ix, None, None, 0, 0, None, before)
        ix.hnsw_build(8, 40, 42)
        refused(ix, ptr, vptr, 1, -3, b"graph", before)
        _, p = ids(3, 3)
        refused(ix, p, vptr, 2, -3, b"graph", before)         # the other structure before the ids
    with engine.Index(base, "cosine", 0) as lists:
        lists.ivf_build(8, 2, 42)
        lists.set_lsh(before[0][0])
        refused(lists, ptr, vptr, 1, -3, b"ivf", before)
    with engine.Index(base, "cosine", 0) as forest:
        forest.hnsw_build_parts([0, 250, 500], 8, 40, 42)
        forest.set_lsh(before[0][0])
        refused(forest, ptr, vptr, 1, -3, b"forest", before)
    with engine.Index(base[:40], "cosine", 0) as empty:       # n == 0 with m > 0: no id is a row
        empty.set_lsh(before[0][0])
        empty.lsh_remove(np.arange(40))
        _, p = ids(0)
        refused(empty, p, vptr, 1, -1, b"not a row")
        assert empty.n == 0 and _native_n(empty) == 0 and empty.lsh_sizes() == (TABLES, BITS)
        assert not empty.lsh_get()[2].any()
        refused(empty, p, vptr, 0, 0)
    with engine.Index(base, "cosine", 0) as ix:               # ... and the handle after all that is a handle that updates
        ix.set_lsh(before[0][0])
        assert L.hnswgpu_lsh_update(ix._h, ptr, vptr, 1) == 0
        with _fresh(engine, U.apply(base, one, value[:1]), "cosine", before[0][0]) as fresh:
            TLR._assert_same_tables(ix, fresh)


# ---- 7. searches beside updates ---------------------------------------------------------------------------------------------
def test_searches_beside_updates_see_one_of_the_index_states(native_lib):
    from hnsw_clj_amd import engine

    n0, step = 700, 50
    rows, Q = _data(32, n0)
    q = np.ascontiguousarray(Q[:8])
    rng = np.random.default_rng(8)
    updates, bases = [], [rows]
    for _ in range(3):
        ids = rng.choice(n0, step, replace=False).astype(np.int32)
        updates.append((ids, _new_values(rng, bases[-1], ids)))
        bases.append(U.apply(bases[-1], *updates[-1]))
    with engine.Index(rows, "l2", 0) as ix:
        ix.lsh_build(TABLES, BITS, 64, 42)
        planes = ix.lsh_get()[0]
        states = []                                          # per index state: (ids, distance bits), from fresh handles
        for now in bases:
            with _fresh(engine, now, "l2", planes) as fresh:
                i, d = fresh.lsh_search(q, K)
                states.append((i, _bits(d)))
        stop, errors, seen = threading.Event(), [], [set(), set()]

        def matches(i, d):
            return [s for s in range(4) if np.array_equal(i, states[s][0]) and np.array_equal(_bits(d), states[s][1])]

        def searcher(t):
            try:
                for _ in range(20000):                       # bounded: the updater sets `stop` long before
                    if stop.is_set():
                        break
                    hit = matches(*ix.lsh_search(q, K))
                    if not hit:
                        raise AssertionError("thread %d: an answer that belongs to none of the four index states" % t)
                    seen[t].update(hit)
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
                stop.set()

        def updater():
            try:
                for s, (ids, new) in enumerate(updates):
                    if stop.is_set():
                        return
                    ix.lsh_update(ids, new)
                    assert s + 1 in matches(*ix.lsh_search(q, K)), "the updated index is what every later search sees"
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
            finally:
                stop.set()

        threads = [threading.Thread(target=searcher, args=(t,), daemon=True) for t in range(2)]
        threads.append(threading.Thread(target=updater, daemon=True))
        for th in threads:
            th.start()
        for th in threads:
            th.join(STEP_SECONDS)
            assert not th.is_alive(), "a thread did not finish within its time limit"
        assert not errors, errors[0]
        assert ix.n == n0
        assert 3 in matches(*ix.lsh_search(q, K))


# ---- 8. the Python mirror ---------------------------------------------------------------------------------------------------
def test_python_mirror_update_vectors(native_lib):
    from hnsw_clj_amd import hybrid_lsh as H

    rows, _ = _data(20)
    n0 = 600
    index = H.build_index([("v-%d" % i, rows[i]) for i in range(n0)], show_progress=False)
    try:
        assert H.search_knn(index, rows[33], 5)[0]["id"] == "v-33"
        assert H.update_vectors(index, [("v-33", rows[700]), ("v-0", rows[701])]) is index
        assert H.index_info(index)["vectors"] == n0 and len(index.ids) == n0
        res = H.search_knn(index, rows[700], 5)
        assert res[0]["id"] == "v-33" and abs(res[0]["distance"]) <= 1e-5
        assert H.search_knn(index, rows[701], 5)[0]["id"] == "v-0"
        got = H.search_knn(index, rows[33], 5)
        assert not got or got[0]["id"] != "v-33" or got[0]["distance"] > 1e-3      # the old value is gone
        with pytest.raises(KeyError):
            H.update_vectors(index, [("v-1", rows[702]), ("w-9", rows[703])])
        assert H.search_knn(index, rows[1], 5)[0]["id"] == "v-1"                    # ... nothing was updated, not even v-1
        assert H.update_vectors(index, []) is index
    finally:
        index.close()
