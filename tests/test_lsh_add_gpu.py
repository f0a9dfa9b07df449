"""hnswgpu_lsh_add on the device: a handle that grew is indistinguishable, bit for bit, from a fresh handle over all the rows that
was given the same hyperplanes through set_lsh -- lsh_get array for array, every search's ids and distance BITS, norms, the saved
file's bytes.  The fresh handle's buckets come from the host counting sort of a build, its codes are pinned to the CPU oracle by
test_lsh_gpu.py: two independent implementations have to agree.  As yardsticks that run none of the code under test: the numpy
counting sort (lsh_model.buckets) for every table, and for one case the numpy search model fed the oracle's device-order
distances."""
import ctypes
import threading

import numpy as np
import pytest

import lsh_model as M
from util import assert_exact

pytestmark = pytest.mark.gpu

N0, M_ADD, NQ, K = 1500, 1000, 33, 10
STEP_SECONDS = 60          # the time limit of one step of the threaded test
# (num_probes, probe_radius, take_main, take_flip): the five modes and search-hybrid's default form, as in test_lsh_gpu.py
CONFIGS = [(p, r, 2 * K, K) for p, r in M.MODES.values()] + [(2, 0, 3 * K, K)]
_DATA = {}


def _data(dim, n=N0 + M_ADD):
    """(rows f32 [n, dim], queries f32 [NQ, dim], every other query near a row); made once per shape."""
    if (dim, n) not in _DATA:
        rng = np.random.default_rng(1000 * dim + n)
        rows = rng.standard_normal((n, dim)).astype(np.float32)
        Q = rng.standard_normal((NQ, dim)).astype(np.float32)
        near = rng.integers(0, n, (NQ + 1) // 2)
        Q[::2] = rows[near] + 0.05 * rng.standard_normal((len(near), dim)).astype(np.float32)
        _DATA[(dim, n)] = (rows, Q)
    return _DATA[(dim, n)]


def _bits(d):
    return np.ascontiguousarray(d, np.float32).view(np.uint32)


def _same(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=what + ": ids")
    np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]), err_msg=what + ": distance bits")


def _fresh(engine, rows, metric, planes, mode=None):
    ix = engine.Index(rows, metric, 0)
    if mode is not None:                                    # None: the mode new handles get
        ix.set_rejection_test(mode)
    ix.set_lsh(planes)
    return ix


def _assert_same_tables(grown, fresh, what=""):
    """lsh_get array for array, and the buckets against the numpy counting sort of the codes"""
    gp, gc, go, gi = grown.lsh_get()
    fp, fc, fo, fi = fresh.lsh_get()
    assert grown.n == fresh.n and grown.lsh_sizes() == fresh.lsh_sizes()
    np.testing.assert_array_equal(_bits(gp), _bits(fp), err_msg=what + ": planes")
    np.testing.assert_array_equal(gc, fc, err_msg=what + ": codes")
    np.testing.assert_array_equal(go, fo, err_msg=what + ": off")
    np.testing.assert_array_equal(gi, fi, err_msg=what + ": ids")
    eo, ei = M.buckets(gc, grown.lsh_sizes()[1])
    np.testing.assert_array_equal(go, eo, err_msg=what + ": off against the counting sort")
    np.testing.assert_array_equal(gi, ei, err_msg=what + ": ids against the counting sort")
    return gp, gc, go, gi


def _tables_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _dense(O, base, Q, metric):
    """Every query's device-order distance to every row, [nq][n] (-0 canonicalised as the keys do); as in test_lsh_gpu.py"""
    om = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    ids, d, _ = O.exact_knn(base, Q, len(base), metric=om, mode=O.MODE_DEV)
    D = np.empty((len(Q), len(base)), np.float64)
    np.put_along_axis(D, ids.astype(np.int64), d, axis=1)
    return D + 0.0


# ---- 1. grown equals fresh ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2"])
@pytest.mark.parametrize("dim", [20, 136])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_grown_handle_equals_fresh_handle(native_lib, oracle, tmp_path, metric, dim, mode):
    from hnsw_clj_amd import engine

    rows, Q = _data(dim)
    n1 = N0 + M_ADD
    with engine.Index(rows[:N0], metric, 0) as grown:
        grown.set_rejection_test(mode)
        grown.lsh_build(8, 6, 64, 42)                       # buckets of about 23 rows: every call puts rows into most of them
        planes = grown.lsh_get()[0]
        at = N0
        for m in (1, 63, 64, 65, 255, 257, M_ADD - (1 + 63 + 64 + 65 + 255 + 257)):
            got = grown.lsh_add(rows[at:at + m])
            np.testing.assert_array_equal(got, np.arange(at, at + m, dtype=np.int32))
            at += m
        assert grown.n == n1 and at == n1
        with _fresh(engine, rows, metric, planes, mode) as fresh:
            _, codes, off, ids = _assert_same_tables(grown, fresh)
            np.testing.assert_array_equal(grown.lsh_hash(rows[N0:]), codes[N0:], err_msg="a row's code depends on how it came")
            for cfg in CONFIGS:
                for nq in (1, NQ):
                    _same(grown.lsh_search(Q[:nq], K, *cfg), fresh.lsh_search(Q[:nq], K, *cfg), "lsh_search %s nq %d" % (cfg, nq))
            _same(grown.exact_knn(Q[:5], K), fresh.exact_knn(Q[:5], K), "exact_knn")
            np.testing.assert_array_equal(_bits(grown.norms()), _bits(fresh.norms()), err_msg="norms")
            pick = np.array([N0, n1 - 1, (N0 + n1) // 2, 0], np.int32)
            np.testing.assert_array_equal(_bits(grown.batch_distances(Q[0], ids=pick)), _bits(fresh.batch_distances(Q[0], ids=pick)),
                                          err_msg="batch_distances")
            fa, fb = tmp_path / "grown.idx", tmp_path / "fresh.idx"
            grown.save(fa)
            fresh.save(fb)
            assert fa.read_bytes() == fb.read_bytes(), "the saved files differ"
            with engine.Index.load(fa, 0) as back:
                assert back.n == n1 and back.lsh_sizes() == (0, 0)
        if metric == "cosine" and dim == 20 and mode == 2:  # ... and to the model, not only to its twin
            D = _dense(oracle, rows, Q, metric)
            qcodes = grown.lsh_hash(Q)
            for cfg in CONFIGS:
                gi, gd = grown.lsh_search(Q, K, *cfg)
                ei, ed = M.search_batch(D, qcodes, off, ids, 6, K, *cfg)
                assert_exact(gi, gd, ei, ed, "grown handle against the model %s" % (cfg,))


# ---- 2. split independence ------------------------------------------------------------------------------------------------
def test_tables_do_not_depend_on_how_the_rows_were_split(native_lib):
    from hnsw_clj_amd import engine

    rows, _ = _data(20)
    with engine.Index(rows[:N0], "cosine", 0) as one, engine.Index(rows[:N0], "cosine", 0) as many:
        one.lsh_build(8, 6, 64, 42)
        many.lsh_build(8, 6, 64, 42)
        one.lsh_add(rows[N0:])
        for at in range(N0, N0 + M_ADD, 7):
            many.lsh_add(rows[at:min(at + 7, N0 + M_ADD)])
        a, b = one.lsh_get(), many.lsh_get()
        assert _tables_equal(a, b)
        assert (a[2][:, -1] == N0 + M_ADD).all() and (np.sort(a[3], axis=1) == np.arange(N0 + M_ADD)).all()


# ---- 3. bucket shapes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables,bits", [(1, 1), (16, 1), (3, 5), (8, 12), (2, 16), (16, 16)])
def test_bucket_shapes(native_lib, tables, bits):
    """bits 1: every row of a step collides, the ranks run to m.  bits 12: most buckets are empty and get their first rows.
    bits 16: the 65,537-entry scan, the cursors beyond LDS, and (16, 16) both limits at once."""
    from hnsw_clj_amd import engine

    n0, m = 300, 330
    rng = np.random.default_rng(100 * tables + bits)
    rows = rng.standard_normal((n0 + m, 20)).astype(np.float32)
    planes = rng.standard_normal((tables, bits, 20)).astype(np.float32)
    with engine.Index(rows[:n0], "dot", 0) as grown:
        grown.set_lsh(planes)
        grown.lsh_add(rows[n0:n0 + 65])
        grown.lsh_add(rows[n0 + 65:])
        with _fresh(engine, rows, "dot", planes) as fresh:
            _assert_same_tables(grown, fresh, "%d x %d" % (tables, bits))


# ---- 4. twins -------------------------------------------------------------------------------------------------------------
def _twin_base(n0=300, dim=20):
    rng = np.random.default_rng(44)
    return rng.standard_normal((n0, dim)).astype(np.float32), rng.standard_normal(dim).astype(np.float32)


@pytest.mark.parametrize("m", [1, 64, 65, 1025])
def test_copies_of_one_new_vector_share_a_bucket_in_every_table(native_lib, m):
    """The ranks cross the wave and more: copy j sits j places behind the bucket's old members, in every table."""
    from hnsw_clj_amd import engine

    base, v = _twin_base()
    n0 = len(base)
    new = np.repeat(v[None, :], m, axis=0)
    with engine.Index(base, "l2", 0) as grown:
        grown.lsh_build(8, 6, 64, 42)
        planes = grown.lsh_get()[0]
        grown.lsh_add(new)
        with _fresh(engine, np.concatenate([base, new]), "l2", planes) as fresh:
            _, codes, off, ids = _assert_same_tables(grown, fresh, "m %d" % m)
            for t in range(8):
                b = int(codes[n0, t])
                assert (codes[n0:, t] == b).all()
                assert ids[t, off[t, b + 1] - m:off[t, b + 1]].tolist() == list(range(n0, n0 + m))
            got = grown.lsh_search(v, K, 8, 0, 30, 10)
            _same(got, fresh.lsh_search(v, K, 8, 0, 30, 10), "twins, m %d" % m)
            # equal distance bits: ordered by their position in the bucket, which is id order
            assert got[0][0, :min(m, K)].tolist() == list(range(n0, n0 + min(m, K)))
            assert (_bits(got[1][0, :min(m, K)]) == _bits(got[1][0, :1])).all()


def test_copies_of_a_base_row_line_up_behind_it(native_lib):
    from hnsw_clj_amd import engine

    base, _ = _twin_base()
    n0, r = len(base), 123
    new = np.repeat(base[r][None, :], 70, axis=0)
    with engine.Index(base, "l2", 0) as grown:
        grown.lsh_build(8, 6, 64, 42)
        planes = grown.lsh_get()[0]
        grown.lsh_add(new)
        with _fresh(engine, np.concatenate([base, new]), "l2", planes) as fresh:
            _assert_same_tables(grown, fresh)
            got = grown.lsh_search(base[r], K, 8, 0, 30, 10)
            _same(got, fresh.lsh_search(base[r], K, 8, 0, 30, 10), "copies of a base row")
            assert got[0][0].tolist() == [r] + list(range(n0, n0 + K - 1))


# ---- 5. from nothing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0", [0, 1])
def test_add_to_an_empty_or_one_row_handle(native_lib, n0):
    from hnsw_clj_amd import engine

    rng = np.random.default_rng(16)
    rows = rng.standard_normal((n0 + 300, 16)).astype(np.float32)
    with engine.Index(rows[:n0].reshape(n0, 16), "cosine", 0) as grown:
        grown.lsh_build()
        planes = grown.lsh_get()[0] if n0 else None
        got = grown.lsh_add(rows[n0:])
        np.testing.assert_array_equal(got, np.arange(n0, n0 + 300, dtype=np.int32))
        if planes is None:
            planes = grown.lsh_get()[0]
        with _fresh(engine, rows, "cosine", planes) as fresh:
            _assert_same_tables(grown, fresh, "from %d rows" % n0)
            _same(grown.lsh_search(rows[:7], K), fresh.lsh_search(rows[:7], K), "from %d rows" % n0)
            np.testing.assert_array_equal(_bits(grown.norms()), _bits(fresh.norms()))


# ---- 6. refusals leave the handle alone -----------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone(native_lib):
    from hnsw_clj_amd import engine

    L = native_lib.lib()
    rows, Q = _data(20)
    base, one = rows[:500], np.ascontiguousarray(rows[N0:N0 + 1])
    ptr = one.ctypes.data_as(ctypes.c_void_p)

    def state(ix):
        return ix.lsh_get(), ix.lsh_search(Q[:5], K)

    def unchanged(ix, before, what):
        assert ix.n == 500
        tables, answer = state(ix)
        assert _tables_equal(tables, before[0]), what
        _same(answer, before[1], what)

    def refused(ix, p, m, code, word=None, before=None):
        assert L.hnswgpu_lsh_add(ix._h, p, m) == code
        if word:
            assert word in L.hnswgpu_last_error().lower()
        if before is not None:                                # every refusal leaves n, the tables and a search's bits alone
            unchanged(ix, before, "after a refusal with code %d (%s)" % (code, word))

    with engine.Index(base, "cosine", 0) as bare:
        refused(bare, ptr, 1, -3, b"no lsh tables")
        assert L.hnswgpu_lsh_add(bare._h, None, 0) == 0       # nothing to add: nothing is looked at
        assert bare.n == 500 and bare.lsh_sizes() == (0, 0)
    with engine.Index(base, "cosine", 0) as ix:
        ix.lsh_build(8, 6, 64, 42)
        before = state(ix)
        refused(ix, None, 1, -1, b"rows is null", before)
        refused(ix, ptr, -1, -1, None, before)
        refused(ix, ptr, 2 ** 31, -5, b"2^31", before)       # refused before the one-row buffer is read
        refused(ix, ptr, 0, 0, None, before)                  # nothing to add: nothing happens
        refused(ix, None, 0, 0, None, before)
        ix.hnsw_build(8, 40, 42)
        refused(ix, ptr, 1, -3, b"graph", before)
    with engine.Index(base, "cosine", 0) as lists:
        lists.ivf_build(8, 2, 42)
        lists.set_lsh(before[0][0])
        refused(lists, ptr, 1, -3, b"ivf", before)
    with engine.Index(base, "cosine", 0) as forest:
        forest.hnsw_build_parts([0, 250, 500], 8, 40, 42)
        forest.set_lsh(before[0][0])
        refused(forest, ptr, 1, -3, b"forest", before)


# ---- 7. searches beside adds ----------------------------------------------------------------------------------------------
def test_searches_beside_adds_see_one_of_the_index_states(native_lib):
    from hnsw_clj_amd import engine

    n0, step = 500, 50
    rows, Q = _data(32, n0 + 4 * step)
    q = np.ascontiguousarray(Q[:8])
    cuts = [n0 + i * step for i in range(5)]
    with engine.Index(rows[:n0], "l2", 0) as ix:
        ix.lsh_build(8, 6, 64, 42)
        planes = ix.lsh_get()[0]
        states = []                                          # per index state: (ids, distance bits), from fresh handles
        for n in cuts:
            with _fresh(engine, rows[:n], "l2", planes) as fresh:
                i, d = fresh.lsh_search(q, K)
                states.append((i, _bits(d)))
        stop, errors, seen = threading.Event(), [], [set(), set()]

        def matches(i, d):
            return [s for s in range(5) if np.array_equal(i, states[s][0]) and np.array_equal(_bits(d), states[s][1])]

        def searcher(t):
            try:
                for _ in range(20000):                       # bounded: the adder sets `stop` long before
                    if stop.is_set():
                        break
                    hit = matches(*ix.lsh_search(q, K))
                    if not hit:
                        raise AssertionError("thread %d: an answer that belongs to none of the five index states" % t)
                    seen[t].update(hit)
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
                stop.set()

        def adder():
            try:
                for s, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                    if stop.is_set():
                        return
                    ix.lsh_add(rows[a:b])
                    assert s + 1 in matches(*ix.lsh_search(q, K)), "the grown index is what every later search sees"
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
            finally:
                stop.set()

        threads = [threading.Thread(target=searcher, args=(t,), daemon=True) for t in range(2)]
        threads.append(threading.Thread(target=adder, daemon=True))
        for th in threads:
            th.start()
        for th in threads:
            th.join(STEP_SECONDS)
            assert not th.is_alive(), "a thread did not finish within its time limit"
        assert not errors, errors[0]
        assert ix.n == cuts[-1]
        assert matches(*ix.lsh_search(q, K)) and 4 in matches(*ix.lsh_search(q, K))


# ---- 8. the Python mirror -------------------------------------------------------------------------------------------------
def test_python_mirror_add_vectors(native_lib):
    from hnsw_clj_amd import hybrid_lsh as H
    from hnsw_clj_amd import protocol

    rows, _ = _data(20)
    n0, m = 600, 70
    data = [("old-%d" % i, rows[i]) for i in range(n0)]
    more = [("new-%d" % i, rows[N0 + i]) for i in range(m)]
    index = H.build_index(data, show_progress=False)
    try:
        assert H.add_vectors(index, more) is index
        assert H.index_info(index)["vectors"] == n0 + m and len(index.ids) == n0 + m
        for i in (0, 33, m - 1):
            res = H.search_knn(index, rows[N0 + i], 5)
            assert res[0]["id"] == "new-%d" % i and abs(res[0]["distance"]) <= 1e-5
        batch = protocol.GpuHybridLshIndex(index).search_batch_star(rows[N0:N0 + 3], 5, "fast")
        assert [r[0]["id"] for r in batch] == ["new-0", "new-1", "new-2"]
        assert H.add_vectors(index, []) is index and H.index_info(index)["vectors"] == n0 + m
    finally:
        index.close()
