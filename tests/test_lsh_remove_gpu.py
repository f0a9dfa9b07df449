"""hnswgpu_lsh_remove on the device: a handle that shrank is indistinguishable, bit for bit, from a fresh handle over the kept rows
in their old order that was given the same hyperplanes through set_lsh -- lsh_get array for array, every search's ids and
distance BITS, norms, the saved file's bytes.  The fresh handle's buckets come from the host counting sort of a build.  As
yardsticks that run none of the code under test: the numpy removal (lsh_remove_model.compact), the numpy counting sort
(lsh_model.buckets), and for one case the numpy search model fed the oracle's device-order distances.  And between two device
paths, neither of them the fresh handle: a removal is the permanent form of the allow-mask of the filtered search."""
import ctypes
import threading

import numpy as np
import pytest

import lsh_model as M
import lsh_remove_model as R
from util import assert_exact

pytestmark = pytest.mark.gpu

N, NQ, K = 2500, 33, 10    # 2500 = 78 x 32 + 4: the last mask word is partial
STEP_SECONDS = 60          # the time limit of one step of the threaded test
# (num_probes, probe_radius, take_main, take_flip): the five modes and search-hybrid's default form, as in test_lsh_gpu.py
CONFIGS = [(p, r, 2 * K, K) for p, r in M.MODES.values()] + [(2, 0, 3 * K, K)]
_DATA = {}


def _data(dim, n=N):
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


def _assert_same_tables(shrunk, fresh, what=""):
    """lsh_get array for array, and the buckets against the numpy counting sort of the codes"""
    gp, gc, go, gi = shrunk.lsh_get()
    fp, fc, fo, fi = fresh.lsh_get()
    assert shrunk.n == fresh.n and shrunk.lsh_sizes() == fresh.lsh_sizes()
    np.testing.assert_array_equal(_bits(gp), _bits(fp), err_msg=what + ": planes")
    np.testing.assert_array_equal(gc, fc, err_msg=what + ": codes")
    np.testing.assert_array_equal(go, fo, err_msg=what + ": off")
    np.testing.assert_array_equal(gi, fi, err_msg=what + ": ids")
    eo, ei = M.buckets(gc, shrunk.lsh_sizes()[1])
    np.testing.assert_array_equal(go, eo, err_msg=what + ": off against the counting sort")
    np.testing.assert_array_equal(gi, ei, err_msg=what + ": ids against the counting sort")
    return gp, gc, go, gi


def _native_n(ix):
    """the handle's own row count (hnswgpu_info), beside engine.Index.n"""
    from hnsw_clj_amd import _native

    n = ctypes.c_int64(-1)
    assert _native.lib().hnswgpu_info(ix._h, ctypes.byref(n), None, None, None, None) == 0
    return n.value


def _tables_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _remove(ix, rows):
    """lsh_remove through the ABI with n_after, checked against the model: returns kept (old ids that remain)"""
    n0 = ix.n
    expect = R.kept(n0, rows)
    kept = ix.lsh_remove(rows)                              # (asserts n_after == len(kept) itself)
    assert kept.dtype == np.int64
    np.testing.assert_array_equal(kept, expect)
    assert ix.n == len(expect) == _native_n(ix)
    return kept


def _dense(O, base, Q, metric):
    """Every query's device-order distance to every row, [nq][n] (-0 canonicalised as the keys do); as in test_lsh_gpu.py"""
    om = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    ids, d, _ = O.exact_knn(base, Q, len(base), metric=om, mode=O.MODE_DEV)
    D = np.empty((len(Q), len(base)), np.float64)
    np.put_along_axis(D, ids.astype(np.int64), d, axis=1)
    return D + 0.0


def _removals(seed):
    """The sequence of case 1, each list in the numbering that is CURRENT when its turn comes (n = rows at that time)"""
    rng = np.random.default_rng(seed)
    yield lambda n: [0]
    yield lambda n: [n - 1]
    yield lambda n: np.arange(64, 96)                       # one aligned word
    yield lambda n: np.arange(31, 64)                       # 33 rows over two word boundaries
    for m in (63, 64, 65):
        yield lambda n, m=m: rng.choice(n, m, replace=False)
    yield lambda n: np.arange(0, n, 2)                      # every other remaining row
    yield lambda n: np.concatenate([np.arange(n - 1, n - 200, -3), [5, 5, n - 1, 7, 5]])   # descending, with repeats


# ---- 1. shrunken equals fresh ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2"])
@pytest.mark.parametrize("dim", [20, 136])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_shrunken_handle_equals_fresh_handle(native_lib, oracle, tmp_path, metric, dim, mode):
    from hnsw_clj_amd import engine

    rows, Q = _data(dim)
    with engine.Index(rows, metric, 0) as shrunk:
        shrunk.set_rejection_test(mode)
        shrunk.lsh_build(8, 6, 64, 42)                      # buckets of about 39 rows
        planes, codes0, off0, ids0 = shrunk.lsh_get()
        total = np.arange(N, dtype=np.int64)                # old id of every present row
        model = (codes0, off0, ids0)
        for pick in _removals(7):
            gone = np.asarray(pick(shrunk.n))
            model = R.compact(*model, gone)
            total = total[_remove(shrunk, gone)]
        n1 = len(total)
        assert 0 < n1 < N // 2 and shrunk.n == n1
        with _fresh(engine, rows[total], metric, planes, mode) as fresh:
            _, codes, off, ids = _assert_same_tables(shrunk, fresh)
            for got, want, what in zip((codes, off, ids), model, ("codes", "off", "ids")):
                np.testing.assert_array_equal(got, want, err_msg=what + " against the removal model")
            np.testing.assert_array_equal(codes, codes0[total], err_msg="a kept row's code changed")
            np.testing.assert_array_equal(shrunk.lsh_hash(rows[total]), codes, err_msg="a row's code depends on how the handle came")
            for cfg in CONFIGS:
                for nq in (1, NQ):
                    _same(shrunk.lsh_search(Q[:nq], K, *cfg), fresh.lsh_search(Q[:nq], K, *cfg), "lsh_search %s nq %d" % (cfg, nq))
            _same(shrunk.exact_knn(Q[:5], K), fresh.exact_knn(Q[:5], K), "exact_knn")
            np.testing.assert_array_equal(_bits(shrunk.norms()), _bits(fresh.norms()), err_msg="norms")
            pick = np.array([0, n1 - 1, n1 // 2, 31, 32], np.int32)
            np.testing.assert_array_equal(_bits(shrunk.batch_distances(Q[0], ids=pick)), _bits(fresh.batch_distances(Q[0], ids=pick)),
                                          err_msg="batch_distances")
            fa, fb = tmp_path / "shrunk.idx", tmp_path / "fresh.idx"
            shrunk.save(fa)
            fresh.save(fb)
            assert fa.read_bytes() == fb.read_bytes(), "the saved files differ"
        if metric == "cosine" and dim == 20 and mode == 2:  # ... and to the model, not only to its twin
            D = _dense(oracle, rows[total], Q, metric)
            qcodes = shrunk.lsh_hash(Q)
            for cfg in CONFIGS:
                gi, gd = shrunk.lsh_search(Q, K, *cfg)
                ei, ed = M.search_batch(D, qcodes, off, ids, 6, K, *cfg)
                assert_exact(gi, gd, ei, ed, "shrunken handle against the model %s" % (cfg,))


# ---- 2. split independence ------------------------------------------------------------------------------------------------
def test_tables_do_not_depend_on_how_the_removal_was_split(native_lib):
    from hnsw_clj_amd import engine

    rows, _ = _data(20)
    gone = np.random.default_rng(2).choice(N, 400, replace=False)
    with engine.Index(rows, "cosine", 0) as one, engine.Index(rows, "cosine", 0) as many:
        one.lsh_build(8, 6, 64, 42)
        many.lsh_build(8, 6, 64, 42)
        kept = _remove(one, gone)
        now = np.arange(N, dtype=np.int64)                  # old id of every row present in `many`
        for at in range(0, len(gone), 7):
            new_id = np.full(N, -1, np.int64)
            new_id[now] = np.arange(len(now))
            now = now[_remove(many, new_id[gone[at:at + 7]])]
        np.testing.assert_array_equal(now, kept)
        a, b = one.lsh_get(), many.lsh_get()
        assert _tables_equal(a, b)
        assert (a[2][:, -1] == N - 400).all() and (np.sort(a[3], axis=1) == np.arange(N - 400)).all()


# ---- 3. removal is the permanent form of the filter -----------------------------------------------------------------------
def test_removal_is_the_permanent_form_of_the_filter(native_lib):
    from hnsw_clj_amd import engine

    rows, Q = _data(20)
    gone = np.random.default_rng(3).choice(N, 900, replace=False)
    keep = np.ones(N, np.bool_)
    keep[gone] = False
    new_id = np.append(R.rank(N, gone), -1).astype(np.int32)    # (-1 -> -1: the padding of a short result)
    with engine.Index(rows, "l2", 0) as ix:
        ix.lsh_build(8, 6, 64, 42)
        before = [ix.lsh_search_filtered(Q, K, engine.pack_mask(keep, N), *cfg) for cfg in CONFIGS]
        _remove(ix, gone)
        for cfg, (fi, fd) in zip(CONFIGS, before):
            assert ((fi < 0) | keep[fi]).all()
            gi, gd = ix.lsh_search(Q, K, *cfg)
            np.testing.assert_array_equal(new_id[fi], gi, err_msg="ids %s" % (cfg,))
            np.testing.assert_array_equal(_bits(fd), _bits(gd), err_msg="distance bits %s" % (cfg,))


# ---- 4. buckets that empty, tables at the limits, twins -------------------------------------------------------------------
def test_a_bucket_that_empties(native_lib):
    from hnsw_clj_amd import engine

    rows, _ = _data(20)
    with engine.Index(rows, "dot", 0) as ix:
        ix.lsh_build(8, 6, 64, 42)
        planes, codes, off, ids = ix.lsh_get()
        b = int(np.argmax(np.diff(off[0])))                 # the fullest bucket of table 0
        gone = ids[0, off[0, b]:off[0, b + 1]].copy()
        assert len(gone) > 32
        kept = _remove(ix, gone)
        with _fresh(engine, rows[kept], "dot", planes) as fresh:
            _, c1, o1, i1 = _assert_same_tables(ix, fresh)
        assert o1[0, b] == o1[0, b + 1] and not (c1[:, 0] == b).any()
        new_id = R.rank(N, gone)
        for t in range(1, 8):                               # the other tables' buckets list exactly their kept members
            for bb in np.unique(codes[gone, t])[:5]:
                old = ids[t, off[t, bb]:off[t, bb + 1]]
                assert i1[t, o1[t, bb]:o1[t, bb + 1]].tolist() == [new_id[r] for r in old if new_id[r] >= 0]


@pytest.mark.parametrize("tables,bits", [(1, 1), (1, 16), (16, 1), (16, 12), (16, 16)])
def test_table_shapes(native_lib, tables, bits):
    """bits 1: two buckets hold everything.  bits 12: the counts still in LDS, most buckets empty or emptied.  bits 16: the
    65,537-entry scan, the counts beyond LDS, and (16, 16) both limits at once."""
    from hnsw_clj_amd import engine

    n = 600
    rng = np.random.default_rng(100 * tables + bits)
    rows = rng.standard_normal((n, 20)).astype(np.float32)
    planes = rng.standard_normal((tables, bits, 20)).astype(np.float32)
    with engine.Index(rows, "dot", 0) as ix:
        ix.set_lsh(planes)
        kept = _remove(ix, rng.choice(n, 65, replace=False))
        kept = kept[_remove(ix, rng.choice(len(kept), 200, replace=True))]
        with _fresh(engine, rows[kept], "dot", planes) as fresh:
            _assert_same_tables(ix, fresh, "%d x %d" % (tables, bits))


@pytest.mark.parametrize("m", [1, 64, 960])
def test_copies_of_one_vector(native_lib, m):
    """1,025 rows share a bucket in every table: the kept ones close up over word, wave and chunk boundaries."""
    from hnsw_clj_amd import engine

    rng = np.random.default_rng(44)
    base, v = rng.standard_normal((300, 20)).astype(np.float32), rng.standard_normal(20).astype(np.float32)
    rows = np.concatenate([base[:150], np.repeat(v[None, :], 1025, axis=0), base[150:]])
    twins = np.arange(150, 150 + 1025)
    gone = rng.choice(twins, m, replace=False)
    with engine.Index(rows, "l2", 0) as ix:
        ix.lsh_build(8, 6, 64, 42)
        planes = ix.lsh_get()[0]
        kept = _remove(ix, gone)
        with _fresh(engine, rows[kept], "l2", planes) as fresh:
            _assert_same_tables(ix, fresh, "m %d" % m)
            got = ix.lsh_search(v, K, 8, 0, 30, 10)
            _same(got, fresh.lsh_search(v, K, 8, 0, 30, 10), "twins, m %d" % m)
            assert got[0][0].tolist() == list(range(150, 150 + K))   # the kept twins, renumbered, in id order


# ---- 5. to nothing and back -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 300])
def test_to_nothing_and_back(native_lib, n):
    from hnsw_clj_amd import engine

    rng = np.random.default_rng(16)
    rows = rng.standard_normal((n, 16)).astype(np.float32)
    with engine.Index(rows, "cosine", 0) as ix:
        ix.lsh_build()
        planes = ix.lsh_get()[0]
        kept = _remove(ix, rng.permutation(n))
        assert len(kept) == 0 and ix.n == 0 and _native_n(ix) == 0 and ix.lsh_sizes() == (8, 12)
        p, c, o, i = ix.lsh_get()
        np.testing.assert_array_equal(_bits(p), _bits(planes))
        assert c.shape == (0, 8) and i.shape == (8, 0) and o.shape == (8, 4097) and not o.any()
        gi, gd = ix.lsh_search(rows[:3], K)
        assert (gi == -1).all() and np.isposinf(gd).all()
        got = ix.lsh_add(rows)
        np.testing.assert_array_equal(got, np.arange(n, dtype=np.int32))
        with _fresh(engine, rows, "cosine", planes) as fresh:
            _assert_same_tables(ix, fresh, "grown again from nothing")
            _same(ix.lsh_search(rows[:3], K), fresh.lsh_search(rows[:3], K), "grown again from nothing")
            np.testing.assert_array_equal(_bits(ix.norms()), _bits(fresh.norms()))


# ---- 6. add and remove interleaved ----------------------------------------------------------------------------------------
def test_add_and_remove_interleaved(native_lib):
    from hnsw_clj_amd import engine

    rows, Q = _data(136)
    n0 = 1000
    rng = np.random.default_rng(6)
    with engine.Index(rows[:n0], "cosine", 0) as ix:
        ix.set_rejection_test(2)
        ix.lsh_build(8, 6, 64, 42)
        planes = ix.lsh_get()[0]
        ix.lsh_add(rows[n0:n0 + 257])
        gone = np.concatenate([rng.choice(n0, 100, replace=False), n0 + rng.choice(257, 50, replace=False)])
        now = np.arange(n0 + 257)[_remove(ix, gone)]
        ix.lsh_add(rows[n0 + 257:n0 + 320])
        now = np.concatenate([now, np.arange(n0 + 257, n0 + 320)])
        assert ix.n == len(now) == n0 + 320 - 150
        with _fresh(engine, rows[now], "cosine", planes, 2) as fresh:
            _assert_same_tables(ix, fresh)
            for cfg in CONFIGS:
                _same(ix.lsh_search(Q, K, *cfg), fresh.lsh_search(Q, K, *cfg), "lsh_search %s" % (cfg,))
            np.testing.assert_array_equal(_bits(ix.norms()), _bits(fresh.norms()))


# ---- 7. refusals leave the handle alone -----------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone(native_lib):
    from hnsw_clj_amd import engine

    L = native_lib.lib()
    rows, Q = _data(20)
    base = rows[:500]

    def ids(*v):
        a = np.array(v, np.int32)
        return a, a.ctypes.data_as(ctypes.c_void_p)

    one, ptr = ids(3)

    def state(ix):
        return ix.lsh_get(), ix.lsh_search(Q[:5], K)

    def unchanged(ix, before, what):
        assert ix.n == 500 and _native_n(ix) == 500
        tables, answer = state(ix)
        assert _tables_equal(tables, before[0]), what
        _same(answer, before[1], what)

    def refused(ix, p, m, code, word=None, before=None):
        out = ctypes.c_int64(-7)
        assert L.hnswgpu_lsh_remove(ix._h, p, m, ctypes.byref(out)) == code
        assert out.value == (500 if code == 0 else -7)        # a refusal does not write n_after
        if word:
            assert word in L.hnswgpu_last_error().lower()
        if before is not None:                                # every refusal leaves n, the tables and a search's bits alone
            unchanged(ix, before, "after a refusal with code %d (%s)" % (code, word))

    with engine.Index(base, "cosine", 0) as bare:
        refused(bare, ptr, 1, -3, b"no lsh tables")
        refused(bare, None, 0, 0)                             # nothing to remove: nothing is looked at
        assert bare.n == 500 and bare.lsh_sizes() == (0, 0)
    with engine.Index(base, "cosine", 0) as ix:
        ix.lsh_build(8, 6, 64, 42)
        before = state(ix)
        refused(ix, None, 1, -1, b"rows is null", before)
        refused(ix, ptr, -1, -1, None, before)
        for bad in (-1, 500):
            arr, p = ids(3, 4, bad, 5)
            refused(ix, p, 4, -1, b"not a row", before)
        refused(ix, ptr, 0, 0, None, before)                  # nothing to remove: nothing happens
        refused(ix, None, 0, 0, None, before)
        assert L.hnswgpu_lsh_remove(ix._h, None, 0, None) == 0    # n_after may be null
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
    with engine.Index(base, "cosine", 0) as ix:               # ... and n_after null on a call that removes
        ix.set_lsh(before[0][0])
        assert L.hnswgpu_lsh_remove(ix._h, ptr, 1, None) == 0
        assert _native_n(ix) == 499


# ---- 8. searches beside removals ------------------------------------------------------------------------------------------
def test_searches_beside_removals_see_one_of_the_index_states(native_lib):
    from hnsw_clj_amd import engine

    n0, step = 700, 50
    rows, Q = _data(32, n0)
    q = np.ascontiguousarray(Q[:8])
    rng = np.random.default_rng(8)
    removals, present = [], [np.arange(n0)]                 # each removal in the numbering current at its turn
    for _ in range(3):
        removals.append(rng.choice(len(present[-1]), step, replace=False))
        present.append(present[-1][R.kept(len(present[-1]), removals[-1])])
    with engine.Index(rows, "l2", 0) as ix:
        ix.lsh_build(8, 6, 64, 42)
        planes = ix.lsh_get()[0]
        states = []                                          # per index state: (ids, distance bits), from fresh handles
        for now in present:
            with _fresh(engine, rows[now], "l2", planes) as fresh:
                i, d = fresh.lsh_search(q, K)
                states.append((i, _bits(d)))
        stop, errors, seen = threading.Event(), [], [set(), set()]

        def matches(i, d):
            return [s for s in range(4) if np.array_equal(i, states[s][0]) and np.array_equal(_bits(d), states[s][1])]

        def searcher(t):
            try:
                for _ in range(20000):                       # bounded: the remover sets `stop` long before
                    if stop.is_set():
                        break
                    hit = matches(*ix.lsh_search(q, K))
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
                    ix.lsh_remove(gone)
                    assert s + 1 in matches(*ix.lsh_search(q, K)), "the shrunken index is what every later search sees"
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
            finally:
                stop.set()

        threads = [threading.Thread(target=searcher, args=(t,), daemon=True) for t in range(2)]
        threads.append(threading.Thread(target=remover, daemon=True))
        for th in threads:
            th.start()
        for th in threads:
            th.join(STEP_SECONDS)
            assert not th.is_alive(), "a thread did not finish within its time limit"
        assert not errors, errors[0]
        assert ix.n == len(present[-1])
        assert 3 in matches(*ix.lsh_search(q, K))


# ---- 9. the Python mirror -------------------------------------------------------------------------------------------------
def test_python_mirror_remove_vectors(native_lib):
    from hnsw_clj_amd import hybrid_lsh as H

    rows, _ = _data(20)
    n0 = 600
    index = H.build_index([("v-%d" % i, rows[i]) for i in range(n0)], show_progress=False)
    try:
        assert H.search_knn(index, rows[33], 5)[0]["id"] == "v-33"
        assert H.remove_vectors(index, ["v-33", "v-0", "v-599"]) is index
        assert H.index_info(index)["vectors"] == n0 - 3 and len(index.ids) == n0 - 3
        assert all(r["id"] not in ("v-33", "v-0", "v-599") for r in H.search_knn(index, rows[33], 10))
        res = H.search_knn(index, rows[34], 5)
        assert res[0]["id"] == "v-34" and abs(res[0]["distance"]) <= 1e-5
        with pytest.raises(KeyError):
            H.remove_vectors(index, ["v-1", "v-33"])
        assert len(index.ids) == n0 - 3 and index.index.n == n0 - 3
        H.add_vectors(index, [("w-0", rows[700])])
        assert H.search_knn(index, rows[700], 5)[0]["id"] == "w-0"
    finally:
        index.close()
