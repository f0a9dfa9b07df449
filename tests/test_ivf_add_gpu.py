"""hnswgpu_ivf_add on the device: a handle that grew is indistinguishable from a fresh handle over all the rows that was given the
same centroids and the merged lists (ivf_add_model.merged_lists) through set_ivf -- get_ivf exactly, every search's ids and
distance BITS, norms, the saved file's bytes.

Expected membership of the new rows: kmeans_assign on a fresh handle over all rows with HNSWGPU_TUNE_TILE = 0 (the GEMV order,
the one order hnswgpu_ivf_add assigns in); as a guard that does not depend on the device, the f64 distance of every new row to
the centroid it was given is within 1e-5 relative of its f64 minimum."""
import ctypes
import threading

import numpy as np
import pytest

from ivf_add_model import f64_distances, merged_lists

pytestmark = pytest.mark.gpu

N0, M_ADD, NLIST, NQ = 3000, 1000, 16, 64
STEP_SECONDS = 60          # the time limit of one step of the threaded test
_DATA = {}


def _data(O, dim, n=N0 + M_ADD):
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


def _device_assign(engine, tune, rows, metric, cen):
    """The nearest list of every row in the GEMV order: kmeans_assign on a fresh handle with the tile path off for that call."""
    with engine.Index(rows, metric, 0) as ix:
        tune.set("TILE", 0)
        try:
            a, _ = ix.kmeans_assign(cen)
        finally:
            tune.restore()
    return a


def _check_f64_guard(metric, rows, cen, assign):
    d = f64_distances(metric, rows, cen)
    got, best = d[np.arange(len(rows)), assign], d.min(axis=1)
    assert (np.abs(got - best) <= 1e-5 * np.abs(best)).all(), "a new row was not given (one of) its nearest centroids"


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


def _assert_same_answers(engine, grown, fresh, Q, n0, seed=5):
    """Everything a search reads, through every entry point that reads it."""
    n1 = grown.n
    assert fresh.n == n1
    for nq in (1, 5, 64):
        for nprobe in (1, 4, 16):
            _same(grown.ivf_search(Q[:nq], 10, nprobe), fresh.ivf_search(Q[:nq], 10, nprobe), "ivf_search nq %d nprobe %d" % (nq, nprobe))
    nl = grown.nlist
    probes = np.array([[0, -1, nl - 1], [nl - 1, nl // 2, -1], [-1, -1, 1 % nl], [nl // 3, (nl // 3 + 1) % nl, 0],
                       [-1, -1, -1]], np.int32)
    _same(grown.ivf_search_lists(Q[:5], 10, probes), fresh.ivf_search_lists(Q[:5], 10, probes), "ivf_search_lists")
    rng = np.random.default_rng(seed)
    for name, bits in (("half", rng.random(n1) < 0.5), ("ones", np.ones(n1, np.bool_))):
        mask = engine.pack_mask(bits, n1)
        _same(grown.ivf_search_filtered(Q[:5], 10, 4, mask), fresh.ivf_search_filtered(Q[:5], 10, 4, mask), "ivf_search_filtered " + name)
    _same(grown.exact_knn(Q[:5], 10), fresh.exact_knn(Q[:5], 10), "exact_knn")
    np.testing.assert_array_equal(_bits(grown.norms()), _bits(fresh.norms()), err_msg="norms")
    at = np.array([n0, n1 - 1, (n0 + n1) // 2, 0], np.int32)
    np.testing.assert_array_equal(_bits(grown.batch_distances(Q[0], ids=at)), _bits(fresh.batch_distances(Q[0], ids=at)),
                                  err_msg="batch_distances")


# ---- 1. grown equals fresh ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2"])
@pytest.mark.parametrize("dim", [64, 136])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_grown_handle_equals_fresh_handle(native_lib, oracle, tune, tmp_path, metric, dim, mode):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, dim)
    with engine.Index(rows[:N0], metric, 0) as grown:
        grown.set_rejection_test(mode)
        grown.ivf_build(NLIST, 3, 42)
        cen, off0, ids0 = grown.get_ivf()
        assign = _device_assign(engine, tune, rows, metric, cen)[N0:]
        _check_f64_guard(metric, rows[N0:], cen, assign)
        off, ids = merged_lists(off0, ids0, assign)
        at = N0
        for m in (1, 63, 64, 65, 257, M_ADD - (1 + 63 + 64 + 65 + 257)):
            got = grown.ivf_add(rows[at:at + m])
            np.testing.assert_array_equal(got, np.arange(at, at + m, dtype=np.int32))
            at += m
        assert grown.n == N0 + M_ADD
        _assert_same_ivf(grown, cen, off, ids)
        with _fresh(engine, rows, metric, mode, cen, off, ids, grown.ivf_stream_state()) as fresh:
            _assert_same_answers(engine, grown, fresh, Q, N0)
            fa, fb = tmp_path / "grown.idx", tmp_path / "fresh.idx"
            grown.save(fa)
            fresh.save(fb)
            assert fa.read_bytes() == fb.read_bytes(), "the saved files differ"
            with engine.Index.load(fa, 0) as back:
                assert back.n == N0 + M_ADD
                _assert_same_ivf(back, cen, off, ids, "loaded")
                _same(back.ivf_search(Q, 10, 4), fresh.ivf_search(Q, 10, 4), "loaded file")


# ---- 2. split independence ------------------------------------------------------------------------------------------------
def test_lists_do_not_depend_on_how_the_rows_were_split(native_lib, oracle):
    from hnsw_clj_amd import engine

    rows, _ = _data(oracle, 64)
    with engine.Index(rows[:N0], "cosine", 0) as one, engine.Index(rows[:N0], "cosine", 0) as many:
        one.ivf_build(NLIST, 3, 42)
        cen, off0, ids0 = one.get_ivf()
        many.set_ivf(cen, off0, ids0)
        one.ivf_add(rows[N0:])
        for at in range(N0, N0 + M_ADD, 7):
            many.ivf_add(rows[at:min(at + 7, N0 + M_ADD)])
        c1, o1, i1 = one.get_ivf()
        _assert_same_ivf(many, c1, o1, i1)
        assert o1[-1] == N0 + M_ADD and sorted(i1.tolist()) == list(range(N0 + M_ADD))


# ---- 3. placement edges ---------------------------------------------------------------------------------------------------
def _edge_base(seed=3, n0=200, dim=64):
    rng = np.random.default_rng(seed)
    cen = (4.0 * rng.standard_normal((4, dim))).astype(np.float32)
    cen[2] = cen[1]                                        # two identical centroids: the lower index wins every tie
    base = (cen[rng.integers(0, 2, n0)] + 0.1 * rng.standard_normal((n0, dim))).astype(np.float32)   # lists 0 and 1; 2 and 3 empty
    a0 = f64_distances("l2", base, cen).argmin(axis=1)     # (argmin: the first minimum)
    assert set(a0.tolist()) == {0, 1}
    order = np.argsort(a0, kind="stable").astype(np.int32)
    off0 = np.zeros(5, np.int64)
    off0[1:] = np.cumsum(np.bincount(a0, minlength=4))
    return cen, base, off0, order


def _found_at_zero(ix, rows, first, dup_of=None):
    ids, d = ix.ivf_search(rows, 1, ix.nlist)
    assert (np.abs(d[:, 0]) <= 1e-5).all(), "an added row is not found at distance ~ 0"
    if dup_of is None:
        np.testing.assert_array_equal(ids[:, 0], np.arange(first, first + len(rows), dtype=np.int32))
    else:                                                   # copies of one vector: the first of them in the list wins
        assert (ids[:, 0] >= dup_of).all()


@pytest.mark.parametrize("m", [1, 64, 65, 1025])
def test_all_rows_into_one_list_below_an_identical_centroid(native_lib, m):
    from hnsw_clj_amd import engine

    cen, base, off0, ids0 = _edge_base()
    new = np.repeat(cen[1][None, :], m, axis=0)            # copies of one centroid: distance 0 to lists 1 AND 2
    with engine.Index(base, "l2", 0) as ix:
        ix.set_ivf(cen, off0, ids0)
        ix.ivf_add(new)
        off, ids = merged_lists(off0, ids0, np.full(m, 1))
        _assert_same_ivf(ix, cen, off, ids)
        _found_at_zero(ix, new[:min(m, 70)], len(base), dup_of=len(base))
        with _fresh(engine, np.concatenate([base, new]), "l2", None, cen, off, ids) as fresh:
            _same(ix.ivf_search(new[:3], 10, 4), fresh.ivf_search(new[:3], 10, 4), "one list, m %d" % m)


def test_an_empty_list_receives_its_first_rows(native_lib):
    from hnsw_clj_amd import engine

    cen, base, off0, ids0 = _edge_base()
    rng = np.random.default_rng(11)
    a = np.array([3, 0] * 32 + [3], np.int64)               # 65 rows, alternating between the empty list 3 and list 0
    new = (cen[a] + 0.1 * rng.standard_normal((len(a), cen.shape[1]))).astype(np.float32)
    assert (f64_distances("l2", new, cen).argmin(axis=1) == a).all()
    with engine.Index(base, "l2", 0) as ix:
        ix.set_ivf(cen, off0, ids0)
        ix.ivf_add(new)
        off, ids = merged_lists(off0, ids0, a)
        assert off[4] - off[3] == 33 and off[3] == off[2]   # list 3 got its first rows; list 2 still has none
        _assert_same_ivf(ix, cen, off, ids)
        _found_at_zero(ix, new, len(base))
        with _fresh(engine, np.concatenate([base, new]), "l2", None, cen, off, ids) as fresh:
            _assert_same_answers(engine, ix, fresh, new, len(base))


def test_one_list(native_lib):
    from hnsw_clj_amd import engine

    rng = np.random.default_rng(2)
    base = rng.standard_normal((100, 64)).astype(np.float32)
    new = rng.standard_normal((300, 64)).astype(np.float32)
    cen = base.mean(axis=0, keepdims=True).astype(np.float32)
    ids0 = np.arange(99, -1, -1, dtype=np.int32)
    with engine.Index(base, "cosine", 0) as ix:
        ix.set_ivf(cen, [0, 100], ids0)
        ix.ivf_add(new[:1])
        ix.ivf_add(new[1:])
        off, ids = merged_lists([0, 100], ids0, np.zeros(300, np.int64))
        _assert_same_ivf(ix, cen, off, ids)
        _found_at_zero(ix, new, 100)
        with _fresh(engine, np.concatenate([base, new]), "cosine", None, cen, off, ids) as fresh:
            _same(ix.ivf_search(new[:5], 10, 1), fresh.ivf_search(new[:5], 10, 1), "one list")


# ---- 4. a handle whose lists are its base rows in place --------------------------------------------------------------------
def test_alias_handle_scatter_and_last_list(native_lib, oracle, tune):
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
    for new, stays_identity in ((rows[N0:], False), (tail, True)):
        everything = np.concatenate([base, new])
        assign = _device_assign(engine, tune, everything, "cosine", cen)[N0:]
        _check_f64_guard("cosine", new, cen, assign)
        off, ids = merged_lists(off0, ident, assign)
        assert (ids == np.arange(len(ids))).all() == stays_identity
        if stays_identity:
            assert (assign == last).all()
        with engine.Index(base, "cosine", 0) as ix:
            ix.set_ivf(cen, off0, ident)
            ix.ivf_add(new[:17])
            ix.ivf_add(new[17:])
            _assert_same_ivf(ix, cen, off, ids)
            with _fresh(engine, everything, "cosine", None, cen, off, ids) as fresh:
                _assert_same_answers(engine, ix, fresh, Q, N0)


# ---- 5. refusals leave the handle alone -----------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone(native_lib, oracle):
    from hnsw_clj_amd import engine

    L = native_lib.lib()
    rows, Q = _data(oracle, 64)
    base, one = rows[:500], np.ascontiguousarray(rows[N0:N0 + 1])
    ptr = one.ctypes.data_as(ctypes.c_void_p)

    def refused(ix, p, m, code, word=None):
        assert L.hnswgpu_ivf_add(ix._h, p, m) == code
        if word:
            assert word in L.hnswgpu_last_error().lower()

    with engine.Index(base, "cosine", 0) as bare:
        refused(bare, ptr, 1, -3, b"no ivf lists")
        assert bare.nlist == 0 and bare.n == 500
    with engine.Index(base, "cosine", 0) as ix:
        ix.ivf_build(8, 2, 42)
        cen, off, ids = ix.get_ivf()
        before = ix.ivf_search(Q[:5], 10, 4)
        refused(ix, None, 1, -1, b"rows is null")
        refused(ix, ptr, -1, -1)
        refused(ix, ptr, 2 ** 31, -5, b"2^31")               # refused before the one-row buffer is read
        assert L.hnswgpu_ivf_add(ix._h, ptr, 0) == 0          # nothing to add: nothing happens
        assert L.hnswgpu_ivf_add(ix._h, None, 0) == 0
        ix.hnsw_build(8, 40, 42)
        refused(ix, ptr, 1, -3, b"graph")
        with pytest.raises(native_lib.HnswGpuError, match="IVF"):
            ix.hnsw_add(one)
        assert ix.n == 500
        _assert_same_ivf(ix, cen, off, ids)
        _same(ix.ivf_search(Q[:5], 10, 4), before, "after the refusals")
    with engine.Index(base, "cosine", 0) as shard:
        shard.set_ivf_shard(cen, off, ids, np.diff(off) + 3)
        before = shard.ivf_search(Q[:5], 10, 4)
        refused(shard, ptr, 1, -3, b"shard")
        _assert_same_ivf(shard, cen, off, ids)
        _same(shard.ivf_search(Q[:5], 10, 4), before, "shard after the refusal")


# ---- 6. the first-search verdict of a mode-1 handle is kept ---------------------------------------------------------------
def test_mode_1_verdict_is_kept(native_lib, oracle, tune):
    from hnsw_clj_amd import engine

    n0 = 5000
    rows, Q = _data(oracle, 128, n0 + M_ADD)
    with engine.Index(rows[:n0], "cosine", 0) as ix:
        ix.set_rejection_test(1)
        ix.ivf_build(NLIST, 3, 42)
        cen, off0, ids0 = ix.get_ivf()
        assign = _device_assign(engine, tune, rows, "cosine", cen)[n0:]
        _check_f64_guard("cosine", rows[n0:], cen, assign)
        verdict = ix.ivf_stream_state()
        ix.ivf_add(rows[n0:n0 + 500])
        assert ix.ivf_stream_state() == verdict
        off, ids = merged_lists(off0, ids0, assign[:500])
        _assert_same_ivf(ix, cen, off, ids)
        with _fresh(engine, rows[:n0 + 500], "cosine", 1, cen, off, ids, verdict) as fresh:
            _assert_same_answers(engine, ix, fresh, Q, n0)
        # ... kept, not measured again: an installed verdict that the handle's own measurement would not give survives too
        ix.ivf_set_stream_state(1 - verdict)
        ix.ivf_add(rows[n0 + 500:])
        assert ix.ivf_stream_state() == 1 - verdict
        off, ids = merged_lists(off0, ids0, assign)
        with _fresh(engine, rows, "cosine", 1, cen, off, ids, 1 - verdict) as fresh:
            _assert_same_answers(engine, ix, fresh, Q, n0)


# ---- 7. searches beside adds ----------------------------------------------------------------------------------------------
def test_searches_beside_adds_see_one_of_the_index_states(native_lib, oracle, tune):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, 64)
    cuts = [N0, N0 + 300, N0 + 650, N0 + M_ADD]
    with engine.Index(rows[:N0], "l2", 0) as ix:
        ix.ivf_build(NLIST, 3, 42)
        cen, off0, ids0 = ix.get_ivf()
        assign = _device_assign(engine, tune, rows, "l2", cen)[N0:]
        qs = [np.ascontiguousarray(Q[3 * t:3 * t + 3]) for t in range(4)]
        states = []                                         # per index state, per thread: (ids, distance bits)
        for n in cuts:
            off, ids = merged_lists(off0, ids0, assign[:n - N0])
            with _fresh(engine, rows[:n], "l2", None, cen, off, ids) as fresh:
                states.append([(i, _bits(d)) for i, d in (fresh.ivf_search(q, 10, 4) for q in qs)])
        stop, errors, seen = threading.Event(), [], [set() for _ in range(4)]

        def searcher(t):
            try:
                while not stop.is_set():
                    i, d = ix.ivf_search(qs[t], 10, 4)
                    hit = [s for s in range(4) if np.array_equal(i, states[s][t][0]) and np.array_equal(_bits(d), states[s][t][1])]
                    if not hit:
                        raise AssertionError("thread %d: an answer that belongs to none of the four index states" % t)
                    seen[t].update(hit)
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
                stop.set()

        def adder():
            try:
                for a, b in zip(cuts[:-1], cuts[1:]):
                    if stop.is_set():
                        return
                    ix.ivf_add(rows[a:b])
                    for t in range(4):                      # the grown index is what every later search sees
                        i, d = ix.ivf_search(qs[t], 10, 4)
                        s = cuts.index(b)
                        assert np.array_equal(i, states[s][t][0]) and np.array_equal(_bits(d), states[s][t][1])
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
            finally:
                stop.set()

        threads = [threading.Thread(target=searcher, args=(t,), daemon=True) for t in range(4)]
        threads.append(threading.Thread(target=adder, daemon=True))
        for th in threads:
            th.start()
        for th in threads:
            th.join(STEP_SECONDS)
            assert not th.is_alive(), "a thread did not finish within its time limit"
        assert not errors, errors[0]
        assert ix.n == N0 + M_ADD and all(seen)


# ---- 8. the Python mirror -------------------------------------------------------------------------------------------------
def test_python_mirror_add_vectors(native_lib, oracle):
    from hnsw_clj_amd import ivf_flat

    rows, _ = _data(oracle, 64)
    n0, m = 600, 70
    data = [("old-%d" % i, rows[i]) for i in range(n0)]
    more = [("new-%d" % i, rows[N0 + i]) for i in range(m)]
    index = ivf_flat.build_index(data, num_partitions=8, max_iterations=2)
    try:
        assert ivf_flat.add_vectors(index, more) is index
        info = ivf_flat.index_info(index)
        assert info["vectors"] == n0 + m and len(index.ids) == n0 + m
        for i in (0, 33, m - 1):
            res = ivf_flat.search_knn(index, rows[N0 + i], 5, mode="precise")
            assert res[0]["id"] == "new-%d" % i and abs(res[0]["distance"]) <= 1e-5
        res = ivf_flat.search_knn_filtered(index, rows[5], 5, lambda i: i.startswith("new-"), mode="precise")
        assert len(res) == 5 and all(r["id"].startswith("new-") for r in res)
        assert ivf_flat.add_vectors(index, []) is index and ivf_flat.index_info(index)["vectors"] == n0 + m
    finally:
        index.close()
