"""hnswgpu_ivf_update on the device: a handle whose rows took new values is indistinguishable, bit for bit, from a fresh handle over
the base with the new values that was given the same centroids and the model's lists (ivf_update_model.updated_lists) through
set_ivf -- get_ivf exactly, every search's ids and distance BITS, norms, the saved file's bytes.  No tolerance anywhere.

Expected list of every new value: kmeans_assign on a fresh handle with HNSWGPU_TUNE_TILE = 0 (the GEMV order, the one order
hnswgpu_ivf_update assigns in); as a guard that does not depend on the device, the f64 distance of every new value to the centroid
it was given is within 1e-5 relative of its f64 minimum.  New values are spare rows of the same generator, paired with the rows
they replace so that about half of a batch stays in its list and half moves; every batch of at least 4 rows is asserted to hold at
least a quarter of each (a batch of one row cannot hold both: there the sum of all batches is what is asserted)."""
import ctypes
import threading

import numpy as np
import pytest

import ivf_remove_model as R
import ivf_update_model as U
from ivf_add_model import f64_distances, merged_lists

pytestmark = pytest.mark.gpu

N0, SPARE, NLIST, NQ = 3001, 1400, 16, 64   # 3001 rows: 12 chunks of 256 list positions and 94 mask words, the last of each partial
STEP_SECONDS = 60                           # the time limit of one step of the threaded test
_DATA = {}


def _data(O, dim, n=N0 + SPARE):
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


def _check_f64_guard(metric, rows, cen, assign):
    d = f64_distances(metric, rows, cen)
    got, best = d[np.arange(len(rows)), assign], d.min(axis=1)
    assert (np.abs(got - best) <= 1e-5 * np.abs(best)).all(), "a new value was not given (one of) its nearest centroids"


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


def _assert_same_answers(engine, updated, fresh, Q, seed=5):
    """Everything a search reads, through every entry point that reads it."""
    n = updated.n
    assert fresh.n == n and _native_n(updated) == n
    for nq in (1, 5, 64):
        for nprobe in (1, 4, 16):
            if nprobe > updated.nlist:
                continue
            _same(updated.ivf_search(Q[:nq], 10, nprobe), fresh.ivf_search(Q[:nq], 10, nprobe), "ivf_search nq %d nprobe %d" % (nq, nprobe))
    nl = updated.nlist
    probes = np.array([[0, -1, nl - 1], [nl - 1, nl // 2, -1], [-1, -1, 1 % nl], [nl // 3, (nl // 3 + 1) % nl, 0],
                       [-1, -1, -1]], np.int32)
    _same(updated.ivf_search_lists(Q[:5], 10, probes), fresh.ivf_search_lists(Q[:5], 10, probes), "ivf_search_lists")
    rng = np.random.default_rng(seed)
    for name, bits in (("half", rng.random(n) < 0.5), ("ones", np.ones(n, np.bool_))):
        mask = engine.pack_mask(bits, n)
        _same(updated.ivf_search_filtered(Q[:5], 10, min(4, nl), mask), fresh.ivf_search_filtered(Q[:5], 10, min(4, nl), mask),
              "ivf_search_filtered " + name)
    _same(updated.exact_knn(Q[:5], 10), fresh.exact_knn(Q[:5], 10), "exact_knn")
    np.testing.assert_array_equal(_bits(updated.norms()), _bits(fresh.norms()), err_msg="norms")
    at = np.array([n // 3, n - 1, n // 2, 0], np.int32)
    np.testing.assert_array_equal(_bits(updated.batch_distances(Q[0], ids=at)), _bits(fresh.batch_distances(Q[0], ids=at)),
                                  err_msg="batch_distances")


def _assert_same_file(updated, fresh, tmp_path, what=""):
    fa, fb = tmp_path / "updated.idx", tmp_path / "fresh.idx"
    updated.save(fa)
    fresh.save(fb)
    assert fa.read_bytes() == fb.read_bytes(), "the saved files differ " + what


def _list_of(off, ids):
    out = np.empty(len(ids), np.int64)
    out[np.asarray(ids, np.int64)] = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return out


class _Pairing:
    """Pairs spare values with the rows they replace: value j (nearest list spare_assign[j]) replaces, in turn, a row of that list
    (a stayer) or a row of another list (a mover).  Every spare value is used once."""

    def __init__(self, seed, spare_assign):
        self.rng = np.random.default_rng(seed)
        self.spare_assign = np.asarray(spare_assign, np.int64)
        self.next = 0

    def batch(self, list_of, m, first_moves=False):
        """(row ids [m], spare indices [m], moves bool [m]) against the present lists `list_of` (row -> list)."""
        taken = np.zeros(len(list_of), bool)
        rows, spares, moves = [], [], []
        while len(rows) < m:
            j, self.next = self.next, self.next + 1
            assert j < len(self.spare_assign), "out of spare values"
            want_move = (len(rows) % 2 == 0) == first_moves
            pool = np.flatnonzero(~taken & ((list_of != self.spare_assign[j]) == want_move))
            if len(pool) == 0:                               # (no row left in / outside that list: the value is skipped)
                continue
            r = int(self.rng.choice(pool))
            taken[r] = True
            rows.append(r)
            spares.append(j)
            moves.append(want_move)
        p = self.rng.permutation(m)                          # the call names its rows in no particular order
        return np.array(rows, np.int32)[p], np.array(spares, np.int64)[p], np.array(moves, bool)[p]


def _assert_mixed(moves):
    if len(moves) >= 4:
        assert 4 * moves.sum() >= len(moves) and 4 * (~moves).sum() >= len(moves), "a batch must hold both kinds of row"


# ---- 1. updated equals fresh ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2"])
@pytest.mark.parametrize("dim", [64, 136])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_updated_handle_equals_fresh_handle(native_lib, oracle, tune, tmp_path, metric, dim, mode):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, dim)
    spare = rows[N0:]
    with engine.Index(rows[:N0], metric, 0) as ix:
        ix.set_rejection_test(mode)
        ix.ivf_build(NLIST, 3, 42)
        cen, off, ids = ix.get_ivf()
        assign = _device_assign(engine, tune, spare, metric, cen)
        _check_f64_guard(metric, spare, cen, assign)
        pairing = _Pairing(41, assign)
        cur = rows[:N0].copy()
        all_moves = []
        for m in (1, 63, 64, 65, 257, 300):
            at, sp, moves = pairing.batch(_list_of(off, ids), m, first_moves=(m == 1))
            _assert_mixed(moves)
            all_moves.append(moves)
            off, ids = U.updated_lists(off, ids, at, assign[sp])
            ix.ivf_update(at, spare[sp])
            cur[at] = spare[sp]
            assert ix.n == N0 and _native_n(ix) == N0
            _assert_same_ivf(ix, cen, off, ids, "after m %d" % m)
            with _fresh(engine, cur, metric, mode, cen, off, ids, ix.ivf_stream_state()) as fresh:
                _assert_same_answers(engine, ix, fresh, Q)
                _assert_same_file(ix, fresh, tmp_path, "after m %d" % m)
        _assert_mixed(np.concatenate(all_moves))
        with engine.Index.load(tmp_path / "updated.idx", 0) as back, _fresh(engine, cur, metric, mode, cen, off, ids) as fresh:
            assert back.n == N0
            _assert_same_ivf(back, cen, off, ids, "loaded")
            _same(back.ivf_search(Q, 10, 4), fresh.ivf_search(Q, 10, 4), "loaded file")


# ---- 2. the order of `ids` within a call ----------------------------------------------------------------------------------
def test_order_of_ids_within_a_call_does_not_matter(native_lib, oracle, tune, tmp_path):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, 64)
    spare = rows[N0:]
    with engine.Index(rows[:N0], "cosine", 0) as first:
        first.ivf_build(NLIST, 3, 42)
        cen, off0, ids0 = first.get_ivf()
        assign = _device_assign(engine, tune, spare, "cosine", cen)
        at, sp, moves = _Pairing(42, assign).batch(_list_of(off0, ids0), 500)
        _assert_mixed(moves)
        asc = np.argsort(at)
        off, ids = U.updated_lists(off0, ids0, at, assign[sp])
        first.ivf_update(at[asc], spare[sp[asc]])
        _assert_same_ivf(first, cen, off, ids, "ascending")
        for name, order in (("descending", asc[::-1]), ("shuffled", np.random.default_rng(1).permutation(500))):
            with _fresh(engine, rows[:N0], "cosine", None, cen, off0, ids0) as other:
                other.ivf_update(at[order], spare[sp[order]])
                _assert_same_ivf(other, cen, off, ids, name)
                _assert_same_answers(engine, other, first, Q)
                _assert_same_file(other, first, tmp_path, name)


# ---- 3. the result depends on how an update is split over calls ------------------------------------------------------------
def test_split_over_calls_is_the_model_applied_twice(native_lib, oracle, tune):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, 64)
    spare = rows[N0:]
    with engine.Index(rows[:N0], "l2", 0) as ix:
        ix.ivf_build(NLIST, 3, 42)
        cen, off0, ids0 = ix.get_ivf()
        assign = _device_assign(engine, tune, spare, "l2", cen)
        where = _list_of(off0, ids0)
        target = int(assign[0])                              # the list the first spare values belong into
        vals = np.flatnonzero(assign == target)[:40]
        assert len(vals) == 40
        outside = np.flatnonzero(where != target)
        lo, hi = outside[:20], outside[-20:]                 # movers with low and with high row ids
        # the high ids first, the low ids in a second call: they stand BEHIND the high ones; one call would sort them in front
        once = U.updated_lists(off0, ids0, np.concatenate([hi, lo]), np.full(40, target))
        off, ids = U.updated_lists(off0, ids0, hi, np.full(20, target))
        off, ids = U.updated_lists(off, ids, lo, np.full(20, target))
        assert not np.array_equal(ids, once[1]) and np.array_equal(off, once[0])
        assert ids[off[target + 1] - 40:off[target + 1]].tolist() == hi.tolist() + lo.tolist()
        ix.ivf_update(hi, spare[vals[:20]])
        ix.ivf_update(lo, spare[vals[20:]])
        _assert_same_ivf(ix, cen, off, ids, "two calls")
        cur = rows[:N0].copy()
        cur[hi], cur[lo] = spare[vals[:20]], spare[vals[20:]]
        with _fresh(engine, cur, "l2", None, cen, off, ids) as fresh:
            _assert_same_answers(engine, ix, fresh, Q)


# ---- 4. rows updated to the values they have -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2"])
def test_update_to_the_same_values_changes_nothing(native_lib, oracle, tune, tmp_path, mode):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, 136)
    base = rows[:N0]
    with engine.Index(base, "cosine", 0) as b:
        b.ivf_build(NLIST, 3, 42)
        cen, _, _ = b.get_ivf()
    a = _device_assign(engine, tune, base, "cosine", cen)    # lists by the GEMV order: every row sits in the list an update gives it
    ids0 = np.lexsort((-np.arange(N0), a)).astype(np.int32)  # members of a list in descending row order: not the identity
    off0 = np.zeros(NLIST + 1, np.int64)
    off0[1:] = np.cumsum(np.bincount(a, minlength=NLIST))
    with _fresh(engine, base, "cosine", mode, cen, off0, ids0) as ix:
        before = tmp_path / "before.idx"
        ix.save(before)
        answer = ix.ivf_search(Q, 10, 4)
        for at in (np.array([7], np.int32), np.random.default_rng(9).permutation(N0)[:700].astype(np.int32), np.arange(N0, dtype=np.int32)):
            ix.ivf_update(at, base[at])
            _assert_same_ivf(ix, cen, off0, ids0, "m %d" % len(at))
            after = tmp_path / "after.idx"
            ix.save(after)
            assert after.read_bytes() == before.read_bytes(), "the saved file changed"
            _same(ix.ivf_search(Q, 10, 4), answer, "m %d" % len(at))


# ---- 5. edges on a crafted base -------------------------------------------------------------------------------------------
def _edge_base(seed=3, n0=200, dim=64):
    """200 x 64 over 4 centroids: lists 0 and 1 hold the rows, centroid 2 is a copy of centroid 1 (the lower index wins every tie,
    list 2 stays empty), list 3 is empty"""
    rng = np.random.default_rng(seed)
    cen = (4.0 * rng.standard_normal((4, dim))).astype(np.float32)
    cen[2] = cen[1]
    base = (cen[rng.integers(0, 2, n0)] + 0.1 * rng.standard_normal((n0, dim))).astype(np.float32)
    a0 = f64_distances("l2", base, cen).argmin(axis=1)     # (argmin: the first minimum)
    assert set(a0.tolist()) == {0, 1}
    order = np.argsort(a0, kind="stable").astype(np.int32)
    off0 = np.zeros(5, np.int64)
    off0[1:] = np.cumsum(np.bincount(a0, minlength=4))
    return rng, cen, base, off0, order, a0


def _near(rng, cen, lists):
    lists = np.asarray(lists, np.int64)
    new = (cen[lists] + 0.1 * rng.standard_normal((len(lists), cen.shape[1]))).astype(np.float32)
    assert (f64_distances("l2", new, cen).argmin(axis=1) == np.where(lists == 2, 1, lists)).all()
    return new


@pytest.mark.parametrize("case", ["list_emptied", "first_members", "doubled_centroid", "every_row"])
def test_edges_of_the_lists(native_lib, case):
    from hnsw_clj_amd import engine

    rng, cen, base, off0, ids0, a0 = _edge_base()
    n = len(base)
    if case == "list_emptied":                               # every member of list 0 leaves, in descending order of position
        at = ids0[off0[0]:off0[1]][::-1].copy()
        to = np.full(len(at), 1)
        new = _near(rng, cen, to)
    elif case == "first_members":                            # 65 rows, alternating between the empty list 3 and their own list
        at = rng.permutation(n)[:65].astype(np.int32)
        to = np.where(np.arange(65) % 2 == 0, 3, a0[at])
        new = _near(rng, cen, to)
    elif case == "doubled_centroid":                         # copies of the doubled centroid: distance 0 to lists 1 AND 2 -> list 1
        at = np.concatenate([ids0[off0[0]:off0[1]][:33], ids0[off0[1]:off0[2]][:32]]).astype(np.int32)
        to = np.full(65, 1)
        new = np.repeat(cen[2][None, :], 65, axis=0)
    else:                                                    # m == n
        at = rng.permutation(n).astype(np.int32)
        to = rng.choice([0, 1, 3], n)
        new = _near(rng, cen, to)
    off, ids = U.updated_lists(off0, ids0, at, to)
    if case == "list_emptied":
        assert off[0] == off[1] == 0 and off[2] == n
    if case == "first_members":
        assert off[4] - off[3] == 33 and off[3] == off[2]
    cur = base.copy()
    cur[at] = new
    with engine.Index(base, "l2", 0) as ix:
        ix.set_ivf(cen, off0, ids0)
        ix.ivf_update(at, new)
        _assert_same_ivf(ix, cen, off, ids, case)
        with _fresh(engine, cur, "l2", None, cen, off, ids) as fresh:
            _assert_same_answers(engine, ix, fresh, cur[:64])


def test_one_list(native_lib):
    from hnsw_clj_amd import engine

    rng = np.random.default_rng(2)
    base = rng.standard_normal((100, 64)).astype(np.float32)
    new = rng.standard_normal((37, 64)).astype(np.float32)
    cen = base.mean(axis=0, keepdims=True).astype(np.float32)
    ids0 = np.arange(99, -1, -1, dtype=np.int32)
    at = rng.permutation(100)[:37].astype(np.int32)
    cur = base.copy()
    cur[at] = new
    with engine.Index(base, "cosine", 0) as ix:
        ix.set_ivf(cen, [0, 100], ids0)
        ix.ivf_update(at, new)
        _assert_same_ivf(ix, cen, np.array([0, 100]), ids0)  # everybody stays where they are
        with _fresh(engine, cur, "cosine", None, cen, [0, 100], ids0) as fresh:
            _same(ix.ivf_search(new[:5], 10, 1), fresh.ivf_search(new[:5], 10, 1), "one list")
            _same(ix.exact_knn(new[:5], 10), fresh.exact_knn(new[:5], 10), "one list, exact")


# ---- 6. a handle whose lists are its base rows in place --------------------------------------------------------------------
@pytest.mark.parametrize("case", ["stayers", "mover", "mover_identity"])
def test_alias_handle(native_lib, oracle, tune, tmp_path, case):
    from hnsw_clj_amd import engine

    if case == "mover_identity":                             # the last row moves into the empty last list: still the identity
        rng, cen, b0, off0, order, a0 = _edge_base()
        base = np.ascontiguousarray(b0[order])
        n, metric, Q = len(base), "l2", base[:64]
        at, to = np.array([n - 1], np.int32), np.array([3])
        new = _near(rng, cen, to)
    else:
        rows, Q = _data(oracle, 64)
        n, metric = N0, "cosine"
        with engine.Index(rows[:N0], metric, 0) as b:
            b.ivf_build(NLIST, 3, 42)
            cen, off0, ids_b = b.get_ivf()
        base = np.ascontiguousarray(rows[:N0][ids_b])       # the base in list order: identity list_ids
        spare = rows[N0:]
        assign = _device_assign(engine, tune, spare, metric, cen)
        where = np.repeat(np.arange(NLIST), np.diff(off0))
        if case == "stayers":                                # 100 values, each for a row of the list it belongs into
            sp = np.arange(100)
            taken, at = set(), []
            for j in sp:
                r = next(int(r) for r in np.flatnonzero(where == assign[j]) if int(r) not in taken)
                taken.add(r)
                at.append(r)
            at = np.array(at, np.int32)
        else:                                                # 100 values, half for rows of their list and half for rows of another
            at, sp, moves = _Pairing(43, assign).batch(where, 100)
            _assert_mixed(moves)
        new, to = spare[sp], assign[sp]
    ident = np.arange(n, dtype=np.int32)
    off, ids = U.updated_lists(off0, ident, at, to)
    assert np.array_equal(ids, ident) == (case != "mover")
    if case == "mover_identity":
        assert off0[3] == off0[4] and off[4] - off[3] == 1   # the empty last list got the last row
    cur = base.copy()
    cur[at] = new
    with engine.Index(base, metric, 0) as ix:
        ix.set_ivf(cen, off0, ident)
        ix.ivf_update(at, new)
        _assert_same_ivf(ix, cen, off, ids, case)
        with _fresh(engine, cur, metric, None, cen, off, ids) as fresh:
            _assert_same_answers(engine, ix, fresh, Q)
            _assert_same_file(ix, fresh, tmp_path, case)
        ix.ivf_update(at, new)                               # ... and once more: everybody stays now, whatever the handle became
        _assert_same_ivf(ix, cen, off, ids, case + ", again")
        with _fresh(engine, cur, metric, None, cen, off, ids) as fresh:
            _assert_same_answers(engine, ix, fresh, Q)


# ---- 7. the first-search verdict of a mode-1 handle is kept ---------------------------------------------------------------
def test_mode_1_verdict_is_kept(native_lib, oracle, tune):
    from hnsw_clj_amd import engine

    n0 = 5000
    rows, Q = _data(oracle, 128, n0 + 1000)
    spare = rows[n0:]
    with engine.Index(rows[:n0], "cosine", 0) as ix:
        ix.set_rejection_test(1)
        ix.ivf_build(NLIST, 3, 42)
        cen, off, ids = ix.get_ivf()
        assign = _device_assign(engine, tune, spare, "cosine", cen)
        _check_f64_guard("cosine", spare, cen, assign)
        pairing = _Pairing(47, assign)
        cur = rows[:n0].copy()
        verdict = ix.ivf_stream_state()
        for state in (verdict, 1 - verdict):                 # ... kept, not measured again: an installed verdict survives too
            ix.ivf_set_stream_state(state)
            at, sp, moves = pairing.batch(_list_of(off, ids), 400)
            _assert_mixed(moves)
            off, ids = U.updated_lists(off, ids, at, assign[sp])
            ix.ivf_update(at, spare[sp])
            cur[at] = spare[sp]
            assert ix.ivf_stream_state() == state
            _assert_same_ivf(ix, cen, off, ids)
            with _fresh(engine, cur, "cosine", 1, cen, off, ids, state) as fresh:
                _assert_same_answers(engine, ix, fresh, Q)


# ---- 8. refusals leave the handle alone -----------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone(native_lib, oracle):
    from hnsw_clj_amd import engine

    L = native_lib.lib()
    rows, Q = _data(oracle, 64)
    base = rows[:500]
    vals = np.ascontiguousarray(rows[N0:N0 + 4])
    vptr = vals.ctypes.data_as(ctypes.c_void_p)

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

    def refused(ix, p, v, m, code, word=None, before=None):
        assert L.hnswgpu_ivf_update(ix._h, p, v, m) == code
        if word:
            assert word in L.hnswgpu_last_error().lower(), L.hnswgpu_last_error()
        if before is not None:                                # every refusal leaves n, the lists and a search's bits alone
            unchanged(ix, before, "after a refusal with code %d (%s)" % (code, word))

    with engine.Index(base, "cosine", 0) as bare:
        refused(bare, ptr, vptr, 1, -3, b"no ivf lists")
        refused(bare, None, None, 0, 0)                       # nothing to update: nothing is looked at
        refused(bare, ptr, vptr, 0, 0)
        assert bare.n == 500 and bare.nlist == 0
    with engine.Index(base, "cosine", 0) as ix:
        ix.ivf_build(8, 2, 42)
        before = state(ix)
        cen, off, lids = before[0]
        refused(ix, None, vptr, 1, -1, b"ids is null", before)
        refused(ix, ptr, None, 1, -1, b"rows is null", before)
        refused(ix, ptr, vptr, -1, -1, None, before)
        for bad in (-1, 500):
            arr, p = ids(3, 4, bad, 5)
            refused(ix, p, vptr, 4, -1, b"ids[2]", before)    # the message names the position
        arr, p = ids(9, 4, 7, 4)
        refused(ix, p, vptr, 4, -1, b"named twice", before)   # two values for one row have no winner
        assert b"ids[3]" in L.hnswgpu_last_error()
        nan = vals.copy()
        nan[2, 5] = np.nan
        arr, p = ids(9, 4, 7, 5)
        refused(ix, p, nan.ctypes.data_as(ctypes.c_void_p), 4, -1, b"no nearest centroid", before)
        refused(ix, ptr, vptr, 0, 0, None, before)            # nothing to update: nothing happens
        refused(ix, None, None, 0, 0, None, before)
        ix.lsh_build(8, 6, 64, 42)
        refused(ix, ptr, vptr, 1, -3, b"lsh tables", before)
    with engine.Index(base, "cosine", 0) as graph:
        graph.set_ivf(cen, off, lids)
        graph.hnsw_build(8, 40, 42)
        refused(graph, ptr, vptr, 1, -3, b"graph", before)
    with engine.Index(base, "cosine", 0) as forest:
        forest.hnsw_build_parts([0, 250, 500], 8, 40, 42)
        forest.set_ivf(cen, off, lids)
        refused(forest, ptr, vptr, 1, -3, b"forest", before)
    with engine.Index(base, "cosine", 0) as shard:
        shard.set_ivf_shard(cen, off, lids, np.diff(off) + 3)
        shard_before = state(shard)
        refused(shard, ptr, vptr, 1, -3, b"shard", shard_before)
    with engine.Index(base, "cosine", 0) as ix:               # ... and the same call on a plain handle with lists goes through
        ix.set_ivf(cen, off, lids)
        assert L.hnswgpu_ivf_update(ix._h, ptr, vptr, 1) == 0
        gi, gd = ix.ivf_search(vals[:1], 1, 8)
        assert gi[0, 0] == 3 and abs(gd[0, 0]) <= 1e-5


# ---- 9. composed with its neighbours --------------------------------------------------------------------------------------
def test_update_remove_add_update(native_lib, oracle, tune):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, 136)
    spare = rows[N0:]
    rng = np.random.default_rng(6)
    with engine.Index(rows[:N0], "cosine", 0) as ix:
        ix.set_rejection_test(2)
        ix.ivf_build(NLIST, 3, 42)
        cen, off, ids = ix.get_ivf()
        assign = _device_assign(engine, tune, spare, "cosine", cen)
        pairing = _Pairing(49, assign)
        cur = rows[:N0].copy()
        at, sp, moves = pairing.batch(_list_of(off, ids), 200)
        _assert_mixed(moves)
        off, ids = U.updated_lists(off, ids, at, assign[sp])
        ix.ivf_update(at, spare[sp])
        cur[at] = spare[sp]
        gone = np.concatenate([rng.choice(N0, 150, replace=False), at[:10]])    # old rows, and ten that were just updated
        off, ids = R.compact_lists(off, ids, gone)
        kept = ix.ivf_remove(gone)
        cur = cur[kept]
        added = np.arange(1000, 1100)                        # spare values the pairing has not reached
        assert pairing.next <= 1000
        ix.ivf_add(spare[added])
        off, ids = merged_lists(off, ids, assign[added])
        cur = np.concatenate([cur, spare[added]])
        pairing.next = 1100
        at, sp, moves = pairing.batch(_list_of(off, ids), 150)
        _assert_mixed(moves)
        assert (at >= len(kept)).any(), "the second update must reach rows that were added"
        off, ids = U.updated_lists(off, ids, at, assign[sp])
        ix.ivf_update(at, spare[sp])
        cur[at] = spare[sp]
        assert ix.n == len(cur) == N0 - len(np.unique(gone)) + 100
        _assert_same_ivf(ix, cen, off, ids)
        with _fresh(engine, cur, "cosine", 2, cen, off, ids, ix.ivf_stream_state()) as fresh:
            _assert_same_answers(engine, ix, fresh, Q)


# ---- 10. searches beside updates ------------------------------------------------------------------------------------------
def test_searches_beside_updates_see_one_of_the_index_states(native_lib, oracle, tune):
    from hnsw_clj_amd import engine

    rows, Q = _data(oracle, 64)
    spare = rows[N0:]
    qs = [np.ascontiguousarray(Q[3 * t:3 * t + 3]) for t in range(4)]
    with engine.Index(rows[:N0], "l2", 0) as ix:
        ix.ivf_build(NLIST, 3, 42)
        cen, off, ids = ix.get_ivf()
        assign = _device_assign(engine, tune, spare, "l2", cen)
        pairing = _Pairing(48, assign)
        cur = rows[:N0].copy()
        updates, states = [], []                            # per index state, per thread: (ids, distance bits), from fresh handles
        for s in range(4):
            if s > 0:
                at, sp, _ = pairing.batch(_list_of(off, ids), 300)
                updates.append((at, spare[sp]))
                off, ids = U.updated_lists(off, ids, at, assign[sp])
                cur[at] = spare[sp]
            with _fresh(engine, cur, "l2", None, cen, off, ids) as fresh:
                states.append([(i, _bits(d)) for i, d in (fresh.ivf_search(q, 10, 4) for q in qs)])
        stop, errors, seen = threading.Event(), [], [set() for _ in range(4)]

        def matches(t, i, d):
            return [s for s in range(4) if np.array_equal(i, states[s][t][0]) and np.array_equal(_bits(d), states[s][t][1])]

        def searcher(t):
            try:
                for _ in range(20000):                      # bounded: the updater sets `stop` long before
                    if stop.is_set():
                        break
                    hit = matches(t, *ix.ivf_search(qs[t], 10, 4))
                    if not hit:
                        raise AssertionError("thread %d: an answer that belongs to none of the four index states" % t)
                    seen[t].update(hit)
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
                stop.set()

        def updater():
            try:
                for s, (at, new) in enumerate(updates):
                    if stop.is_set():
                        return
                    ix.ivf_update(at, new)
                    for t in range(4):                      # the updated index is what every later search sees
                        assert s + 1 in matches(t, *ix.ivf_search(qs[t], 10, 4))
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
            finally:
                stop.set()

        threads = [threading.Thread(target=searcher, args=(t,), daemon=True) for t in range(4)]
        threads.append(threading.Thread(target=updater, daemon=True))
        for th in threads:
            th.start()
        for th in threads:
            th.join(STEP_SECONDS)
            assert not th.is_alive(), "a thread did not finish within its time limit"
        assert not errors, errors[0]
        assert ix.n == N0
        assert all(3 in matches(t, *ix.ivf_search(qs[t], 10, 4)) for t in range(4))
        _assert_same_ivf(ix, cen, off, ids)


# ---- 11. the Python mirror ------------------------------------------------------------------------------------------------
def test_python_mirror_update_vectors(native_lib, oracle):
    from hnsw_clj_amd import ivf_flat

    rows, _ = _data(oracle, 64)
    n0 = 600
    index = ivf_flat.build_index([("v-%d" % i, rows[i]) for i in range(n0)], num_partitions=8, max_iterations=2)
    try:
        names = list(index.ids)
        assert ivf_flat.search_knn(index, rows[33], 5, mode="precise")[0]["id"] == "v-33"
        new = {"v-33": rows[N0 + 1], "v-0": rows[N0 + 2], "v-599": rows[N0 + 3]}
        assert ivf_flat.update_vectors(index, list(new.items())) is index
        assert index.ids == names and ivf_flat.index_info(index)["vectors"] == n0
        for name, v in new.items():                          # the new vector is found at distance ~ 0 under its old id
            res = ivf_flat.search_knn(index, v, 5, mode="precise")
            assert res[0]["id"] == name and abs(res[0]["distance"]) <= 1e-5
        res = ivf_flat.search_knn(index, rows[34], 5, mode="precise")
        assert res[0]["id"] == "v-34" and abs(res[0]["distance"]) <= 1e-5       # its neighbours keep their ids
        gone = ivf_flat.search_knn(index, rows[33], 1, mode="precise")[0]
        assert gone["id"] != "v-33" or abs(gone["distance"]) > 1e-5             # the old values are gone
        with pytest.raises(KeyError):
            ivf_flat.update_vectors(index, [("v-1", rows[N0 + 4]), ("nobody", rows[N0 + 5])])
        with pytest.raises(ValueError):
            ivf_flat.update_vectors(index, [("v-1", rows[N0 + 4]), ("v-1", rows[N0 + 5])])
        res = ivf_flat.search_knn(index, rows[1], 5, mode="precise")
        assert res[0]["id"] == "v-1" and abs(res[0]["distance"]) <= 1e-5        # neither call touched the index
    finally:
        index.close()
