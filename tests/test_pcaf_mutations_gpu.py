"""Rows join, leave and take new values on a live P-HNSW handle (include/hnswgpu.h "P-HNSW": hnswgpu_pcaf_add / _remove /
_update): the mutated handle against a fresh one over the rows it should hold (numpy's concatenate, delete and indexed
assignment), bit for bit, and against the float64 restatement of pcaf.clj."""
import ctypes
import functools

import numpy as np
import pytest

import util
from hnsw_clj_amd import datagen, engine, pcaf
from test_pcaf_one_handle_gpu import clustered, reference

pytestmark = pytest.mark.gpu

NQ, K, KF = 33, 10, 32  # two query blocks, the second ragged


@functools.lru_cache(maxsize=None)
def pool(dim):
    """rows to draw from (read only), queries"""
    rows, Q = clustered(1600, dim), clustered(NQ, dim, seed=44)
    rows.setflags(write=False)
    return rows, Q


def scattered(count):
    return lambda n, rng: rng.choice(n, count, replace=False)


def ends_and(count):
    """`count` >= 2 shuffled ids that include 0 and n - 1"""
    return lambda n, rng: rng.permutation(np.concatenate([[0, n - 1], 1 + rng.choice(n - 2, count - 2, replace=False)]))


INTERLEAVED = (700, [("add", 129), ("remove", scattered(50)), ("update", ends_and(33)), ("add", 1)])
SCRIPTS = {"add_%d_onto_%d" % (m, n0): (n0, [("add", m)]) for m in (1, 33, 129) for n0 in (0, 1, 700)}
SCRIPTS.update({
    "remove_first": (700, [("remove", lambda n, rng: [0])]),
    "remove_last": (700, [("remove", lambda n, rng: [699])]),
    "remove_word_named_twice": (700, [("remove", lambda n, rng: list(range(32, 64)) * 2)]),
    "remove_scattered": (700, [("remove", scattered(50))]),
    "remove_all_but_6": (700, [("remove", scattered(694))]),
    "remove_all_then_add": (700, [("remove", lambda n, rng: rng.permutation(n)), ("add", 40)]),
    "update_1": (700, [("update", lambda n, rng: [n - 1])]),
    "update_33": (700, [("update", ends_and(33))]),
    "update_129": (700, [("update", ends_and(129))]),
    "update_to_same": (700, [("same", ends_and(129))]),
    "interleaved": INTERLEAVED,
})


def play(idx, dim, script, seed=7):
    """The script on the handle (None: on the model alone) and on the numpy model -> the rows the handle should now hold."""
    n0, steps = script
    rows, _ = pool(dim)
    X, used, rng = rows[:n0].copy(), n0, np.random.RandomState(seed)
    for op, arg in steps:
        if op == "add":
            new, used = rows[used:used + arg], used + arg
            if idx is not None:
                np.testing.assert_array_equal(idx.pcaf_add(new), np.arange(len(X), len(X) + arg))
            X = np.concatenate([X, new])
            continue
        ids = np.asarray(arg(len(X), rng), np.int32)
        if op == "remove":
            X = np.delete(X, ids, axis=0)
            if idx is not None:
                assert idx.pcaf_remove(ids) == len(X)
        else:
            new = X[ids] if op == "same" else rows[used:used + len(ids)]
            used += 0 if op == "same" else len(ids)
            if idx is not None:
                idx.pcaf_update(ids, new)
            X[ids] = new
    return X


def observe(idx, Q, allow):
    got = [idx.pcaf_get()[1], idx.norms(), *idx.pcaf_search(Q, K, KF),
           *idx.pcaf_search_filtered(Q, K, engine.pack_mask(allow, idx.n), KF)]
    return [np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a for a in got]


@pytest.mark.parametrize("name", list(SCRIPTS))
@pytest.mark.parametrize("dim,T", [(96, 16), (100, 20), (768, 100)])
def test_mutated_handle_equals_fresh(native_lib, dim, T, name):
    rows, Q = pool(dim)
    P = pcaf.create_random_projection(dim, T)
    n0 = SCRIPTS[name][0]
    with engine.Index(rows[:n0], "cosine", 0) as idx:
        idx.set_pcaf(P)
        before = observe(idx, Q, np.random.RandomState(3).rand(n0) < 0.5) if name == "update_to_same" else None
        want_rows = play(idx, dim, SCRIPTS[name])
        assert idx.n == len(want_rows)
        allow = np.random.RandomState(3).rand(idx.n) < 0.5  # (n unchanged: the mask of `before`)
        got = observe(idx, Q, allow)
        for a, b in zip(got, before or []):
            np.testing.assert_array_equal(a, b)
    with engine.Index(want_rows, "cosine", 0) as fresh:
        fresh.set_pcaf(P)
        want = observe(fresh, Q, allow)
    for what, a, b in zip(("low rows", "norms", "ids", "distances", "filtered ids", "filtered distances"), got, want):
        np.testing.assert_array_equal(a, b, err_msg=what)


@pytest.mark.parametrize("dim,T", [(100, 20), (768, 100)])
def test_mutated_handle_against_f64(native_lib, dim, T):
    """(seeds of pool() and play(): the f64 reference alone leaves at most 1 query in 8 undecided over the expected rows)"""
    rows, Q = pool(dim)
    P = pcaf.create_random_projection(dim, T)
    with engine.Index(rows[:INTERLEAVED[0]], "cosine", 0) as idx:
        idx.set_pcaf(P)
        X = play(idx, dim, INTERLEAVED)
        ids, d = idx.pcaf_search(Q, K, KF)
    want_ids, want_d, decided, _, _ = reference(X, P, Q, K, KF)
    print("undecided queries: %d of %d" % ((~decided).sum(), NQ))
    assert (~decided).sum() * 8 <= NQ
    util.assert_topk_parity(ids[decided], d[decided], want_ids[decided], want_d[decided], "decided")
    for q in np.flatnonzero(~decided):   # the returned distances are those of the returned ids
        got = ids[q][ids[q] >= 0]
        assert len(got) == K and len(set(got.tolist())) == K
        a, b = np.float64(Q[q]), np.float64(X[got])
        f64 = 1.0 - b @ a / (np.linalg.norm(b, axis=1) * np.linalg.norm(a))
        assert util.close(d[q], f64).all()


def test_return_codes_leave_the_handle_untouched(native_lib):
    L, dim, n = native_lib.lib(), 96, 200
    rows, _ = pool(dim)
    new = np.ascontiguousarray(rows[1000:1004])
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    i32 = lambda *v: np.asarray(v, np.int32)           # noqa: E731
    n_after = ctypes.c_int64(-7)
    with engine.Index(rows[:n], "cosine", 0) as idx, engine.Index(rows[:n], "cosine", 0) as plain:
        idx.set_pcaf(pcaf.create_random_projection(dim, 16))
        h, before = idx._h, (idx.pcaf_get()[1].view(np.uint32), idx.norms().view(np.uint32))
        add = lambda hh, r, m: L.hnswgpu_pcaf_add(hh, r, m)                                      # noqa: E731
        remove = lambda hh, i, m: L.hnswgpu_pcaf_remove(hh, i, m, ctypes.byref(n_after))         # noqa: E731
        update = lambda hh, i, r, m: L.hnswgpu_pcaf_update(hh, i, r, m)                          # noqa: E731
        ids0 = ptr(i32(0))
        cases = [
            # 1. a null handle (before m == 0), m < 0, null arrays with m > 0
            (lambda: add(None, ptr(new), 0), -1), (lambda: remove(None, ids0, 0), -1), (lambda: update(None, ids0, ptr(new), 0), -1),
            (lambda: add(h, ptr(new), -1), -1), (lambda: remove(h, ids0, -1), -1), (lambda: update(h, ids0, ptr(new), -1), -1),
            (lambda: add(h, None, 1), -1), (lambda: remove(h, None, 1), -1),
            (lambda: update(h, None, ptr(new), 1), -1), (lambda: update(h, ids0, None, 1), -1),
            # 2. m == 0, also on a handle without the state
            (lambda: add(h, None, 0), 0), (lambda: remove(h, None, 0), 0), (lambda: update(h, None, None, 0), 0),
            (lambda: add(plain._h, None, 0), 0),
            # 3. no P-HNSW state
            (lambda: add(plain._h, ptr(new), 1), -3), (lambda: remove(plain._h, ids0, 1), -3),
            (lambda: update(plain._h, ids0, ptr(new), 1), -3),
            # 4. too many rows, before `rows` is read
            (lambda: add(h, ptr(new), 2**31 - 1 - n), -5),
            # 5. ids outside [0, n); an id named twice
            (lambda: remove(h, ptr(i32(3, n)), 2), -1), (lambda: remove(h, ptr(i32(-1)), 1), -1),
            (lambda: update(h, ptr(i32(n, 3)), ptr(new), 2), -1), (lambda: update(h, ptr(i32(5, 9, 5)), ptr(new), 3), -1),
            # the other families still refuse the handle
            (lambda: L.hnswgpu_lsh_add(h, ptr(new), 1), -3), (lambda: L.hnswgpu_ivf_add(h, ptr(new), 1), -3),
        ]
        for i, (call, want) in enumerate(cases):
            assert call() == want, (i, L.hnswgpu_last_error())
            assert idx.n == n and idx.pcaf_sizes() == 16
            np.testing.assert_array_equal(idx.pcaf_get()[1].view(np.uint32), before[0])
            np.testing.assert_array_equal(idx.norms().view(np.uint32), before[1])
        assert remove(h, None, 0) == 0 and n_after.value == n  # (m == 0: *n_after = n)


def test_mirror_keeps_ids_in_step(native_lib):
    rows = pool(96)[0].copy()
    first = lambda ix, v: pcaf.search_knn(ix, v, 3)[0]["id"]  # noqa: E731
    one = pcaf.build_index(datagen.indexed(rows[:300]), n_components=16, one_handle=True)
    three = pcaf.build_index(datagen.indexed(rows[:50]), n_components=16)
    try:
        last = one.ids[-1]
        pcaf.add_vectors(one, [("new_%d" % i, v) for i, v in enumerate(rows[300:340])])
        assert len(one.ids) == one.high_index.n == 340 and first(one, rows[333]) == "new_33"
        gone = [one.ids[i] for i in (0, 17, 200, 338)]
        pcaf.remove_vectors(one, gone)
        assert len(one.ids) == one.high_index.n == 336
        for i in (0, 17, 200, 338):
            assert not set(gone) & {r["id"] for r in pcaf.search_knn(one, rows[i], 10)}
        assert first(one, rows[299]) == last and first(one, rows[339]) == "new_39"
        pcaf.update_vectors(one, [(last, rows[900])])
        assert first(one, rows[900]) == last and first(one, rows[299]) != last and one.ids.count(last) == 1
        with pytest.raises(KeyError):
            pcaf.remove_vectors(one, ["nobody"])
        for call in (lambda: pcaf.add_vectors(three, [("x", rows[60])]), lambda: pcaf.remove_vectors(three, [three.ids[0]]),
                     lambda: pcaf.update_vectors(three, [(three.ids[0], rows[60])])):
            with pytest.raises(ValueError):
                call()
    finally:
        pcaf.cleanup(one)
        pcaf.cleanup(three)
