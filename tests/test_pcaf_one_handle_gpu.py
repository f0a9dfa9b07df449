"""P-HNSW on one handle (include/hnswgpu.h "P-HNSW"; pcaf_kernels.hpp): projection, low-dimensional filter and exact refine
against a plain float64 restatement of pcaf.clj:195-253."""
import numpy as np
import pytest

import util
from hnsw_clj_amd import datagen, engine, pcaf

pytestmark = pytest.mark.gpu


def reference(base, P, Q, k, k_filter):
    """f64: rows and queries projected by the f32 matrix P, the kf = min(k_filter, 3 k, n) smallest projected cosine distances
    (ties to the lower id), f64 cosine on the original rows of those, the min(k, kf) smallest.
    -> ids [nq][k] (-1 padded), distances (+inf padded), decided [nq], projected rows, projected queries"""
    def cos(a, b):
        den = np.linalg.norm(a, axis=1)[:, None] * np.linalg.norm(b, axis=1)[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(den > 0, 1.0 - (a @ b.T) / den, 1.0)

    base, P, Q = (np.asarray(x, np.float64) for x in (base, P, Q))
    n, kf = len(base), min(k_filter or 32, 3 * k, len(base))
    low, qlow = base @ P.T, Q @ P.T
    d1 = cos(qlow, low)
    ids = np.full((len(Q), k), -1, np.int32)
    dist = np.full((len(Q), k), np.inf)
    decided = np.ones(len(Q), bool)
    for q in range(len(Q)):
        order = np.lexsort((np.arange(n), d1[q]))
        if kf < n:
            a, b = d1[q][order[kf - 1]], d1[q][order[kf]]
            decided[q] = b - a > util.RTOL * abs(b) + util.ATOL
        cand = order[:kf]
        d2 = cos(Q[q:q + 1], base[cand])[0]
        top = np.lexsort((cand, d2))[:k]
        ids[q, :len(top)], dist[q, :len(top)] = cand[top], d2[top]
    return ids, dist, decided, low, qlow


def clustered(n, dim, seed=42):
    return datagen.generate_dataset(n, dim, "clustered", num_clusters=20, noise_level=0.6, seed=seed)


@pytest.mark.parametrize("n,dim,T,nq,k,k_filter", [
    (1500, 96, 16, 33, 10, 32),   # two query blocks, the second ragged; kf = 30
    (1500, 100, 20, 1, 8, 24),    # dim and T off the tile granularities; a single query
    (700, 768, 100, 32, 10, 32),  # the reference's defaults
    (300, 36, 8, 5, 30, 64),      # kf = 64 against a 2 kf buffer that refills many times
    (20, 96, 16, 4, 10, 32),      # kf = n: every row is a candidate, no padding
    (6, 96, 16, 4, 10, 32),       # kf = n < k: padding
])
def test_search_parity(native_lib, n, dim, T, nq, k, k_filter):
    base, Q = clustered(n, dim), clustered(nq, dim, seed=44)  # (seed: the f64 reference alone leaves at most 1 query in 8 undecided)
    with engine.Index(base, "cosine", 0) as idx:
        assert idx.pcaf_sizes() == 0
        idx.pcaf_build(T, 42)
        assert idx.pcaf_sizes() == T
        P, low = idx.pcaf_get()
        np.testing.assert_array_equal(P.view(np.uint32), pcaf.create_random_projection(dim, T).view(np.uint32))
        want_ids, want_d, decided, want_low, want_qlow = reference(base, P, Q, k, k_filter)
        assert util.close(low, want_low, util.metric_scale("dot", base, P)).all()
        assert util.close(idx.pcaf_project(Q), want_qlow, util.metric_scale("dot", Q, P)).all()
        ids, d = idx.pcaf_search(Q, k, k_filter)
    print("undecided queries: %d of %d" % ((~decided).sum(), nq))
    assert (~decided).sum() * 8 <= nq
    util.assert_topk_parity(ids[decided], d[decided], want_ids[decided], want_d[decided], "decided")
    for q in np.flatnonzero(~decided):   # the returned distances are those of the returned ids
        got = ids[q][ids[q] >= 0]
        assert len(got) == min(k, k_filter, 3 * k, n) and len(set(got.tolist())) == len(got)
        a, b = np.float64(Q[q]), np.float64(base[got])
        f64 = 1.0 - b @ a / (np.linalg.norm(b, axis=1) * np.linalg.norm(a))
        assert util.close(d[q][:len(got)], f64).all() and np.isinf(d[q][len(got):]).all()


@pytest.mark.parametrize("kf,k", [(3, 3), (32, 12)])
@pytest.mark.parametrize("planted_last", [False, True])
def test_two_phases_not_an_exact_search(native_lib, kf, k, planted_last):
    """The projection keeps the first T coordinates, so phase 1 is computable by hand: the query's true nearest row points
    away from it there and never becomes a candidate; kf rows aligned there are all the candidates; two of them are equal."""
    dim, T, rng = 32, 8, np.random.RandomState(7)
    head, tail = np.eye(T)[0], rng.randn(dim - T)
    q = np.concatenate([0.2 * head, tail])
    planted = np.concatenate([-0.01 * head, tail])                 # cosine distance to q under 1e-3 overall, 2 in the first T
    twin = np.concatenate([head + 0.01 * np.eye(T)[1], 0.8 * tail])
    aligned = [np.concatenate([head + 0.02 * (i + 2) * np.eye(T)[1 + i % (T - 1)], rng.randn(dim - T)]) for i in range(kf - 2)]
    fillers = [np.concatenate([np.eye(T)[1 + i % (T - 1)], rng.randn(dim - T)]) for i in range(40)]
    rows = fillers[:20] + [twin] + aligned + fillers[20:] + [twin]
    rows = rows + [planted] if planted_last else [planted] + rows
    base, Q = np.float32(rows), np.float32([q])
    planted_id, twins = (len(rows) - 1 if planted_last else 0), np.flatnonzero((base == np.float32(twin)).all(axis=1))
    with engine.Index(base, "cosine", 0) as idx:
        idx.set_pcaf(np.eye(T, dim, dtype=np.float32))
        np.testing.assert_array_equal(idx.pcaf_get()[1], base[:, :T])
        ids, d = idx.pcaf_search(Q, k, kf)
        exact, _ = idx.exact_knn(Q, 1)
    want_ids, _, decided, _, _ = reference(base, np.eye(T, dim), Q, k, kf)
    assert exact[0, 0] == planted_id and planted_id not in ids[0]
    assert decided.all()
    np.testing.assert_array_equal(ids, want_ids)
    assert ids[0].tolist()[:2] == twins.tolist() and d[0, 0] == d[0, 1]


@pytest.mark.parametrize("mode", [None, "turbo", "precise"])
def test_mirror(native_lib, mode):
    vecs, Q, k = clustered(1500, 96), clustered(24, 96, seed=43), 10
    data = datagen.indexed(vecs)
    one, three = pcaf.build_index(data, n_components=16, one_handle=True), pcaf.build_index(data, n_components=16)
    try:
        assert pcaf.index_info(one) == pcaf.index_info(three)
        _, _, decided, _, _ = reference(vecs, one.projection, Q, k, pcaf.MODE_K_FILTER.get(mode, 32))
        a, b = pcaf.search_batch(one, Q, k, mode), pcaf.search_batch(three, Q, k, mode)
        for q in np.flatnonzero(decided):
            assert [r["id"] for r in a[q]] == [r["id"] for r in b[q]], (mode, q)
        for ra, rb in zip(a, b):
            assert len(ra) == len(rb) == k
            assert util.close([r["distance"] for r in ra], [r["distance"] for r in rb]).all()
        assert pcaf.search_knn(one, vecs[5], 3)[0]["id"] == "vec_5"
    finally:
        pcaf.cleanup(one)
        pcaf.cleanup(three)


ROWS, QS = clustered(200, 32), clustered(3, 32, seed=43)


@pytest.mark.parametrize("metric,state,call,code", [
    ("l2", None, lambda i: i.pcaf_build(8, 42), -1),
    ("cosine", None, lambda i: i.pcaf_build(0, 42), -1),
    ("cosine", None, lambda i: i.pcaf_build(257, 42), -5),
    ("cosine", "pcaf", lambda i: i.pcaf_search(QS, 43, 129), -5),
    ("cosine", None, lambda i: i.pcaf_search(QS, 5), -3),
    ("cosine", "graph", lambda i: i.pcaf_build(8, 42), -3),
    ("cosine", "pcaf", lambda i: i.hnsw_build(8, 40, 42), -3),
    ("cosine", "pcaf", lambda i: i.ivf_build(4, 2, 42), -3),
    ("cosine", "pcaf", lambda i: i.lsh_build(2, 4, 8, 42), -3),
    ("cosine", "pcaf", lambda i: i.ivf_add(ROWS[:2]), -3),
])
def test_refusals(native_lib, metric, state, call, code):
    with engine.Index(ROWS, metric, 0) as idx:
        if state == "pcaf":
            idx.pcaf_build(8, 42)
        elif state == "graph":
            idx.hnsw_build(8, 40, 42)
        search = {"pcaf": lambda: idx.pcaf_search(QS, 5), "graph": lambda: idx.hnsw_search(QS, 5, 32)[:2],
                  None: lambda: idx.exact_knn(QS, 5)}[state]
        before = search()
        with pytest.raises(engine._native.HnswGpuError) as e:
            call(idx)
        assert e.value.code == code, str(e.value)
        after = search()
        assert idx.n == len(ROWS) and idx.pcaf_sizes() == (8 if state == "pcaf" else 0)
        np.testing.assert_array_equal(before[0], after[0])
        np.testing.assert_array_equal(before[1], after[1])
