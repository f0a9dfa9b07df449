"""The dense bounds table in front of large HNSW launches (dense_kernels.hpp; hnswgpu_set_hnsw_dense_bounds).

The int8 dot product of a query code and a row is exact in any summation order, so the rejection test's lower bound of every
(query, row) pair computed as one int8 GEMM on the matrix cores is the float the traversal computes from the same pair, bit for
bit: hnswgpu_hnsw_dense_bounds against hnswgpu_hnsw_rejection_bounds, NaNs in the same places.  And a traversal that reads its
bounds from the table (mode 2: every eligible launch) decides what one that computes them decides (mode 0), on one handle: ids,
distance BITS, both per-query counters and the handle's (f32 rows, neighbours) pair are equal.

2,000-row indexes, M 8, ef 32, HNSW_WAVE = 2, PREFETCH = 0, rejection mode 2, as tests/test_hnsw_query_order.py.

Zero rows and zero queries: the traversal's own bound abstains (NaN) for them under cosine only -- under L2 and dot a zero vector
has an exact code and a finite bound -- so the table is held to hnswgpu_hnsw_rejection_bounds there, NaN for NaN, and to "all
NaN" where that function abstains for every metric: non-finite and uncoded tiny queries, rows holding NaN."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scripted_graphs as sg  # noqa: E402
from util import assert_exact  # noqa: E402

pytestmark = pytest.mark.gpu

N, DIM, M, EF, K = 2000, 128, 8, 32, 10
SENT_ID, SENT_D, SENT_ST = -7, -1.0, -3
METRICS = ("cosine", "dot", "l2")
NS = (1, 31, 32, 33, 2000, 2049)
NQS = (1, 31, 32, 33, 257)


@pytest.fixture(scope="module")
def eng(native_lib):
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    return engine


@pytest.fixture(scope="module")
def data():
    from hnsw_clj_amd import datagen

    return datagen.generate_dataset(N, DIM), datagen.generate_dataset(4000, DIM, seed=43)


@pytest.fixture(scope="module")
def indexes(eng, data):
    """One built index per metric, shared by the tests of this module (none of them changes its rows or graph)."""
    made = {}

    def get(metric):
        if metric not in made:
            idx = eng.Index(data[0], metric)
            idx.set_rejection_test(2)
            idx.hnsw_build(M, 100, 42)
            idx.set_profiling(True)      # the traversals count (f32 rows, neighbours)
            made[metric] = idx
        return made[metric]

    yield get
    for idx in made.values():
        idx.close()


def _wave(tune):
    tune.set("HNSW_WAVE", 2)
    tune.set("PREFETCH", 0)     # no small-launch kernels: every batch size takes the wave kernel


def _reference(idx, Q, n):
    """hnswgpu_hnsw_rejection_bounds of every query against all rows: (nq, n)."""
    ids = np.arange(n, dtype=np.int32)
    return np.stack([idx.hnsw_rejection_bounds(q, ids) for q in Q])


def _same_bits(tab, ref, tag):
    assert tab.shape == ref.shape, tag
    np.testing.assert_array_equal(np.isnan(tab), np.isnan(ref), err_msg=tag + ": NaNs in other places")
    ok = ~np.isnan(ref)
    np.testing.assert_array_equal(tab.view(np.uint32)[ok], ref.view(np.uint32)[ok], err_msg=tag + ": bound bits")


def _rows_and_queries(n, nq, dim, seed):
    rs = np.random.RandomState(seed)
    base = rs.randn(n, dim).astype(np.float32) * np.exp(rs.uniform(-2, 2, (n, 1))).astype(np.float32)
    Q = rs.randn(nq, dim).astype(np.float32) * np.exp(rs.uniform(-2, 2, (nq, 1))).astype(np.float32)
    return base, Q


# ---- the table itself

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", NS)
def test_table_equals_the_traversals_bounds_at_every_ragged_size(eng, metric, n):
    """Rows and queries around the 32-wide operand blocks and the 128-wide tiles, one tile and several; the reference of the 257
    queries is computed once per index and every smaller batch is its leading rows."""
    base, Q = _rows_and_queries(n, max(NQS), DIM, 100 + n)
    with eng.Index(base, metric) as idx:
        idx.set_rejection_test(2)
        ref = _reference(idx, Q, n)
        for nq in NQS:
            _same_bits(idx.hnsw_dense_bounds(Q[:nq]), ref[:nq], "%s n %d nq %d" % (metric, n, nq))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [128, 200, 768, 1000, 1030, 1536, 2048, 2050, 3072])
def test_table_at_every_code_range(eng, metric, dim):
    """Every K the kernel loops over: 200 (padded codes), 768, 1536 (A = 11008) and 3072 (A = 5504, where the planes' own products
    pass 2^31 before they are summed); 1000 and 2048 (the traversals' loaders of four and eight chunks), 1030 and 2050 (a last
    loader chunk that is padding from end to end).  Rows of the largest codes in every place (+-127 against +-A) among the gaussian
    ones."""
    for n, nq in ((2049, 33), (33, 257)):
        base, Q = _rows_and_queries(n, nq, dim, dim + n)
        base[0] = 3.0
        base[1] = -3.0
        Q[0] = 2.0
        Q[min(1, nq - 1)] = base[min(7, n - 1)]
        with eng.Index(base, metric) as idx:
            idx.set_rejection_test(2)
            _same_bits(idx.hnsw_dense_bounds(Q), _reference(idx, Q, n), "%s dim %d n %d nq %d" % (metric, dim, n, nq))


@pytest.mark.parametrize("metric", METRICS)
def test_table_of_a_strided_query_block(eng, indexes, data, metric):
    idx = indexes(metric)
    wide = np.full((40, DIM + 24), np.nan, np.float32)      # what lies between the queries is not read
    wide[:, :DIM] = data[1][:40]
    view = wide[:, :DIM]
    assert view.strides[0] == 4 * (DIM + 24)
    _same_bits(idx.hnsw_dense_bounds(view), _reference(idx, data[1][:40], N), metric + " qld > dim")


# ---- mode 2 against mode 0 on one handle

def _dev_search(eng, idx, Q, k=K, ef=EF):
    """hnswgpu_hnsw_search_dev into sentinel-filled buffers: ids, distances, stats as numpy."""
    import torch

    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    ids = torch.full((len(Q), k), SENT_ID, dtype=torch.int32, device=dev)
    d = torch.full((len(Q), k), SENT_D, dtype=torch.float32, device=dev)
    st = torch.full((len(Q), 2), SENT_ST, dtype=torch.int64, device=dev)
    idx.hnsw_search_dev(Qd, k, ef, out=(ids, d), stats=st)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), d.cpu().numpy(), st.cpu().numpy()


def _both(eng, idx, search, tag, used=True):
    """search() with the table never (0) and on every eligible launch (2): the state entry says which launches used it, and ids,
    distance bits, per-query counters and the handle's (f32 rows, neighbours) are equal."""
    out, rej = {}, {}
    for mode in (0, 2):
        idx.set_hnsw_dense_bounds(mode)
        idx.rejection_stats(reset=True)
        w0, l0 = eng.debug_counter("hnsw_wave"), idx.hnsw_dense_bounds_state()[2]
        out[mode] = search()
        rej[mode] = idx.rejection_stats(reset=True)
        assert eng.debug_counter("hnsw_wave") > w0, "%s: the wave kernel did not run (mode %d)" % (tag, mode)
        took = idx.hnsw_dense_bounds_state()[2] - l0
        assert (took > 0) == (mode == 2 and used), "%s: %d launches with the table in mode %d" % (tag, took, mode)
    idx.set_hnsw_dense_bounds(1)
    (i0, d0, s0), (i2, d2, s2) = out[0], out[2]
    np.testing.assert_array_equal(s2, s0, err_msg=tag + ": counters")
    assert_exact(i2, d2, i0, d0, tag)
    assert rej[2] == rej[0] and rej[0][1] > 0, "%s: (f32 rows, neighbours) %s with the table, %s without" % (tag, rej[2], rej[0])
    return i2, d2, s2


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nq", [1, 7, 8, 9, 63, 64, 65, 1000])
def test_search_with_the_table_equals_search_without(eng, indexes, data, tune, nq, metric):
    idx, Q = indexes(metric), data[1][:nq]
    _wave(tune)
    ids, d, st = _both(eng, idx, lambda: _dev_search(eng, idx, Q), "%s nq %d, device buffers" % (metric, nq))
    assert (ids != SENT_ID).all() and (d != SENT_D).all() and (st != SENT_ST).all(), "a query was not answered"
    # ... and through the host entry point: a mapped slot (its own table) up to 256 queries, the staging block beyond
    _both(eng, idx, lambda: idx.hnsw_search(Q, K, EF, want_stats=True), "%s nq %d, host buffers" % (metric, nq))


@pytest.mark.parametrize("metric", METRICS)
def test_ordered_launch_reads_the_table_by_query(eng, indexes, data, tune, metric):
    """HNSW_ORDER = 2: slots and queries differ; the table is indexed by the query."""
    idx, Q = indexes(metric), data[1][:1000]
    _wave(tune)
    tune.set("HNSW_ORDER", 2)
    o0 = eng.debug_counter("hnsw_ordered")
    ids, d, st = _both(eng, idx, lambda: _dev_search(eng, idx, Q), metric + " ordered")
    assert eng.debug_counter("hnsw_ordered") >= o0 + 2 and (ids != SENT_ID).all()


def test_persistent_grid(eng, indexes, data, tune):
    """The visited set in HBM stamps (VIS_GLOBAL forced): a persistent grid (3,072 workgroups at this n) strides over 4,000 slots."""
    idx, Q = indexes("cosine"), data[1]
    _wave(tune)
    tune.set("VIS_GLOBAL", 1)
    ids, d, st = _both(eng, idx, lambda: _dev_search(eng, idx, Q), "persistent grid")
    assert (ids != SENT_ID).all() and (st > 0).all()
    tune.set("HNSW_ORDER", 2)
    _both(eng, idx, lambda: _dev_search(eng, idx, Q), "persistent grid, ordered")


@pytest.mark.parametrize("dim", sg.DIMS)
def test_repeat_pass_behind_a_launch_with_the_table(eng, oracle, tune, dim):
    """S-tie-many (tests/scripted_graphs.py): the scripted query lists itself for the repeat pass, which keeps computing its own
    bounds (hnsw_search_kernel).  Equal to mode 0 and to the oracle's device-order search, through device and host buffers."""
    O = oracle
    case = next(c for c, _ in sg.scenarios() if c.name.startswith("S-tie-many"))
    ef = case.efs[0]
    rows, Qs = sg.queries(case, "l2", dim)
    rs = np.random.RandomState(5)
    Q = rows[rs.choice(len(rows), 150, replace=False)].copy()
    Q[np.array([0, 3, 8, 9, 64, 77, 120, 149])] = Qs[0]
    g = sg.graph(O, case)
    oi, od, ost = O.hnsw_search(rows, g, Q, sg.result_k(ef), ef=ef, metric=O.L2, mode=O.MODE_DEV)[:3]
    with eng.Index(rows, "l2") as idx:
        idx.set_rejection_test(2)
        idx.set_graph(g)
        idx.set_profiling(True)
        _wave(tune)
        for what, search in (("device buffers", lambda: _dev_search(eng, idx, Q, k=sg.result_k(ef), ef=ef)),
                             ("host buffers", lambda: idx.hnsw_search(Q, sg.result_k(ef), ef, want_stats=True))):
            ids, d, st = _both(eng, idx, search, "S-tie-many dim %d, %s" % (dim, what))
            np.testing.assert_array_equal(st, ost, err_msg=what + ": counters against the oracle")
            assert_exact(ids, d, oi, od, what + " against the oracle")


# ---- special values

def _special(base, Qs):
    rows = base.copy()
    rows[5] = 0.0
    Q = Qs[:40].copy()
    Q[5] = 0.0
    Q[6] = (Qs[6].astype(np.float64) * 1e-20).astype(np.float32)
    assert 0 < np.abs(Q[6]).max() < 1e-18
    return rows, Q


@pytest.mark.parametrize("metric", METRICS)
def test_table_of_special_queries_and_rows(eng, data, metric):
    """Queries: NaN, infinity, all zero, largest component below 1e-18 (no code).  Rows: all zero, holding NaN.  The table's rows
    and columns abstain (NaN) exactly where the traversal's own bounds do."""
    rows, Q = _special(*data)
    rows[9, 17] = np.nan
    Q[3, 100] = np.nan
    Q[4, 0] = np.inf
    with eng.Index(rows, metric) as idx:
        idx.set_rejection_test(2)
        tab = idx.hnsw_dense_bounds(Q)
        _same_bits(tab, _reference(idx, Q, N), metric + " special values")
        assert np.isnan(tab[[3, 4, 6]]).all(), "a non-finite or uncoded query got a bound"
        assert np.isnan(tab[:, 9]).all(), "a row holding NaN got a bound"
        if metric == "cosine":          # (L2 and dot code a zero vector exactly: a finite bound)
            assert np.isnan(tab[5]).all() and np.isnan(tab[:, 5]).all()
        assert not np.isnan(np.delete(np.delete(tab, [3, 4, 5, 6], axis=0), [5, 9], axis=1)).any()


@pytest.mark.parametrize("metric", METRICS)
def test_search_of_special_queries_and_rows(eng, indexes, data, tune, metric):
    """The zero query, the uncoded tiny query (NaN rows of the table: every neighbour takes the exact path) and the zero row, in a
    copy of the shared index's rows under ITS graph: the search equals mode 0's.

    NOT searched: queries holding NaN or infinity, and rows holding NaN.  Every distance of such a pair is NaN, and the
    traversal's list (hnsw_list.hpp: admit) ranks several NaN survivors of one expansion at the same buffer place, so that it
    takes the places between them from LDS nobody has written: hnsw_wave_kernel then follows node ids that are whatever the
    workgroup before it left there, whichever way its bounds are computed.  Measured once, on the three metrics: the table's
    NaN rows and column are right (above), but searching with the table NEVER on, twice, on one handle, already gives other ids
    for the NaN / infinity query (and under dot for a finite query that reaches the NaN row: counters 452 / 46 against 161 /
    22).  A search that has no reproducible answer, and reads adjacency at ids it did not write, is not run on the device
    again by this suite."""
    rows, Q = _special(*data)
    g = indexes(metric).get_graph()
    with eng.Index(rows, metric) as idx:
        idx.set_rejection_test(2)
        idx.set_graph(g)
        idx.set_profiling(True)
        tab = idx.hnsw_dense_bounds(Q)
        assert np.isnan(tab[6]).all() and (metric != "cosine" or (np.isnan(tab[5]).all() and np.isnan(tab[:, 5]).all()))
        _wave(tune)
        ids, d, st = _both(eng, idx, lambda: _dev_search(eng, idx, Q), metric + " special values")
        assert not np.isnan(d).any()


# ---- scratch

def test_budget_below_the_need(eng, indexes, data, tune):
    """1,000 queries x 2,048 floats are 7.8 MiB: with a budget of 4 MiB the launch takes today's path and says so."""
    idx, Q = indexes("dot"), data[1][:1000]
    _wave(tune)
    try:
        idx.set_hnsw_dense_bounds(2, 4)
        assert idx.hnsw_dense_bounds_state()[:2] == (2, 4)
        _both(eng, idx, lambda: _dev_search(eng, idx, Q), "budget 4 MiB", used=False)
        idx.set_hnsw_dense_bounds(2, 8)
        _both(eng, idx, lambda: _dev_search(eng, idx, Q), "budget 8 MiB")
    finally:
        idx.set_hnsw_dense_bounds(1, 2048)
    assert idx.hnsw_dense_bounds_state()[:2] == (1, 2048)


def test_table_is_reused_by_growing_and_shrinking_batches(eng, indexes, data, tune):
    idx, Qs = indexes("l2"), data[1]
    _wave(tune)
    sizes = []
    for nq in (300, 1500, 40, 1500, 700, 3000, 9):
        _both(eng, idx, lambda: _dev_search(eng, idx, Qs[:nq]), "nq %d after %s" % (nq, sizes))
        sizes.append(idx.hnsw_dense_bounds_state()[3])
    assert sizes[1] > sizes[0] and sizes[5] > sizes[4], sizes
    assert sizes[2] == sizes[1] == sizes[3] == sizes[4] and sizes[6] == sizes[5], "the scratch shrank or grew without need: %s" % sizes
    assert sizes[5] >= 3000 * 2048 * 4


def test_after_hnsw_add_the_table_follows_n(eng, data, tune):
    """2,000 rows + 100: n passes the 2,048 of the first tile row, so the table's row stride changes.  Equal to a fresh handle that
    took the same steps with the table never on."""
    base, Qs = data
    Q, extra = Qs[:500], Qs[3000:3100]
    _wave(tune)
    res = {}
    for mode in (0, 2):
        with eng.Index(base, "cosine") as idx:
            idx.set_rejection_test(2)
            idx.set_hnsw_dense_bounds(mode)
            idx.hnsw_build(M, 100, 42)
            before = _dev_search(eng, idx, Q)
            idx.hnsw_add(extra, 100, 7)
            after = _dev_search(eng, idx, Q)
            assert (idx.hnsw_dense_bounds_state()[2] == 2) == (mode == 2)
            _same_bits(idx.hnsw_dense_bounds(Q[:33]), _reference(idx, Q[:33], N + 100), "after hnsw_add")
            res[mode] = before + after
    for x0, x2 in zip(res[0], res[2]):
        np.testing.assert_array_equal(x2.view(np.uint32) if x2.dtype == np.float32 else x2,
                                      x0.view(np.uint32) if x0.dtype == np.float32 else x0)
    assert (res[2][3] >= N).any(), "no added row among the results: the second search did not see the grown index"
