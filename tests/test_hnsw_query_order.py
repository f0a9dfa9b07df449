"""Ordered launches of the one-wave-per-query HNSW traversal (order_kernels.hpp; HNSWGPU_TUNE_HNSW_ORDER).

The order in which a launch deals its queries to the XCDs is a hint for the L2s and nothing else: with the key at 2 (every
wave-kernel launch) against 0 (never), on the same library and handle, ids, distance BITS and both per-query counters are equal
for every query -- whatever the batch size (the ragged end of the 8-way deal), the keys (one bin, all bins), the metric, the grid
(a persistent grid smaller than the batch), the entry point (device buffers, host buffers through a mapped slot or the staging
block) and the repeat pass (the queries that list themselves for it are the right ones).  The order itself is read back: a
permutation, sorted by (key, query index), the same for two calls.

2,000 x 128 gaussian rows (the smallest dim with int8 rows by default), M 8, ef 32, HNSW_WAVE = 2, rejection mode 2.  Batches of up
to 128 queries are small launches by default (several-CU / helper kernels); PREFETCH = 0 sends them to the wave kernel too, and
every ordered run checks the launch counters for the path it took."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scripted_graphs as sg  # noqa: E402
from util import assert_exact  # noqa: E402

pytestmark = pytest.mark.gpu

N, DIM, M, EF, K = 2000, 128, 8, 32, 10
P = 256                      # pivot rows: i * (N // P)
SENT_ID, SENT_D, SENT_ST = -7, -1.0, -3
METRICS = ("cosine", "dot", "l2")


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
    """One built index per metric, shared by the tests of this module (none of them changes it)."""
    made = {}

    def get(metric):
        if metric not in made:
            idx = eng.Index(data[0], metric)
            idx.set_rejection_test(2)
            idx.hnsw_build(M, 100, 42)
            made[metric] = idx
        return made[metric]

    yield get
    for idx in made.values():
        idx.close()


def _wave(tune):
    tune.set("HNSW_WAVE", 2)
    tune.set("PREFETCH", 0)     # no small-launch kernels: every batch size takes the wave kernel


def _dev_search(eng, idx, Q, k=K, ef=EF, allow=None):
    """hnswgpu_hnsw_search(_filtered)_dev into sentinel-filled buffers: ids, distances, stats as numpy."""
    import torch

    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    ids = torch.full((len(Q), k), SENT_ID, dtype=torch.int32, device=dev)
    d = torch.full((len(Q), k), SENT_D, dtype=torch.float32, device=dev)
    st = torch.full((len(Q), 2), SENT_ST, dtype=torch.int64, device=dev)
    if allow is None:
        idx.hnsw_search_dev(Qd, k, ef, out=(ids, d), stats=st)
    else:
        mask = torch.from_numpy(eng.pack_mask(allow, N).view(np.int32)).to(dev)
        idx.hnsw_search_filtered_dev(Qd, k, mask, ef, out=(ids, d), stats=st)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), d.cpu().numpy(), st.cpu().numpy()


def _both(eng, tune, search, tag):
    """search() with the key at 0 and at 2: the ordered run took the ordered wave kernel, the other did not; all equal."""
    out = {}
    for mode in (0, 2):
        tune.set("HNSW_ORDER", mode)
        w0, o0 = eng.debug_counter("hnsw_wave"), eng.debug_counter("hnsw_ordered")
        out[mode] = search()
        assert eng.debug_counter("hnsw_wave") > w0, "%s: the wave kernel did not run (key %d)" % (tag, mode)
        assert (eng.debug_counter("hnsw_ordered") > o0) == (mode == 2), "%s: ordered launches with the key at %d" % (tag, mode)
    (i0, d0, s0), (i2, d2, s2) = out[0], out[2]
    np.testing.assert_array_equal(s2, s0, err_msg=tag + ": counters")
    assert_exact(i2, d2, i0, d0, tag)
    return i2, d2, s2


def _check_order(idx, Q_len, tag):
    """The last launch's order: a permutation of the queries, sorted by (key, index); keys name pivots."""
    order, keys = idx.hnsw_last_order()
    assert len(order) == Q_len and len(keys) == Q_len, tag
    assert np.array_equal(np.sort(order), np.arange(Q_len)), tag + ": order[] is not a permutation"
    assert keys.min() >= 0 and keys.max() < P, tag
    assert (np.diff(keys[order]) >= 0).all(), tag + ": keys along order[] decrease"
    assert np.array_equal(order, np.argsort(keys, kind="stable")), tag + ": ties are not in query order"
    return order, keys


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nq", [1, 7, 8, 9, 63, 64, 65, 1000])
def test_every_query_is_answered_once_at_its_own_row(eng, indexes, data, tune, nq, metric):
    """Batch sizes around the 8-way deal's ragged end; the output buffers are pre-filled with a sentinel, so a query that no slot
    serves, or one answered at another query's row, shows."""
    idx, Q = indexes(metric), data[1][:nq]
    _wave(tune)
    ids, d, st = _both(eng, tune, lambda: _dev_search(eng, idx, Q), "%s nq %d, device buffers" % (metric, nq))
    assert (ids != SENT_ID).all() and (d != SENT_D).all() and (st != SENT_ST).all(), "a query was not answered"
    assert (st > 0).all()
    _check_order(idx, nq, "%s nq %d" % (metric, nq))
    # ... and through the host entry point: a mapped slot up to 256 queries, the staging block beyond
    _both(eng, tune, lambda: idx.hnsw_search(Q, K, EF, want_stats=True), "%s nq %d, host buffers" % (metric, nq))
    _check_order(idx, nq, "%s nq %d, host buffers" % (metric, nq))


@pytest.mark.parametrize("metric", METRICS)
def test_one_bin_and_all_bins(eng, indexes, data, tune, metric):
    """All queries equal: one key, order[] is the identity.  Queries that are copies of the pivot rows, shuffled: every key once.
    A gaussian row's nearest pivot is itself in all three metrics (q.q = |q|^2 ~ 128 against q.v ~ N(0, 11) for another row), by a
    margin thousands of times the int8 code's error, so the keys are known: keys[j] = the pivot query j copies."""
    idx, (base, Qs) = indexes(metric), data
    _wave(tune)
    same = np.tile(Qs[5], (100, 1))
    _both(eng, tune, lambda: _dev_search(eng, idx, same), metric + " equal queries")
    order, keys = _check_order(idx, 100, metric + " equal queries")
    assert (keys == keys[0]).all() and np.array_equal(order, np.arange(100))
    perm = np.random.RandomState(3).permutation(P)
    piv = base[perm * (N // P)]
    _both(eng, tune, lambda: _dev_search(eng, idx, piv), metric + " pivot rows as queries")
    order, keys = _check_order(idx, P, metric + " pivot rows as queries")
    assert np.array_equal(keys, perm), "a pivot row's nearest pivot is not itself"
    assert np.array_equal(order, np.argsort(perm))


def test_persistent_grid_smaller_than_the_batch(eng, indexes, data, tune):
    """The visited set in HBM stamps: a persistent grid (3,072 workgroups at this n) strides over the 4,000 slots."""
    idx, Q = indexes("cosine"), data[1]
    _wave(tune)
    tune.set("VIS_GLOBAL", 1)
    ids, d, st = _both(eng, tune, lambda: _dev_search(eng, idx, Q), "persistent grid")
    assert (ids != SENT_ID).all() and (st > 0).all()
    _check_order(idx, len(Q), "persistent grid")


def test_order_is_reproducible(eng, indexes, data, tune):
    idx, Q = indexes("l2"), data[1][:1000]
    _wave(tune)
    tune.set("HNSW_ORDER", 2)
    _dev_search(eng, idx, Q)
    o1, k1 = _check_order(idx, 1000, "first call")
    _dev_search(eng, idx, Q)
    o2, k2 = _check_order(idx, 1000, "second call")
    assert np.array_equal(o1, o2) and np.array_equal(k1, k2)
    assert len(np.unique(k1)) > 8, "1,000 gaussian queries fell into %d bins" % len(np.unique(k1))


@pytest.mark.parametrize("metric", METRICS)
def test_filtered_search(eng, indexes, data, tune, metric):
    """The allow-mask of a filtered search is applied to the traversal's per-query result lists: those stay indexed by the query.
    (The mask belongs to the call; three calls with different masks, sparse to dense.)"""
    idx, Q = indexes(metric), data[1][:300]
    _wave(tune)
    rs = np.random.RandomState(11)
    for frac in (0.05, 0.5, 0.95):
        allow = rs.rand(N) < frac
        ids, d, st = _both(eng, tune, lambda: _dev_search(eng, idx, Q, allow=allow), "%s filtered, %.2f pass" % (metric, frac))
        assert (ids != SENT_ID).all() and (st != SENT_ST).all()
        assert allow[ids[ids >= 0]].all()


@pytest.mark.parametrize("dim", sg.DIMS)
def test_repeat_pass_repeats_the_right_queries(eng, oracle, tune, dim):
    """S-tie-many (tests/scripted_graphs.py): 64 evicted entries tie the worst, twice the ghost slots -- the scripted query lists
    itself for the repeat pass.  Here it sits at scattered places among rows of the graph as queries, so slots and queries differ;
    ids, distance bits and counters equal the oracle's device-order search for every query, ordered or not, through device buffers
    (the repeat pass behind the launch) and host buffers (the caller's repeat pass behind a slot launch)."""
    O = oracle
    case = next(c for c, _ in sg.scenarios() if c.name.startswith("S-tie-many"))
    ef = case.efs[0]
    rows, Qs = sg.queries(case, "l2", dim)
    rs = np.random.RandomState(5)
    Q = rows[rs.choice(len(rows), 150, replace=False)].copy()
    at = np.array([0, 3, 8, 9, 64, 77, 120, 149])
    Q[at] = Qs[0]
    g = sg.graph(O, case)
    oi, od, ost = O.hnsw_search(rows, g, Q, sg.result_k(ef), ef=ef, metric=O.L2, mode=O.MODE_DEV)[:3]
    with eng.Index(rows, "l2") as idx:
        idx.set_rejection_test(2)
        idx.set_graph(g)
        _wave(tune)
        for what, search in (("device buffers", lambda: _dev_search(eng, idx, Q, k=sg.result_k(ef), ef=ef)),
                             ("host buffers", lambda: idx.hnsw_search(Q, sg.result_k(ef), ef, want_stats=True))):
            ids, d, st = _both(eng, tune, search, "S-tie-many dim %d, %s" % (dim, what))
            np.testing.assert_array_equal(st, ost, err_msg=what + ": counters against the oracle")
            assert_exact(ids, d, oi, od, what + " against the oracle")
