"""Rows in flight of the dense-table traversal on 768-float rows (wave_kernels.hpp: DENSE, NCH 3; hnswgpu_hnsw_dense_rows).

A launch with the dense bounds table gathers the f32 rows of a hop two or four at a time, as hnsw_launch_plan decides (setting 0) or as
the handle's setting forces (2 / 4); a four-row instance ends a hop whose last trip needs one or two rows with the two-row trip.  A row's
distance does not depend on the trip that fetched it, so on one handle setting 4, setting 2 and a launch without the table (mode 0) give
the same ids, distance BITS, per-query counters and (f32 rows, neighbours) pair.

Set-up as tests/test_hnsw_dense_bounds.py: HNSW_WAVE 2, PREFETCH 0, rejection mode 2, set_hnsw_dense_bounds(2), profiling on.
2,000 rows of dim 768 and 700 (three loader chunks, the last one full and padded), M 16: a layer-0 node has 32 slots, so a hop
needs up to 32 rows.  The hops' needs are restated on the CPU (need_trace: the reference's loop with the table's bounds) and
checked against the device's own count of fetched rows, so that "hops that need 1, 2, 3, 4, 5, ... rows occur" is asserted,
not assumed."""
import bisect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scripted_graphs as sg  # noqa: E402
from util import assert_exact  # noqa: E402

pytestmark = pytest.mark.gpu

N, M, EFC, K = 2000, 16, 100, 10
DIMS = (768, 700)
METRICS = ("cosine", "dot", "l2")
NQS = (1, 33, 257)
EFS = (16, 64, 640)
NTRACE = 33                       # queries whose hops are restated on the CPU
SENT_ID, SENT_D, SENT_ST = -7, -1.0, -3
K_GHOST, MAX_DEG, DENSE_ROWS4_LDS = 32, 64, 7680      # kernels.hpp: kGhost, kMaxDeg; hnsw.hip: kDenseRows4Lds


@pytest.fixture(scope="module")
def eng(native_lib):
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    return engine


@pytest.fixture(scope="module")
def data():
    from hnsw_clj_amd import datagen

    return {dim: (datagen.generate_dataset(N, dim), datagen.generate_dataset(4000, dim, seed=43)) for dim in DIMS}


@pytest.fixture(scope="module")
def indexes(eng, data):
    """One built index per (dim, metric), shared by the tests of this module (none of them changes its rows or graph)."""
    made = {}

    def get(dim, metric):
        if (dim, metric) not in made:
            idx = eng.Index(data[dim][0], metric)
            idx.set_rejection_test(2)
            idx.hnsw_build(M, EFC, 42)
            idx.set_profiling(True)      # the traversals count (f32 rows, neighbours)
            made[dim, metric] = idx
        return made[dim, metric]

    yield get
    for idx in made.values():
        idx.close()


def _wave(tune):
    tune.set("HNSW_WAVE", 2)
    tune.set("PREFETCH", 0)     # no small-launch kernels: every batch size takes the wave kernel


def _dev_search(idx, Q, k, ef):
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


def _launch(eng, idx, tune, search, mode, rows, tag):
    """search() with the table in `mode` and the rows setting at `rows`: (ids, d, stats, (f32 rows, neighbours), launches that took
    four rows).  The launch counters and the handle's state say which kernel served it."""
    idx.set_hnsw_dense_bounds(mode)
    assert idx.hnsw_dense_rows(rows)[0] == rows
    idx.rejection_stats(reset=True)
    w0, l0, r0 = eng.debug_counter("hnsw_wave"), idx.hnsw_dense_bounds_state()[2], idx.hnsw_dense_rows()[1]
    out = search()
    rej = idx.rejection_stats(reset=True)
    assert eng.debug_counter("hnsw_wave") > w0, tag + ": the wave kernel did not run"
    took = idx.hnsw_dense_bounds_state()[2] - l0
    assert (took > 0) == (mode == 2), "%s: %d launches with the table in mode %d" % (tag, took, mode)
    four = idx.hnsw_dense_rows(0)[1] - r0          # (and back to the rule)
    return out + (rej, four)


def _all_settings(eng, idx, tune, search, tag):
    """No table (mode 0), then the table with two and with four rows in flight, on one handle: everything equal."""
    i0, d0, s0, rej0, four0 = _launch(eng, idx, tune, search, 0, 4, tag + ", no table")
    assert four0 == 0 and rej0[1] > 0, tag
    try:
        for rows in (2, 4):
            what = "%s, %d rows in flight" % (tag, rows)
            ids, d, st, rej, four = _launch(eng, idx, tune, search, 2, rows, what)
            assert (four > 0) == (rows == 4), "%s: %d launches of the four-row instance" % (what, four)
            np.testing.assert_array_equal(st, s0, err_msg=what + ": counters")
            assert_exact(ids, d, i0, d0, what)
            assert rej == rej0, "%s: (f32 rows, neighbours) %s, %s without the table" % (what, rej, rej0)
    finally:
        idx.set_hnsw_dense_bounds(1)
    return i0, d0, s0, rej0


# ---- four rows against two against no table

@pytest.mark.parametrize("ef", EFS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", DIMS)
def test_rows_in_flight_do_not_change_the_search(eng, indexes, data, tune, dim, metric, ef):
    idx, Qs = indexes(dim, metric), data[dim][1]
    _wave(tune)
    for nq in NQS:
        tag = "dim %d %s ef %d nq %d" % (dim, metric, ef, nq)
        ids, d, st, _ = _all_settings(eng, idx, tune, lambda: _dev_search(idx, Qs[:nq], K, ef), tag)
        assert (ids != SENT_ID).all() and (d != SENT_D).all() and (st != SENT_ST).all(), tag + ": a query was not answered"


@pytest.mark.parametrize("vis_global", (0, 1))
@pytest.mark.parametrize("order", (0, 2))
def test_both_visited_sets_ordered_and_persistent(eng, indexes, data, tune, vis_global, order):
    """The LDS bitset and the HBM stamps (whose persistent grid, 3,072 workgroups at this n, strides over 4,000 slots), queries in
    their own order and dealt by pivot row (slots and queries differ: the table is indexed by the query)."""
    idx, Q = indexes(768, "cosine"), data[768][1]
    _wave(tune)
    tune.set("VIS_GLOBAL", vis_global)
    tune.set("HNSW_ORDER", order)
    o0 = eng.debug_counter("hnsw_ordered")
    ids, d, st, _ = _all_settings(eng, idx, tune, lambda: _dev_search(idx, Q, K, 64), "stamps %d order %d" % (vis_global, order))
    assert (eng.debug_counter("hnsw_ordered") - o0 == 3) == (order == 2)
    assert (ids != SENT_ID).all() and (st > 0).all()


# ---- the hops' needs, restated

def _layer_lists(g, level):
    """[n, slots] adjacency of one layer of a Graph (-1: no edge, or a node that does not reach the layer)."""
    if level == 0:
        return g.l0_adj.reshape(g.n, -1)
    adj = np.full((g.n, g.M), -1, np.int32)
    up = g.up_adj.reshape(-1, g.M)
    for u in np.flatnonzero(g.levels >= level):
        adj[u] = up[g.up_off[u] + level - 1]
    return adj


def need_trace(dist, lb, layers, entry, ef):
    """search-layer-ultra (ultra_fast.clj:151-212; scripted_graphs.trace) of one query down every layer, with the rejection test:
    an expansion of a FULL list fetches the f32 row of a fresh neighbour only if its bound is not >= the worst the expansion found
    (a NaN bound abstains), every other fresh neighbour counts as +inf.  Returns (rows needed by every layer-0 expansion, rows
    needed on all layers)."""
    total, needs = 0, []
    for level in range(len(layers) - 1, -1, -1):
        ef_l = ef if level == 0 else 1
        seq = 0
        nearest = [(float(dist[entry]), seq, int(entry))]
        cand = list(nearest)
        visited = {int(entry)}
        needs = []
        while cand:
            d, _, node = cand.pop(0)
            full = len(nearest) >= ef_l
            worst0 = nearest[-1][0]
            if full and not d <= worst0:
                break
            fresh = []
            for nb in layers[level][node]:
                nb = int(nb)
                if nb >= 0 and nb not in visited:
                    visited.add(nb)
                    fresh.append(nb)
            need = 0
            for nb in fresh:
                fetched = not full or not float(lb[nb]) >= worst0
                need += fetched
                dn = float(dist[nb]) if fetched else float("inf")
                if len(nearest) < ef_l or dn < nearest[-1][0]:
                    seq += 1
                    bisect.insort(nearest, (dn, seq, nb))
                    bisect.insort(cand, (dn, seq, nb))
                    if len(nearest) > ef_l:
                        nearest.pop()
            needs.append(need)
        total += sum(needs)
        entry = nearest[0][2]
    return needs, total


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", DIMS)
def test_the_searched_hops_need_every_count_of_rows(eng, oracle, indexes, data, tune, dim, metric):
    """The first 33 queries at ef 16, 64 and 640, restated on the CPU from the handle's graph, the oracle's device-order distances
    and the table's bounds: the restatement fetches exactly the rows the device counts (four rows in flight), and its layer-0
    expansions need 1, 2, 3, 4, 5, 8, 9 and more rows, every remainder modulo 4 among them."""
    O = oracle
    idx, (base, Qs) = indexes(dim, metric), data[dim]
    Q = Qs[:NTRACE]
    g = idx.get_graph()
    layers = [_layer_lists(g, level) for level in range(g.max_level + 1)]
    ids, dd, _ = O.exact_knn(base, Q, N, metric=O.METRICS[metric], mode=O.MODE_DEV)
    dist = np.empty_like(dd)
    np.put_along_axis(dist, ids.astype(np.int64), dd, axis=1)
    lb = idx.hnsw_dense_bounds(Q)
    _wave(tune)
    seen = set()
    for ef in EFS:
        needs, total = [], 0
        for q in range(NTRACE):
            nd, t = need_trace(dist[q], lb[q], layers, g.entry, ef)
            needs += nd
            total += t
        tag = "dim %d %s ef %d" % (dim, metric, ef)
        try:
            _, _, _, rej, four = _launch(eng, idx, tune, lambda: _dev_search(idx, Q, K, ef), 2, 4, tag)
        finally:
            idx.set_hnsw_dense_bounds(1)
        assert four == 1 and rej[0] == total, "%s: the device fetched %d f32 rows, the restatement %d" % (tag, rej[0], total)
        seen |= set(needs)
        if ef == 640:
            assert {n % 4 for n in needs if n} == {0, 1, 2, 3}, tag
            assert {1, 2, 3, 4, 5, 8, 9} <= set(needs) and max(needs) > 9, "%s: needs %s" % (tag, sorted(set(needs)))
    assert {1, 2, 3, 4, 5} <= seen


# ---- the scripted graphs, rows of dim 768

SCRIPTED = [c for c, what in sg.scenarios() if what in ("full", "tie", "split")] + \
           [sg.funnel(seed, 640, (0.0, 0.02)[seed % 2], (0.0, 0.3, 0.6)[seed % 3]) for seed in (0, 1, 2, 5)]


@pytest.mark.parametrize("case", range(len(SCRIPTED)), ids=[c.name for c in SCRIPTED])
def test_scripted_graphs_through_the_dense_instances(eng, oracle, tune, case):
    """The fan-out of 64 into a full list, the evicted entry that ties the worst, the split eviction and the funnels
    (tests/scripted_graphs.py) with rows of dim 768, two and four rows in flight, against the oracle's device-order search and,
    for the scripted query, the module's own restatement (trace)."""
    O = oracle
    case = SCRIPTED[case]
    metric = sg.METRICS[len(case.values) % 3]
    rows, Q = sg.queries(case, metric, 768)
    g = sg.graph(O, case)
    dist = sg.dev_distances(O, metric, Q[0], rows)
    _wave(tune)
    with eng.Index(rows, metric) as idx:
        idx.set_rejection_test(2)
        idx.set_graph(g)
        idx.set_profiling(True)
        for ef in case.efs:
            k = sg.result_k(ef)
            tag = "%s %s ef %d" % (case.name, metric, ef)
            oi, od, ost = O.hnsw_search(rows, g, Q, k, ef=ef, metric=O.METRICS[metric], mode=O.MODE_DEV)[:3]
            tr = sg.trace(dist, case.l0, case.entry, ef, k)
            ids, d, st, _ = _all_settings(eng, idx, tune, lambda: _dev_search(idx, Q, k, ef), tag)
            np.testing.assert_array_equal(st, ost, err_msg=tag + ": counters against the oracle")
            assert_exact(ids, d, oi, od, tag + " against the oracle")
            np.testing.assert_array_equal(ids[0], tr.ids, err_msg=tag + ": ids against the restatement")
            assert (tr.evals, tr.hops) == tuple(int(x) for x in st[0]), tag + ": counters against the restatement"


# ---- the rule

def _wave_lds_bytes(ef, n):
    """hnsw.hip: wave_lds_bytes of a first pass at this ef over n rows, visited set in LDS."""
    return 8 * (ef + K_GHOST) + 8 * 64 + 2 * 4 * MAX_DEG + 4 * ((n + 31) // 32) + 16


@pytest.mark.parametrize("ef", (640, 1600))
def test_the_rule_takes_four_rows_from_its_lds_threshold(eng, indexes, data, tune, ef):
    """Setting 0 (hnsw_launch_plan: kDenseRows4Lds): four rows in flight from 7,680 B of LDS per workgroup, where fewer workgroups fit a
    CU than the two-row instance's registers admit anyway, two below.  2,000 rows: 6,668 B at ef 640 (24 workgroups per CU: two
    rows), 14,348 B at ef 1600 (11: four).  The 31,173-row index of the benchmark is at 10,316 B at ef 640: four."""
    idx, Q = indexes(768, "l2"), data[768][1][:33]
    _wave(tune)
    assert _wave_lds_bytes(640, N) == 6668 and _wave_lds_bytes(1600, N) == 14348 and _wave_lds_bytes(640, 31173) == 10316
    try:
        _, _, _, _, four = _launch(eng, idx, tune, lambda: _dev_search(idx, Q, K, ef), 2, 0, "the rule at ef %d" % ef)
    finally:
        idx.set_hnsw_dense_bounds(1)
    assert four == (1 if _wave_lds_bytes(ef, N) > DENSE_ROWS4_LDS else 0)
