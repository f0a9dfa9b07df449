"""The batched HNSW builder (hnswgpu_hnsw_build_ex without SEQUENTIAL, the builder production uses) and hnswgpu_hnsw_add
against the batched restatement in the oracle (oracle.c: orc_hnsw_build_batched), EDGE FOR EDGE: levels, entry point, top,
up_off and both adjacency arrays in row order.  The batched build is a deterministic function of rows, metric, M,
ef_construction, seed, flags and BUILD_BATCH, so nothing here has a tolerance.  The data sets and the conditions they meet
(lists that overflow, tasks with several pending edges, effective symmetric removals, entry changes inside a batch, threaded
linking) are stated in hnsw_build_model.py and asserted on the CPU by test_hnsw_build_model_host.py."""
import numpy as np
import pytest

import hnsw_build_model as H
from util import assert_exact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(native_lib):
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    return engine


@pytest.fixture(scope="module")
def main_base(oracle):
    return H.main_data(oracle)


@pytest.fixture(scope="module")
def add_bases(oracle):
    return {dim: H.add_data(oracle, dim) for dim in sorted({d for d, _ in H.ADD_CASES})}


def _set_batch(tune, B):
    if B != H.DEFAULT_MAX_BATCH:
        tune.set("BUILD_BATCH", B)


def _search_equals_oracle(O, idx, base, g, code, what, ef=60):
    Q = O.generate_dataset(16, base.shape[1], seed=43).astype(np.float32)
    ids, d, st = idx.hnsw_search(Q, 10, ef, want_stats=True)
    oi, od, ost, _ = O.hnsw_search(base, g, Q, 10, ef=ef, metric=code, mode=O.MODE_DEV)
    assert_exact(ids, d, oi, od, "search on the graph of " + what)
    np.testing.assert_array_equal(st, ost, err_msg=what)


@pytest.mark.parametrize("B", H.MAIN_BATCHES)
@pytest.mark.parametrize("flags", H.MAIN_FLAGS)
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_batched_build_equals_the_model(eng, oracle, tune, main_base, metric, flags, B):
    """3000 x 48 clustered rows with duplicated pairs and a zero row, M 8, ef_construction 40: the exported graph equals the
    model run with the engine's batch sizes for BUILD_BATCH = 1, 7, 64 and the default.  One row per batch, closest-m, is
    also the sequential restatement with the batched walk (BUILD_DESCEND)."""
    O = oracle
    code, P, n = O.METRICS[metric], H.MAIN, len(main_base)
    what = "batched %s build, %s, BUILD_BATCH %d" % (flags, metric, B)
    _set_batch(tune, B)
    with eng.Index(main_base, metric) as idx:
        idx.hnsw_build(P["M"], P["efc"], P["seed"], **H.flag_kwargs(flags))
        g = idx.get_graph()
        og, _ = O.hnsw_build_batched(main_base, H.batch_schedule(n, 1, B), code, P["M"], P["efc"], P["seed"], H.flag_bits(O, flags),
                                     O.MODE_DEV)
        H.same_graph(g, og, what)
        if B == 1 and flags == "closest":
            sg = O.hnsw_build_ex(main_base, code, P["M"], P["efc"], P["seed"], O.BUILD_DESCEND, mode=O.MODE_DEV)
            H.same_graph(g, sg, what + " vs the sequential restatement")
        _search_equals_oracle(O, idx, main_base, og, code, what)


@pytest.mark.parametrize("flags", ["closest", "heuristic+symmetric"])
def test_large_batched_build_equals_the_model_for_any_thread_count(eng, oracle, tune, flags):
    """24,000 x 16: batches of 256 and more (linked by the pool's threads: own lists by row range, reverse edges by target
    mod T), more than 1024 selection tasks in one batch (gathered and applied by the threads), and the batches sized by
    2048 + done / 64 (the host test asserts all three from the schedule and the model's counters).  BUILD_THREADS 1 and 5
    both give the model's graph."""
    O = oracle
    base, P = H.large_data(O), H.LARGE
    og, _ = O.hnsw_build_batched(base, H.batch_schedule(len(base), 1), O.COSINE, P["M"], P["efc"], P["seed"], H.flag_bits(O, flags),
                                 O.MODE_DEV)
    with eng.Index(base, "cosine") as idx:
        for nt in (1, 5):
            tune.set("BUILD_THREADS", nt)
            idx.hnsw_build(P["M"], P["efc"], P["seed"], **H.flag_kwargs(flags))
            H.same_graph(idx.get_graph(), og, "24,000-row %s build, %d linker threads" % (flags, nt))
        _search_equals_oracle(O, idx, base, og, O.COSINE, "the 24,000-row %s build" % flags)


@pytest.mark.parametrize("start", ["closest", "heuristic+symmetric", "installed"])
@pytest.mark.parametrize("dim,metric", H.ADD_CASES)
def test_hnsw_add_equals_the_model_continuing_from_the_installed_graph(eng, oracle, add_bases, dim, metric, start):
    """2000 rows, then 1, 1, 5, 300 and 693 more in separate calls: after every call the export equals the model started on
    the previous export with the batch sizes of a graph that already holds those rows.  `installed`: the 2000-row graph
    comes through hnswgpu_set_graph from the sequential restatement -- full lists partly in insertion order, distances the
    handle never stored (edge_dist_kernel recomputes them, `adopt` decides which lists count as sorted) and no builder, so
    the added rows link closest-m."""
    O = oracle
    base, A, code = add_bases[dim], H.ADD, O.METRICS[metric]
    n0 = A["n0"]
    with eng.Index(base[:n0], metric) as idx:
        if start == "installed":
            idx.set_graph(O.hnsw_build_ex(base[:n0], code, A["M"], A["efc"], A["seed"], 0, mode=O.MODE_DEV))
            f = 0
        else:
            idx.hnsw_build(A["M"], A["efc"], A["seed"], **H.flag_kwargs(start))
            f = H.flag_bits(O, start)
        g, pos = idx.get_graph(), n0
        for m in A["calls"]:
            ids = idx.hnsw_add(base[pos:pos + m], A["efc"], A["seed"])
            assert ids[0] == pos and len(ids) == m
            og, _ = O.hnsw_build_batched(base[:pos + m], H.batch_schedule(pos + m, pos), code, A["M"], A["efc"], A["seed"], f,
                                         O.MODE_DEV, start=g)
            g = idx.get_graph()
            H.same_graph(g, og, "%s graph of %d rows + %d, dim %d %s" % (start, pos, m, dim, metric))
            pos += m
        _search_equals_oracle(O, idx, base, g, code, "the grown %s graph, dim %d %s" % (start, dim, metric))


@pytest.mark.parametrize("flags", ["closest", "heuristic", "heuristic+symmetric"])
def test_add_at_a_batch_boundary_equals_build(eng, oracle, tune, main_base, flags):
    """Where a build's batch ends, stopping, exporting nothing and adding the remaining rows in one call goes through the
    same batches against the same graph: build(n0) + add(rest) equals build(n1) array for array.  No oracle involved."""
    n1, P = 2400, H.MAIN
    base = main_base[:n1]
    _set_batch(tune, 64)
    sched = H.batch_schedule(n1, 1, 64)
    cut = len(sched) * 2 // 3
    n0 = 1 + sum(sched[:cut])
    assert H.batch_schedule(n1, n0, 64) == sched[cut:] and n1 - n0 > 256
    with eng.Index(base, "cosine") as whole, eng.Index(base[:n0], "cosine") as part:
        whole.hnsw_build(P["M"], P["efc"], P["seed"], **H.flag_kwargs(flags))
        part.hnsw_build(P["M"], P["efc"], P["seed"], **H.flag_kwargs(flags))
        part.hnsw_add(base[n0:], P["efc"], P["seed"])
        H.same_graph(part.get_graph(), whole.get_graph(), "build(%d) + add(%d) against build(%d), %s" % (n0, n1 - n0, n1, flags))


@pytest.mark.parametrize("flags", ["closest", "heuristic"])
def test_build_with_hundreds_of_copies_of_one_row(eng, oracle, flags):
    """300 copies of one row among 1500.  A build search has no repeat pass, so a search that meets more candidates tied with
    its ef-th than the 32 ghost slots hold may link differently from the model: no comparison with it here.  The
    graph must still be a graph -- the validator accepts the export, every row has a layer-0 edge -- and searching it on the
    device (search does have the repeat pass) equals the oracle's search of the export: ids, distance bits, counters."""
    O = oracle
    base = H.clustered(O, 1500, 32, clusters=8, noise=0.4, seed=31)
    base[np.arange(300) * 5 + 2] = base[7]
    with eng.Index(base, "cosine") as idx:
        idx.hnsw_build(8, 40, 42, **H.flag_kwargs(flags))
        g = idx.get_graph()
        assert ((g.l0_adj.reshape(len(base), -1) >= 0).sum(1) >= 1).all()
        assert g.levels[g.entry] == g.max_level
        with eng.Index(base, "cosine") as chk:
            chk.set_graph(g)
        Q = np.vstack([base[7:8], base[:3], O.generate_dataset(12, 32, seed=43).astype(np.float32)])
        ids, d, st = idx.hnsw_search(Q, 10, 60, want_stats=True)
        oi, od, ost, _ = O.hnsw_search(base, g, Q, 10, ef=60, metric=O.COSINE, mode=O.MODE_DEV)
        assert_exact(ids, d, oi, od, "search of the %s graph with 300 copies" % flags)
        np.testing.assert_array_equal(st, ost)
