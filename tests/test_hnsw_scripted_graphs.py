"""Scripted graphs through every HNSW traversal kernel (tests/scripted_graphs.py has the graphs and says which state of the
candidate list each one reaches; tests/test_scripted_graph_traces.py proves on the CPU that it does).

The wave kernel and the several-CU kernel keep the list as main list + admission buffer + 64-entry tail window (ONE
implementation, hnsw_list.hpp: HnswList, with and without the mirror the several-CU kernel's fetchers read), the
single-workgroup kernel and the round-2 helper kernel merge by position: each runs scenario S (a full fan-out of 64 fresh
neighbours that are all admitted and push 64 main entries out -- the tail window is empty afterwards -- followed by a stop that
depends on the right worst), its ef variants, S-tie, S-tie-many (64 evicted entries that all tie the worst, twice the ghost
slots: such queries are repeated with a larger list), S-split (survivors partly refused, partly admitted and evicted again),
S-small (a fan-out wider than the list) and 24 funnel graphs at six efs around the 64-entry window, in l2, cosine and dot, with
rows of 8 and of 768 floats.  Ids, distance BITS and
both counters equal the oracle's device-order search; no tolerance is involved.  One Index and one set_graph per graph."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scripted_graphs as sg  # noqa: E402
from util import assert_exact  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTERS = ("hnsw_wave", "hnsw_solo", "hnsw_helpers")
SCENARIOS = sg.scenarios()


@pytest.fixture(scope="module")
def eng(native_lib):
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    t0 = time.time()
    yield engine
    print("\nscripted graphs: %.1f s for the module" % (time.time() - t0))


def _every_kernel(eng, O, tune, case, metric, dim):
    code = {"l2": O.L2, "cosine": O.COSINE, "dot": O.DOT}[metric]
    rows, Q = sg.queries(case, metric, dim)       # 127 times the scripted query, then three rows of the graph
    g = sg.graph(O, case)
    want = {ef: O.hnsw_search(rows, g, Q, sg.result_k(ef), ef=ef, metric=code, mode=O.MODE_DEV)[:3] for ef in case.efs}

    def run(idx, what, lo, hi, advances):
        for ef in case.efs:
            oi, od, ost = want[ef]
            before = [eng.debug_counter(c) for c in COUNTERS]
            ids, d, st = idx.hnsw_search(Q[lo:hi], sg.result_k(ef), ef, want_stats=True)
            moved = {c for c, b in zip(COUNTERS, before) if eng.debug_counter(c) > b}
            tag = "%s %s dim %d ef %d, %s, queries %d..%d" % (case.name, metric, dim, ef, what, lo, hi)
            assert moved == advances, "%s: launch counters that advanced: %s" % (tag, sorted(moved))
            tag += " (evals, hops of the first query: %s, the oracle's %s)" % (st[0].tolist(), ost[lo].tolist())
            np.testing.assert_array_equal(st, ost[lo:hi], err_msg=tag + ": counters")
            assert_exact(ids, d, oi[lo:hi], od[lo:hi], tag)

    with eng.Index(rows, metric) as idx:
        idx.set_graph(g)
        # large launches (130 queries): the wave kernel, then the single-workgroup kernel with 1, 2 and 4 waves; visited set in LDS
        # and in HBM stamps; the int8 rejection test on every launch and off
        for vis_global in (0, 1):
            tune.set("VIS_GLOBAL", vis_global)
            for mode in (2, 0):
                idx.set_rejection_test(mode)
                tune.set("HNSW_WAVE", 2)
                tune.unset("HNSW_NW")
                run(idx, "wave kernel, stamps %d, rejection %d" % (vis_global, mode), 0, 130, {"hnsw_wave"})
                tune.set("HNSW_WAVE", 0)
                for nw in (1, 2, 4):
                    tune.set("HNSW_NW", nw)
                    run(idx, "single-workgroup kernel, %d waves, stamps %d, rejection %d" % (nw, vis_global, mode), 0, 130, set())
        # small launches (1 and 20 queries; they switch the rejection test off themselves): one query over several CUs, then the
        # round-2 helper kernel
        tune.set("VIS_GLOBAL", 0)
        tune.unset("HNSW_NW")
        tune.unset("HNSW_WAVE")
        idx.set_rejection_test(2)
        for solo, what, counter in ((2, "several-CU kernel", "hnsw_solo"), (0, "round-2 helper kernel", "hnsw_helpers")):
            tune.set("SOLO", solo)
            run(idx, what, 0, 1, {counter})
            run(idx, what, 110, 130, {counter})       # 17 times the scripted query and the three rows


@pytest.mark.parametrize("dim", sg.DIMS)
@pytest.mark.parametrize("metric", sg.METRICS)
@pytest.mark.parametrize("scenario", range(len(SCENARIOS)), ids=[c.name for c, _ in SCENARIOS])
def test_scripted_scenarios(eng, oracle, tune, scenario, metric, dim):
    _every_kernel(eng, oracle, tune, SCENARIOS[scenario][0], metric, dim)


@pytest.mark.parametrize("seed", sg.FUNNEL_SEEDS)
def test_funnel_graphs(eng, oracle, tune, seed):
    """Shells of 64 that pour into each other: a full fan-out per shell, with ties (0, 30 %, 60 % duplicated values) and a few
    re-pointed slots, at ef 10, 64, 65, 80, 128 and 333."""
    case, metric, dim = sg.funnel_case(seed)
    _every_kernel(eng, oracle, tune, case, metric, dim)
