"""The scripted graphs of tests/scripted_graphs.py, on the CPU: the restated reference loop (`trace`) equals the oracle on every
case the GPU module runs, and its event log shows that every case reaches the candidate-list state it exists for -- so that
no GPU test can pass by missing its state.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scripted_graphs as sg  # noqa: E402


def _run(O, case, metric, dim):
    """ef -> Trace of the scripted query, after comparing it with the oracle's device-order search."""
    code = {"l2": O.L2, "cosine": O.COSINE, "dot": O.DOT}[metric]
    rows, Q = sg.queries(case, metric, dim)
    dist = sg.dev_distances(O, metric, Q[0], rows)
    sg.check_embedding(case.values, dist)
    g = sg.graph(O, case)
    out = {}
    for ef in case.efs:
        k = sg.result_k(ef)
        tr = sg.trace(dist, case.l0, case.entry, ef, k)
        oi, od, ost, _ = O.hnsw_search(rows, g, Q[:1], k, ef=ef, metric=code, mode=O.MODE_DEV)
        what = "%s %s dim %d ef %d" % (case.name, metric, dim, ef)
        np.testing.assert_array_equal(tr.ids, oi[0], err_msg=what + ": ids")
        assert (tr.evals, tr.hops) == tuple(int(x) for x in ost[0]), what + ": evals, hops"
        found = tr.ids[tr.ids >= 0]
        np.testing.assert_array_equal(od[0][:len(found)], dist[found], err_msg=what + ": distances")
        out[ef] = tr
    return out


@pytest.fixture(scope="module")
def scenario_traces(oracle):
    """(case, kind, metric, dim) -> {ef: Trace}: every scripted scenario in every metric and both row widths."""
    return {(case.name, kind, metric, dim): (case, _run(oracle, case, metric, dim))
            for case, kind in sg.scenarios() for metric in sg.METRICS for dim in sg.DIMS}


@pytest.fixture(scope="module")
def funnel_traces(oracle):
    """(seed, ef) -> Trace for the funnel cases of the GPU module (its seeds, its efs, its metric and width per seed)."""
    out = {}
    for seed in sg.FUNNEL_SEEDS:
        case, metric, dim = sg.funnel_case(seed)
        for ef, tr in _run(oracle, case, metric, dim).items():
            out[(seed, ef)] = tr
    return out


def test_trace_equals_oracle(scenario_traces, funnel_traces):
    """(the fixtures compare ids, distances and both counters with oracle.hnsw_search in MODE_DEV as they build)"""
    assert len(scenario_traces) == len(sg.scenarios()) * len(sg.METRICS) * len(sg.DIMS)
    assert len(funnel_traces) == len(sg.FUNNEL_SEEDS) * len(sg.FUNNEL_EFS)


def test_scenario_s_numbers(scenario_traces):
    """Scenario S at ef 80, the figures the layout was written for: 1 + 64 + 17 + 64 evaluations; E, G, H, 64 N's and
    A0..A14 expanded."""
    for (name, kind, metric, dim), (case, traces) in scenario_traces.items():
        if name == "S-plain-ef80":
            assert (traces[80].evals, traces[80].hops) == (146, 82), (metric, dim)


def _kinds(scenario_traces, kind):
    got = [(key, case, traces) for key, (case, traces) in scenario_traces.items() if key[1] == kind]
    assert got
    return got


def test_full_fanout_then_stop_at_a_non_tied_candidate(scenario_traces):
    """S and every ef variant: exactly ONE expansion with a full list, 64 fresh, 64 admitted, 64 older entries pushed out --
    H's --, and later the stop at A[a-1], strictly beyond the worst, with Y never evaluated."""
    for key, case, traces in _kinds(scenario_traces, "full"):
        (ef, tr), = traces.items()
        assert ef >= 65
        full = [i for i, e in enumerate(tr.events) if sg.is_full_fanout(e)]
        assert len(full) == 1 and tr.events[full[0]].node == case.roles["H"], key
        assert len(tr.events) > full[0] + 1, key                              # the stop comes later
        assert tr.stop is not None and tr.stop[0] == case.roles["last_A"] and tr.stop[1] > tr.stop[2], key
        assert case.roles["Y"] not in tr.ids and not any(e.on_tie for e in tr.events), key
        n_seen = 1 + sum(e.n_fresh for e in tr.events)
        assert tr.evals == n_seen == len(case.values) - 1, key                # every node but Y


def test_tie_expansion(scenario_traces):
    """S-tie: the full fan-out, then A[a-1] -- pushed out, but tied with the worst -- IS expanded and Y enters the result.
    S-tie-many: all 64 entries that left tie the worst; every one of them is expanded."""
    for key, case, traces in _kinds(scenario_traces, "tie") + _kinds(scenario_traces, "tie-many"):
        (ef, tr), = traces.items()
        assert sum(sg.is_full_fanout(e) for e in tr.events) == 1, key
        ties = [e for e in tr.events if e.on_tie]
        assert case.roles["last_A"] in [e.node for e in ties], key
        assert len(ties) == (64 if key[1] == "tie-many" else 1), key
        assert case.roles["Y"] in tr.ids, key


def test_split_expansion(scenario_traces):
    """S-split: ONE expansion whose 64 fresh neighbours are all below the worst it found, and of which some are refused
    (the worst has shrunk by their turn, ten of them tie it) and some are admitted and pushed out again."""
    for key, case, traces in _kinds(scenario_traces, "split"):
        tr = traces[80]
        e, = [e for e in tr.events if e.node == case.roles["H"]]
        assert e.list_full and e.n_fresh == 64 and e.n_survivors == 64, key
        assert e.n_admitted == 34 and e.n_admitted_then_evicted == 10 and e.n_evicted_old == 24, key


def test_fanout_wider_than_the_list(scenario_traces):
    """S-small: 64 fresh neighbours meet a FULL list of 1, 10 and 64 entries, and every one of them is admitted: what the
    list cannot hold leaves it again within the same expansion."""
    for key, case, traces in _kinds(scenario_traces, "small"):
        assert sorted(traces) == [1, 10, 64]
        for ef, tr in traces.items():
            e, = [e for e in tr.events if e.node == case.roles["H"]]
            assert e.list_full and e.n_fresh == e.n_survivors == e.n_admitted == 64, (key, ef)
            assert (e.n_evicted_old, e.n_admitted_then_evicted) == (ef, 64 - ef), (key, ef)


def test_funnel_coverage(funnel_traces):
    """Over the funnel cases the GPU module runs: at least a third contain a full 64 / 64 / 64 expansion on a list of ef >= 65
    (the state in which evictions empty the tail window), and each further class occurs."""
    n = len(funnel_traces)
    full = sum(1 for (seed, ef), tr in funnel_traces.items() if ef >= 65 and any(sg.is_full_fanout(e) for e in tr.events))
    assert 3 * full >= n, "%d of %d funnel cases reach the full fan-out: fix the generator, not this bound" % (full, n)
    events = [(ef, e) for (seed, ef), tr in funnel_traces.items() for e in tr.events]
    assert any(ef < 64 and e.list_full and e.n_fresh == 64 and e.n_admitted >= 2 for ef, e in events), "full fan-out at ef < 64"
    assert any(e.boundary_tie for ef, e in events), "a multi-admit with ties at the eviction boundary"
    assert any(e.list_full and e.n_survivors == 1 and e.n_admitted == 1 for ef, e in events), "one survivor on a full list"
    assert any(e.on_tie for ef, e in events), "a candidate expanded on a tie after it had left the list"
