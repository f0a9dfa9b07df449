"""hnswgpu_hnsw_update at every loader width of test_mutation_widths_gpu.py (rejection mode 2 at every dim, mode 1 at 127 and 128):
calls of 1 and 65 rows on 400 rows (M 8, ef_construction 40, the builder by BUILDER_OF), the graph against hnsw_update_model after
each, then the handle against a fresh one -- every search, the norms, the file, and what no search at this size shows: the
base-order int8 rows read directly (mutation_checks.same_base_codes), the traversal's own bounds, the counted traversals
(mutation_checks.same_hnsw_searches under COUNTED_TRAVERSAL) and the plain float64 reference (mutation_checks.matches_f64)."""
import numpy as np
import pytest

import hnsw_build_model as H
import hnsw_update_model as U
import mutation_checks as C
import test_hnsw_remove_gpu as THR
import test_mutation_widths_gpu as W

CASES = [(dim, 2) for dim in W.DIMS] + [(dim, 1) for dim in (127, 128)]
METRIC_OF = {dim: W.METRICS[(j + 1) % 3] for j, dim in enumerate(W.DIMS)}


def test_every_metric_every_width_and_both_builders_are_met():
    assert {METRIC_OF[d] for d in W.DIMS} == set(W.METRICS)
    assert {W._pick_nch(d) for d, _ in CASES} == set(W.WIDTHS)
    assert {W.BUILDER_OF[d] for d, _ in CASES} == {"closest", "heuristic"}
    assert W.CALLS == (1, 65)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,mode", CASES, ids=["dim%d-mode%d" % c for c in CASES])
def test_hnsw_update_at_every_row_width(native_lib, oracle, tmp_path, dim, mode):
    from hnsw_clj_amd import engine

    O = oracle
    metric = METRIC_OF[dim]
    rows, Q = W._data(O, dim)
    base, spare = rows[:W.NH], rows[W.N0:]
    code, heuristic = O.METRICS[metric], W.BUILDER_OF[dim] == "heuristic"
    flags = O.BUILD_HEURISTIC if heuristic else 0
    rng = np.random.default_rng(4000 + dim)
    Qh = np.ascontiguousarray(Q[:32])
    with engine.Index(base, metric, 0) as ix:
        ix.set_rejection_test(mode)
        ix.hnsw_build(W.HM, W.HEFC, W.SEED, heuristic=heuristic)
        g, cur, at = ix.get_graph(), base.copy(), 0
        C.touch(ix, Q)
        for m in W.CALLS:
            ids = rng.choice(W.NH, m, replace=False).astype(np.int32)
            new = spare[at:at + m].copy()                    # rows of other clusters
            new[::3] = cur[ids[::3]] * np.float32(1.01)      # ... and scaled old values: the directions stay, the int8 rows do not
            at += m
            cur = cur.copy()
            cur[ids] = new
            g, _ = U.update(O, cur, code, g, ids, W.HEFC, flags)
            ix.hnsw_update(ids, new, W.HEFC)
            H.same_graph(ix.get_graph(), g, "after updating %d" % m)
        with THR._fresh(engine, cur, metric, mode, g) as fresh:
            THR._assert_same_answers(ix, fresh, Qh, mode)
            copies = W._has_copies(mode, dim)
            row = cur[len(cur) // 2]
            C.same_base_codes(ix, fresh, Q, row, expect=copies)
            if copies:
                C.same_graph_codes(ix, fresh, Q, row)
            C.same_hnsw_searches(ix, fresh, Qh)
            C.matches_f64(ix, cur, metric, Q)
            if not heuristic:                                # (the file carries the builder: set_graph installs a graph without one)
                W._same_file(ix, fresh, tmp_path)
            ix.save(tmp_path / "updated.idx")
            with engine.Index.load(tmp_path / "updated.idx", 0) as back:
                H.same_graph(back.get_graph(), g, "loaded")
                np.testing.assert_array_equal(C.bits(back.norms()), C.bits(fresh.norms()), err_msg="norms of the loaded handle")
                C.same(back.hnsw_search(Qh, C.K, 64), fresh.hnsw_search(Qh, C.K, 64), "loaded")
