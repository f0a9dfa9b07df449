"""hnswgpu_lsh_update at every loader width of test_mutation_widths_gpu.py (rejection mode 2 at every dim, mode 1 at 127 and 128):
calls of 1 and 65 rows on 600 rows under 4 tables x 6 bits, then the handle against a fresh one -- the tables, every search, the
norms, the file, and what no search at this size shows: the base-order int8 rows read directly (mutation_checks.same_base_codes)
and the plain float64 reference (mutation_checks.matches_f64)."""
import numpy as np
import pytest

import lsh_update_model as U
import mutation_checks as C
import test_lsh_remove_gpu as TLR
import test_mutation_widths_gpu as W

CASES = [(dim, 2) for dim in W.DIMS] + [(dim, 1) for dim in (127, 128)]
METRIC_OF = {dim: W.METRICS[j % 3] for j, dim in enumerate(W.DIMS)}


def test_every_metric_and_every_width_is_met():
    assert {METRIC_OF[d] for d in W.DIMS} == set(W.METRICS)
    assert {W._pick_nch(d) for d, _ in CASES} == set(W.WIDTHS)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,mode", CASES, ids=["dim%d-mode%d" % c for c in CASES])
def test_lsh_update_at_every_row_width(native_lib, oracle, tmp_path, dim, mode):
    from hnsw_clj_amd import engine

    metric = METRIC_OF[dim]
    rows, Q = W._data(oracle, dim)
    base, spare = rows[:W.N0], rows[W.N0:]
    rng = np.random.default_rng(3000 + dim)
    configs = sorted({(min(p, W.TABLES), r, tm, tf) for p, r, tm, tf in TLR.CONFIGS})
    with engine.Index(base, metric, 0) as ix:
        ix.set_rejection_test(mode)
        ix.lsh_build(W.TABLES, W.BITS, 64, 42)
        planes, codes, boff, bids = ix.lsh_get()
        C.touch(ix, Q)
        cur, model, at = base.copy(), (codes, boff, bids), 0
        for m in W.CALLS:
            ids = rng.choice(W.N0, m, replace=False).astype(np.int32)
            new = spare[at:at + m].copy()                    # rows of other clusters: most codes change
            new[::3] = cur[ids[::3]] * np.float32(1.01)      # ... and scaled old values: the signs stay, the int8 rows do not
            at += m
            ix.lsh_update(ids, new)
            cur = U.apply(cur, ids, new)
            model = U.merge(*model, ids, ix.lsh_hash(new))
        with TLR._fresh(engine, cur, metric, planes, mode) as fresh:
            _, c1, o1, i1 = TLR._assert_same_tables(ix, fresh)   # (also against lsh_model.buckets, the numpy counting sort)
            for got, want, what in zip((c1, o1, i1), model, ("codes", "off", "ids")):
                np.testing.assert_array_equal(got, want, err_msg=what + " against the update model")
            assert (c1 != codes).any(), "no row moved"
            for cfg in configs:
                for nq in (1, TLR.NQ):
                    C.same(ix.lsh_search(Q[:nq], TLR.K, *cfg), fresh.lsh_search(Q[:nq], TLR.K, *cfg), "lsh_search %s nq %d" % (cfg, nq))
            C.same(ix.exact_knn(Q[:5], TLR.K), fresh.exact_knn(Q[:5], TLR.K), "exact_knn")
            np.testing.assert_array_equal(C.bits(ix.norms()), C.bits(fresh.norms()), err_msg="norms")
            W._same_file(ix, fresh, tmp_path)
            C.same_base_codes(ix, fresh, Q, cur[len(cur) // 2], expect=W._has_copies(mode, dim))
            C.matches_f64(ix, cur, metric, Q)
