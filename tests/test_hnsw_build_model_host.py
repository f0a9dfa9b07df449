"""The batched restatement of the HNSW builder (oracle.c: orc_hnsw_build_batched) on the CPU: it equals the sequential
restatement when every batch holds one row, gives hand-derived graphs on points of a line, continues from a start graph
as a build continues from its own batches, and the batch-size rule gives the values worked out by hand.  The data sets of
the GPU tests (test_hnsw_build_batched_gpu.py, test_hnsw_heuristic_paths_gpu.py) are checked here, from the model's
counters alone, for the conditions those tests rely on."""
import numpy as np
import pytest

import hnsw_build_model as H

LEVEL0_SEED = 200      # java.util.Random(200): the first eight rows all draw level 0


@pytest.fixture(scope="module")
def O(oracle):
    return oracle


def _l0(g):
    return g.l0_adj.reshape(g.n, -1).tolist()


# ---- batches of one: the sequential restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("flags", ["closest", "heuristic", "heuristic+extend"])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_batches_of_one_equal_the_sequential_restatement(O, metric, flags):
    """Every batch one row: nothing is deferred, so the model is orc_hnsw_build_ex with the batched build's walk
    (BUILD_DESCEND) edge for edge.  (SYMMETRIC is left out on purpose: the batched removals wait for the end of the batch's
    re-selections even in a batch of one row, the sequential ones do not.)"""
    base = H.main_data(O)[:1500]
    code, f = O.METRICS[metric], H.flag_bits(O, flags)
    g, cnt = O.hnsw_build_batched(base, [1] * (len(base) - 1), code, 8, 40, 42, f, O.MODE_DEV)
    og, ocnt = O.hnsw_build_ex(base, code, 8, 40, 42, f | O.BUILD_DESCEND, mode=O.MODE_DEV, want_counters=True)
    assert ocnt[3] > 100 and cnt[H.TASKS] > 100, "the data set must overflow lists: %s %s" % (ocnt, cnt)
    H.same_graph(g, og, "batches of one, %s %s" % (flags, metric))


# ---- graphs derived by hand ------------------------------------------------------------------------------------------
def _line(xs):
    return np.asarray(xs, np.float32).reshape(-1, 1)


def test_rows_of_one_batch_do_not_see_each_other(O):
    """Rows at 0, 10, 4, 6 on a line, l2, M = 1 (two links at layer 0), closest-m, every row on level 0.
    Batches [1, 2]: row 1 links to row 0.  Rows 2 and 3 are both searched against {0, 1}: row 2 (at 4) takes 0 (d 4), 1 (d 6);
    row 3 (at 6) takes 1 (d 4), 0 (d 6).  Linked in row order: list 0 = [1 (10), 2 (4)], list 1 = [0 (10), 2 (6)]; then row 3
    overflows both: list 1 = sort [0 (10), 2 (6), 3 (4)] -> [3, 2], list 0 = sort [1 (10), 2 (4), 3 (6)] -> [2, 3].  Rows 2 and 3,
    the closest pair of all, are not linked.
    Batches [1, 1, 1]: row 3 finds 2 (d 2), 1 (d 4), 0 (d 6) and takes [2, 1]; list 2 = sort [0 (4), 1 (6), 3 (2)] -> [3, 0],
    list 1 = sort [0 (10), 2 (6), 3 (4)] -> [3, 2], list 0 stays [1, 2]."""
    base = _line([0, 10, 4, 6])
    g, cnt = O.hnsw_build_batched(base, [1, 2], O.L2, 1, 4, LEVEL0_SEED, 0, O.MODE_DEV)
    assert g.levels.tolist() == [0, 0, 0, 0] and (g.entry, g.max_level) == (0, 0)
    assert _l0(g) == [[2, 3], [3, 2], [0, 1], [1, 0]]
    assert cnt[H.TASKS] == 2
    g, cnt = O.hnsw_build_batched(base, [1, 1, 1], O.L2, 1, 4, LEVEL0_SEED, 0, O.MODE_DEV)
    assert _l0(g) == [[1, 2], [3, 2], [3, 0], [2, 1]]
    assert cnt[H.TASKS] == 2


def test_a_symmetric_removal_waits_for_the_end_of_the_batch(O):
    """Rows T = 0, X = 10, L = -8, R = 18, then a = 4 and b = 13 in one batch; l2, M = 1, ef_construction 1 (a row links to the
    one row its greedy walk ends at), HEURISTIC + SYMMETRIC, every row on level 0, walks start at T.
    One by one: X links T; L links T (list T = [X, L], full); R's walk goes T -> X and links X (list X = [T, R], full).
    The batch: a's walk ends at T, b's at X (T -> X, R is not closer).  Own lists a = [T], b = [X]; both reverse edges are
    pending.  Task T: a (4), L (8), X (10) -> a; L (12 from a, not < 8) -> the list is [a, L]; X is not kept: X is to lose T.
    Task X: b (3), R (8), T (10) -> b; R is 5 from b (< 8): discarded; T is 13 from b (not < 10): kept -> the list is [b, T];
    R is to lose X.  Only now the removals: X = [b, T] loses T -> [b]; R = [X] loses X -> [].
    (Removed at once, T would have left X = [T, R] before X's own task: X would have had room for b and ended as [R, b].)"""
    base = _line([0, 10, -8, 18, 4, 13])
    f = O.BUILD_HEURISTIC | O.BUILD_SYMMETRIC
    g, cnt = O.hnsw_build_batched(base, [1, 1, 1, 2], O.L2, 1, 1, LEVEL0_SEED, f, O.MODE_DEV)
    assert g.levels.tolist() == [0] * 6 and (g.entry, g.max_level) == (0, 0)
    assert _l0(g) == [[4, 2], [5, -1], [0, -1], [-1, -1], [0, -1], [1, -1]]
    assert (cnt[H.TASKS], cnt[H.TASKS_2_PENDING], cnt[H.SYM_REMOVED]) == (2, 0, 2)
    # without SYMMETRIC the dropped edges stay on the other side
    g, cnt = O.hnsw_build_batched(base, [1, 1, 1, 2], O.L2, 1, 1, LEVEL0_SEED, O.BUILD_HEURISTIC, O.MODE_DEV)
    assert _l0(g) == [[4, 2], [5, 0], [0, -1], [1, -1], [0, -1], [1, -1]]
    assert cnt[H.SYM_REMOVED] == 0


def test_two_pending_edges_of_one_list_are_selected_together(O):
    """Rows 0, 10, -10 one by one (list 0 = [1, 2], full), then 3 (at 4) and 4 (at 2) in one batch; l2, M = 1, ef 1, HEURISTIC.
    Both walks end at row 0, both reverse edges are pending on list 0: one task with the candidates 4 (d 2), 3 (d 4), 1 (10),
    2 (10) -- the tie in id order.  4 is taken; 3 is 2 from 4 (< 4): discarded; 1 is 8 from 4 (< 10): discarded; 2 is 12 from 4:
    taken.  List 0 = [4, 2]."""
    base = _line([0, 10, -10, 4, 2])
    g, cnt = O.hnsw_build_batched(base, [1, 1, 2], O.L2, 1, 1, LEVEL0_SEED, O.BUILD_HEURISTIC, O.MODE_DEV)
    assert _l0(g) == [[4, 2], [0, -1], [0, -1], [0, -1], [0, -1]]
    assert (cnt[H.TASKS], cnt[H.TASKS_2_PENDING]) == (1, 1)


def test_entry_point_moves_after_the_batch(O):
    """Seed 42 draws the levels 0, 0, 1, 1, 0.  Batches [1, 3]: rows 2 and 3 both rise above the top (0) of the graph they
    are searched against, so neither gets a link on layer 1; behind the batch row 2 becomes the entry point, row 3 (not
    higher than row 2) does not.  One by one, row 3 meets the entry point 2 on layer 1 and the two are linked there."""
    base = _line([0, 10, 4, 6, 20])
    g, cnt = O.hnsw_build_batched(base, [1, 3], O.L2, 2, 8, 42, 0, O.MODE_DEV)
    assert g.levels.tolist() == [0, 0, 1, 1, 0] and g.up_off.tolist() == [0, 0, 0, 1, 2, 2]
    assert (g.entry, g.max_level) == (2, 1)
    assert (cnt[H.ABOVE_TOP], cnt[H.ENTRY_CHANGES], cnt[H.ENTRY_CHANGES_IN_BATCH]) == (2, 1, 1)
    assert g.up_adj.tolist() == [-1, -1, -1, -1]
    assert _l0(g) == [[1, 2, 3, 4], [0, 2, 3, 4], [0, 1, -1, -1], [1, 0, -1, -1], [1, 0, -1, -1]]
    g, cnt = O.hnsw_build_batched(base, [1, 1, 1, 1], O.L2, 2, 8, 42, 0, O.MODE_DEV)
    assert (g.entry, g.max_level) == (2, 1)
    assert (cnt[H.ABOVE_TOP], cnt[H.ENTRY_CHANGES], cnt[H.ENTRY_CHANGES_IN_BATCH]) == (1, 1, 0)
    assert g.up_adj.tolist() == [3, -1, 2, -1]


# ---- a start graph: hnswgpu_hnsw_add ---------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ["closest", "heuristic+symmetric"])
def test_continuing_at_a_batch_boundary_equals_the_build(O, flags):
    """The model started on its own export at a boundary of the schedule, with the rest of the schedule, ends where the
    build ends: adopting a graph (lists in their order, distances recomputed owner -> neighbour) loses nothing."""
    base = H.main_data(O)[:1200]
    f = H.flag_bits(O, flags)
    sched = H.batch_schedule(len(base), 1, 64)
    cut = len(sched) * 2 // 3
    n0 = 1 + sum(sched[:cut])
    assert H.batch_schedule(len(base), n0, 64) == sched[cut:]
    whole, _ = O.hnsw_build_batched(base, sched, O.COSINE, 8, 40, 42, f, O.MODE_DEV)
    part, _ = O.hnsw_build_batched(base[:n0], sched[:cut], O.COSINE, 8, 40, 42, f, O.MODE_DEV)
    grown, cnt = O.hnsw_build_batched(base, sched[cut:], O.COSINE, 8, 40, 42, f, O.MODE_DEV, start=part)
    assert cnt[H.ADOPTED_FIRST] > 50
    H.same_graph(grown, whole, "continued at row %d, %s" % (n0, flags))
    with pytest.raises(ValueError):
        O.hnsw_build_batched(base, sched[cut + 1:], O.COSINE, 8, 40, 42, f, O.MODE_DEV, start=part)


# ---- the batch-size rule ---------------------------------------------------------------------------------------------
def test_batch_schedule_values_by_hand():
    # n = 40: rows 1 .. 15 one by one (done // 8 == 0, then 1), from 16 rows two at a time, from 24 three, from 32 four
    assert H.batch_schedule(40, 1) == [1] * 15 + [2, 2, 2, 2, 3, 3, 3, 4, 3]
    assert H.batch_schedule(1, 1) == [] and H.batch_schedule(2, 1) == [1]
    # the 1/8 rule: never more than an eighth of the rows already in
    done = 1
    for b in H.batch_schedule(30000, 1):
        assert 1 <= b <= max(1, done // 8)
        done += b
    assert done == 30000
    # 2048 + done // 64 takes over where done // 8 > 2048 + done // 64: 7 done / 64 > 2048, done > 18724.57
    assert min(18724 // 8, 2048 + 18724 // 64) == 18724 // 8 == 2340
    assert min(18728 // 8, 2048 + 18728 // 64) == 2048 + 18728 // 64 == 2340 < 18728 // 8 == 2341
    assert H.batch_schedule(40000, 18724)[0] == 2340 and H.batch_schedule(40000, 18728)[0] == 2340
    assert H.batch_schedule(40000, 32000)[0] == 2048 + 500
    # a cap: BUILD_BATCH = 7 from 56 rows on; BUILD_BATCH = 1 is one row per batch; hnsw_add starts at the rows it finds
    s = H.batch_schedule(3000, 1, 7)
    assert max(s) == 7 and s[:15] == [1] * 15 and sum(s) == 2999
    done = 1
    for b in s:
        assert b == min(7, max(1, done // 8), 3000 - done)
        done += b
    assert H.batch_schedule(3000, 1, 1) == [1] * 2999
    assert H.batch_schedule(2300, 2000) == [250, 50] and H.batch_schedule(2001, 2000) == [1]
    # the engine caps the setting at 16384: 2048 + 10^6 // 64 = 17673 rows would fit the other terms
    assert H.batch_schedule(2 * 10 ** 6, 10 ** 6, 10 ** 9)[0] == H.batch_schedule(2 * 10 ** 6, 10 ** 6)[0] == 16384


# ---- the GPU tests' data sets meet their conditions ------------------------------------------------------------------
def _distinct_rows(base):
    _, counts = np.unique(base, axis=0, return_counts=True)
    return counts.max()


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_main_sweep_data_meets_its_conditions(O, metric):
    base = H.main_data(O)
    assert _distinct_rows(base) <= 8 and not base[2001].any()
    P, n = H.MAIN, len(base)
    for flags in H.MAIN_FLAGS:
        for B in H.MAIN_BATCHES:
            _, cnt = O.hnsw_build_batched(base, H.batch_schedule(n, 1, B), O.METRICS[metric], P["M"], P["efc"], P["seed"],
                                          H.flag_bits(O, flags), O.MODE_DEV)
            tag = "%s %s BUILD_BATCH %d: %s" % (metric, flags, B, cnt.tolist())
            assert cnt[H.TASKS] > 100, tag
            assert cnt[H.ABOVE_TOP] >= 1, tag
            if B > 1:
                assert cnt[H.ENTRY_CHANGES_IN_BATCH] >= 1, tag
                if "heuristic" in flags:
                    assert cnt[H.TASKS_2_PENDING] >= 20, tag
            if "symmetric" in flags:
                assert cnt[H.SYM_REMOVED] >= 20, tag


def test_large_case_reaches_the_threaded_paths(O):
    base = H.large_data(O)
    assert _distinct_rows(base) <= 8
    P, n = H.LARGE, len(base)
    sched = H.batch_schedule(n, 1)
    assert max(sched) >= 256, "threaded linking starts at batches of 256"
    done, slow = 1, 0
    for b in sched:
        if 2048 + done // 64 < min(done // 8, n - done):
            assert b == 2048 + done // 64
            slow += 1
        done += b
    assert slow >= 1, "the 2048 + done / 64 term must size a batch"
    for flags in ("closest", "heuristic+symmetric"):
        _, cnt = O.hnsw_build_batched(base, sched, O.COSINE, P["M"], P["efc"], P["seed"], H.flag_bits(O, flags), O.MODE_DEV)
        assert cnt[H.MOST_TASKS_IN_BATCH] >= 1024, "%s: threaded gather and apply start at 1024 tasks: %s" % (flags, cnt.tolist())


@pytest.mark.parametrize("dim,metric", H.ADD_CASES)
def test_add_data_meets_its_conditions(O, dim, metric):
    """Rows added to an installed sequential graph (closest-m: it carries no builder) must prune adopted lists, some of them
    full but not in ascending order: the lists on which hnswgpu_hnsw_add's sorted / unsorted verdict decides."""
    base = H.add_data(O, dim)
    assert _distinct_rows(base) <= 8
    A, code = H.ADD, O.METRICS[metric]
    g = O.hnsw_build_ex(base[:A["n0"]], code, A["M"], A["efc"], A["seed"], 0, mode=O.MODE_DEV)
    pos, tot = A["n0"], np.zeros(9, np.int64)
    for m in A["calls"]:
        g, cnt = O.hnsw_build_batched(base[:pos + m], H.batch_schedule(pos + m, pos), code, A["M"], A["efc"], A["seed"], 0,
                                      O.MODE_DEV, start=g)
        tot += cnt
        pos += m
    assert pos == len(base)
    assert tot[H.ADOPTED_FIRST] >= 50 and tot[H.ADOPTED_UNSORTED] >= 10, tot.tolist()


@pytest.mark.parametrize("dim,M", H.PATH_CASES)
def test_selection_path_data_overflows_lists(O, dim, M):
    base = H.paths_data(O, dim)
    assert _distinct_rows(base) == 2 and len(np.unique(base, axis=0)) == len(base) - 20
    for metric in (O.COSINE, O.L2):
        for ext in ((0, O.BUILD_EXTEND) if (dim, M) in H.PATH_EXTEND else (0,)):
            og, cnt = O.hnsw_build_ex(base, metric, M, H.PATHS["efc"], H.PATHS["seed"], O.BUILD_HEURISTIC | ext, mode=O.MODE_DEV,
                                      want_counters=True)
            assert cnt[3] > 100, "the data set must overflow lists: dim %d M %d metric %d: %s" % (dim, M, metric, cnt)
            if M >= 16:      # a list of more than 24 links: the selection that made it filled register slots of all four waves
                assert ((og.l0_adj >= 0).sum(1) > 24).any()
