"""hnswgpu_hnsw_remove without a GPU: the numpy model of a removal (hnsw_remove_model.py, the rule's one specification) against a
hand-written 8-node graph and a per-list loop, the symbol exported, bound and declared, a null handle refused before any HIP
call, the mirror's remove_vectors over a stand-in handle, and what the repair is worth on the model: recall after removing
40 % of a clustered set, repaired against merely compacted."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hnsw_build_model as B
import hnsw_remove_model as R
import lsh_remove_model as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the hand-written graph -------------------------------------------------------------------------------------------------
# Eight points on a line, node i at x = i (Euclidean: d(i, j) = |i - j| exactly), M = 2, M0 = 4.  Node 2 is the entry point on
# level 2, nodes 5 and 6 reach level 1.
def _line(O):
    base = np.zeros((8, 2), np.float32)
    base[:, 0] = np.arange(8)
    levels = [0, 0, 2, 0, 0, 1, 1, 0]
    l0 = [[1, 2, -1, -1], [0, 2, 3, -1], [1, 3, 0, 4], [2, 4, 1, 5], [3, 5, 6, -1], [4, 6, 7, 3], [5, 7, 4, -1], [6, 5, -1, -1]]
    up_off = [0, 0, 0, 2, 2, 2, 3, 4, 4]
    up = [[5, -1], [-1, -1], [2, 6], [5, -1]]          # node 2 layer 1, node 2 layer 2, node 5 layer 1, node 6 layer 1
    return base, O.Graph(levels, np.array(l0, np.int32), up_off, np.array(up, np.int32).reshape(-1), 2, 2, 2)


def _lists(g):
    return g.l0_adj.reshape(g.n, -1).tolist(), g.up_adj.reshape(-1, g.M).tolist()


def test_hand_graph_a_list_loses_one_member(oracle):
    """Row 4 leaves: 0 1 2 3 5 6 7 become 0 .. 6.  Node 3 [2 4 1 5] draws 5 and 6 through 4's list [3 5 6]: candidates 1 2 5 6 at
    distances 2 1 2 3 -> 2 1 5 6; node 2 [1 3 0 4]: 0 1 3 5 6 at 2 1 1 3 4 -> 1 3 0 5; node 5 [4 6 7 3]: 3 6 7 at 2 1 2 -> 6 3 7;
    node 6 [5 7 4]: 3 5 7 at 3 1 1 -> 5 7 3.  Nodes 0, 1 and 7 lose nobody."""
    O = oracle
    base, g = _line(O)
    c = R.remove(O, base, O.L2, g, [4], heuristic=False)
    l0, up = _lists(c)
    assert l0 == [[1, 2, -1, -1], [0, 2, 3, -1], [1, 3, 0, 4], [2, 1, 4, 5], [5, 3, 6, -1], [4, 6, 3, -1], [5, 4, -1, -1]]
    assert up == [[4, -1], [-1, -1], [2, 5], [4, -1]]
    assert c.levels.tolist() == [0, 0, 2, 0, 1, 1, 0] and c.up_off.tolist() == [0, 0, 0, 2, 2, 3, 4, 4]
    assert (c.entry, c.max_level, c.M, c.M0) == (2, 2, 2, 4)
    # the heuristic on the same candidates: node 3: 2 taken, 1 is closer to 2 (1) than to 3 (2), 5 taken, 6 closer to 5;
    # node 2: 1, 3 taken, 0 closer to 1, 5 closer to 3, 6 closer to 3; node 5: 6, 3 taken, 7 closer to 6; node 6: 5, 7 taken, 3 closer to 5
    h = R.remove(O, base, O.L2, g, [4], heuristic=True)
    l0h, uph = _lists(h)
    assert l0h == [[1, 2, -1, -1], [0, 2, 3, -1], [1, 3, -1, -1], [2, 4, -1, -1], [5, 3, -1, -1], [4, 6, -1, -1], [5, 4, -1, -1]]
    assert uph == up
    # merely compacted: every list keeps what it kept
    k = R.remove(O, base, O.L2, g, [4], heuristic=False, repair=False)
    assert _lists(k)[0] == [[1, 2, -1, -1], [0, 2, 3, -1], [1, 3, 0, -1], [2, 1, 4, -1], [5, 6, 3, -1], [4, 6, -1, -1], [5, 4, -1, -1]]


def test_hand_graph_all_neighbours_leave_entry_removed_top_level_empties(oracle):
    """Rows 1 and 2 leave (named out of order, one twice): 0 3 4 5 6 7 become 0 .. 5.  Node 0 [1 2] loses both: its list is drawn
    from two-hop rows only, 3 (through 1 and 2) and 4 (through 2) -> 3 4.  Node 3 [2 4 1 5]: 4 5 and 0 (through both) at 1 2 3.
    The entry point 2 was the only node of level 2: the level empties, the new entry is the lowest id of level 1, old 5 = new 3.
    Node 5's layer-1 list [2 6] loses 2, whose layer-1 list [5] holds only node 5 itself: 6 stays alone."""
    O = oracle
    base, g = _line(O)
    c = R.remove(O, base, O.L2, g, [2, 1, 2], heuristic=False)
    l0, up = _lists(c)
    assert l0 == [[1, 2, -1, -1], [2, 3, 0, -1], [1, 3, 4, -1], [2, 4, 5, 1], [3, 5, 2, -1], [4, 3, -1, -1]]
    assert up == [[4, -1], [3, -1]]
    assert c.levels.tolist() == [0, 0, 0, 1, 1, 0] and c.up_off.tolist() == [0, 0, 0, 0, 1, 2, 2]
    assert (c.entry, c.max_level) == (3, 1)
    h = R.remove(O, base, O.L2, g, [1, 2], heuristic=True)
    assert _lists(h)[0][0] == [1, -1, -1, -1]                  # 4 is closer to 3 (1) than to 0 (4)
    assert _lists(h)[0][1] == [2, 0, -1, -1]                   # node 3: 4 taken, 5 closer to 4, 0 taken (d(0, 4) = 4 > 3)
    # every candidate gone: node 0 after 1, 2, 3 and 4 left has an empty list, which is legal
    e = R.remove(O, base, O.L2, g, [1, 2, 3, 4], heuristic=False)
    assert _lists(e)[0][0] == [-1, -1, -1, -1]
    # nothing left
    z = R.remove(O, base, O.L2, g, np.arange(8)[::-1], heuristic=True)
    assert (z.n, z.entry, z.max_level, z.M, z.M0) == (0, -1, 0, 2, 4) and z.up_off.tolist() == [0] and z.l0_adj.shape == (0, 4)


def test_compaction_equals_the_per_list_loop(oracle):
    """repair = False on a built graph against the plain loop: a list's kept members, in their order, under their new ids."""
    O = oracle
    n, M = 400, 6
    base = B.clustered(O, n, 24, clusters=6, noise=0.4, seed=3)
    g = O.hnsw_build_ex(base, O.COSINE, M, 30, 42, O.BUILD_HEURISTIC, O.MODE_DEV)
    rng = np.random.default_rng(5)
    for rows in ([n - 1], rng.choice(n, 33, replace=False), np.concatenate([[g.entry], rng.choice(n, 150)]), np.arange(384, n)):
        c = R.remove(O, base, O.COSINE, g, rows, heuristic=True, repair=False)
        keep, new_id, kept = np.ones(n, bool), LR.rank(n, rows), LR.kept(n, rows)
        keep[np.asarray(rows)] = False
        assert c.n == len(kept) and c.levels.tolist() == g.levels[kept].tolist()
        assert c.up_off.tolist() == np.concatenate([[0], np.cumsum(g.levels[kept])]).tolist()
        l0, up = _lists(c)
        for u in kept:
            for lc in range(g.levels[u] + 1):
                want = [int(new_id[x]) for x in R.old_list(g, u, lc) if keep[x]]
                got = l0[new_id[u]] if lc == 0 else up[c.up_off[new_id[u]] + lc - 1]
                assert got == want + [-1] * (len(got) - len(want))
        if keep[g.entry]:
            assert (c.entry, c.max_level) == (new_id[g.entry], g.max_level)
        else:
            top = g.levels[kept].max()
            assert c.max_level == top and kept[c.entry] == kept[g.levels[kept] == top][0]
        # an undamaged list is the same with and without the repair
        r = R.remove(O, base, O.COSINE, g, rows, heuristic=True)
        for u in kept:
            if all(keep[x] for x in R.old_list(g, u, 0)):
                assert _lists(r)[0][new_id[u]] == l0[new_id[u]]


# ---- the symbol -------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_bound_and_declared(native_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", native_lib.SO], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^[0-9a-f]+ T hnswgpu_hnsw_remove$", nm, re.M), "hnswgpu_hnsw_remove is not an exported function"
    assert "hnswgpu_hnsw_remove" in native_lib.EXPORTS
    assert native_lib._SIGS["hnswgpu_hnsw_remove"] == ["p", "p", "i64", "p"]
    with open(os.path.join(ROOT, "include", "hnswgpu.h")) as f:
        hdr = f.read()
    assert re.search(r"^int hnswgpu_hnsw_remove\(hnswgpu_index \*idx, const int32_t \*rows, int64_t m, int64_t \*n_after\);$", hdr, re.M)


def test_version_stays_104(native_lib):
    assert native_lib.lib().hnswgpu_version() == 104


def test_null_handle_is_refused_without_gpu(native_lib):
    L = native_lib.lib()
    buf = (ctypes.c_int32 * 4)()
    out = ctypes.c_int64(-7)
    assert L.hnswgpu_hnsw_remove(None, buf, 1, ctypes.byref(out)) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_hnsw_remove(None, buf, 0, ctypes.byref(out)) == -1          # the handle comes before m == 0
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_hnsw_remove(None, None, -1, None) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_hnsw_remove(None, None, 0, None) == -1
    assert out.value == -7


def test_bindings_exist():
    from hnsw_clj_amd import engine, ultra_fast

    assert callable(engine.Index.hnsw_remove) and callable(ultra_fast.remove_vectors)
    assert "no delete" in ultra_fast.remove_vectors.__doc__ and "hnswgpu_hnsw_remove" in ultra_fast.remove_vectors.__doc__


# ---- the mirror over a stand-in handle ----------------------------------------------------------------------------------------
class _Handle:
    """In engine.Index's place: hnsw_remove by the numbering model, every call recorded."""

    def __init__(self, n):
        self.n = n
        self.calls = []

    def hnsw_remove(self, rows):
        self.calls.append(np.asarray(rows).tolist())
        k = LR.kept(self.n, rows)
        self.n = len(k)
        return k


def test_mirror_remove_vectors_keeps_ids_in_step():
    from hnsw_clj_amd import ultra_fast as U

    h = _Handle(6)
    graph = U.UltraGraph(h, ["a", "b", "c", "d", "e", "f"], 4, 20, U.cosine_distance_ultra)
    assert U.remove_vectors(graph, ["e", "b", "e"]) is graph
    assert graph.ids == ["a", "c", "d", "f"] and h.n == 4
    assert sorted(set(h.calls[0])) == [1, 4] and len(h.calls) == 1
    U.remove_vectors(graph, ["f"])
    assert graph.ids == ["a", "c", "d"] and h.calls[1] == [3]           # in the CURRENT numbering
    with pytest.raises(KeyError):
        U.remove_vectors(graph, ["a", "b"])                             # "b" is gone: nothing is removed, not even "a"
    assert len(h.calls) == 2 and graph.ids == ["a", "c", "d"]
    assert U.remove_vectors(graph, []) is graph and len(h.calls) == 2   # empty input does not call it
    H2 = _Handle(4)
    twice = U.UltraGraph(H2, ["x", "y", "x", "z"], 4, 20, U.cosine_distance_ultra)
    U.remove_vectors(twice, ["x"])                                      # an id of several rows removes them all
    assert twice.ids == ["y", "z"] and sorted(H2.calls[0]) == [0, 2]
    U.remove_vectors(graph, ["d", "a", "c"])
    assert graph.ids == [] and h.n == 0


# ---- what the repair is worth -------------------------------------------------------------------------------------------------
def test_repair_beats_compaction_at_40_percent(oracle):
    """hnsw_build_model.clustered rows (n 3000, dim 48), the HEURISTIC builder (M 8, efc 40), 40 % of the rows removed at random:
    recall@10 at ef 50 against the exact neighbours among the kept rows.  The repaired graph must be above the merely compacted
    one.  (Not asserted at 10 %, where the two are within noise, nor for the closest-m builder, whose recall on clustered rows is
    near zero with or without removal.)  The figures of this test are in DESIGN.md beside a fresh build of the kept rows."""
    O = oracle
    n, dim, M, efc = 3000, 48, 8, 40
    base = B.main_data(O)
    assert base.shape == (n, dim)
    g = O.hnsw_build_ex(base, O.COSINE, M, efc, 42, O.BUILD_HEURISTIC, O.MODE_DEV)
    rows = np.random.default_rng(17).choice(n, (n * 4) // 10, replace=False)
    kept = LR.kept(n, rows)
    sub = np.ascontiguousarray(base[kept])
    d = R.Distances(O, base, O.COSINE)
    repaired = R.remove(O, base, O.COSINE, g, rows, heuristic=True, d=d)
    compacted = R.remove(O, base, O.COSINE, g, rows, heuristic=True, repair=False)
    Q = B.clustered(O, 200, dim, clusters=12, noise=0.4, seed=8, pairs=0, zero=False)
    exact, _, _ = O.exact_knn(sub, Q, 10, O.COSINE, O.MODE_DEV)
    rec = {}
    for name, gr in (("compacted", compacted), ("repaired", repaired)):
        ids, _, _, _ = O.hnsw_search(sub, gr, Q, 10, 50, O.COSINE, O.MODE_DEV)
        rec[name] = O.recall(ids, exact)
    print("recall@10 at ef 50 after removing 40 %%: compacted %.3f, repaired %.3f" % (rec["compacted"], rec["repaired"]))
    assert rec["repaired"] > rec["compacted"], rec
