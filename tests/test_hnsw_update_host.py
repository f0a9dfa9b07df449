"""hnswgpu_hnsw_update without a GPU: the numpy model of an update (hnsw_update_model.py, the rule's one specification) anchored to
merged behaviour -- an update of the LAST m rows is hnsw_remove_model.remove followed by oracle.hnsw_build_batched over the start
graph, edge for edge --, the conditions the data sets of test_hnsw_update_gpu.py must meet (from the model's own counters, so that
no GPU test passes vacuously), the model's unlink against hnsw_remove_model.remove, the symbol exported, bound and declared, a
null handle refused before any HIP call, and the mirror's update_vectors over a stand-in handle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hnsw_build_model as H
import hnsw_remove_model as R
import hnsw_update_model as U
import lsh_remove_model as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUILT = {}


def _graph(O, dim, metric, name):
    """The batched build of the GPU tests' base, by the oracle (what engine.Index.hnsw_build makes: test_hnsw_build_batched_gpu.py)."""
    key = (dim, metric, name)
    if key not in _BUILT:
        base, _, _ = U.rows(O, dim)
        _BUILT[key] = O.hnsw_build_batched(base, H.batch_schedule(len(base), 1), O.METRICS[metric], U.M, U.EFC, U.SEED, H.flag_bits(O, name),
                                           O.MODE_DEV)[0]
    return _BUILT[key]


# ---- the model is anchored ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 65, 200])
@pytest.mark.parametrize("name", H.MAIN_FLAGS)
def test_tail_update_is_remove_then_add(oracle, name, m):
    """None of the four differences applies to the last m rows: remove renumbers nothing, add hands out the same ids, the same
    level draws, the same batch schedule (one batch at m = 1 and 65, several at 200)."""
    O = oracle
    flags = H.flag_bits(O, name)
    for dim, metric in ((40, "cosine"), (40, "l2"), (1100, "dot")):
        base, pool, _ = U.rows(O, dim)
        n, code = len(base), O.METRICS[metric]
        g = _graph(O, dim, metric, name)
        ids = np.arange(n - m, n)[::-1]                      # (within one call the order of ids does not matter)
        _, new_base = U.new_values(base, pool, ids)
        got, counters = U.update(O, new_base, code, g, ids, U.EFC, flags)
        start = R.remove(O, base, code, g, ids, "heuristic" in name)
        want, _ = O.hnsw_build_batched(new_base, H.batch_schedule(n, n - m), code, U.M, U.EFC, U.SEED, flags, O.MODE_DEV, start=start)
        H.same_graph(got, want, "%s, the last %d rows, dim %d %s" % (name, m, dim, metric))
        np.testing.assert_array_equal(got.levels, g.levels)  # ... and the levels are the seed's draws by id still
        assert counters[U.BATCHES] == len(H.batch_schedule(n, n - m)) and (m < 200 or counters[U.BATCHES] > 1)


def test_unlink_is_remove_mapped_back_to_the_old_ids(oracle):
    O = oracle
    base, _, _ = U.rows(O, 40)
    n = len(base)
    for name in ("closest", "heuristic"):
        g = _graph(O, 40, "cosine", name)
        ids = U.main_ids(g)
        d = R.Distances(O, base, O.COSINE)
        l0, up = U.unlink(g, d, ids, name == "heuristic")
        c = R.remove(O, base, O.COSINE, g, ids, name == "heuristic", d=d)
        kept = LR.kept(n, ids)
        gone = set(int(x) for x in ids)
        for u in range(n):
            for lc in range(int(g.levels[u]) + 1):
                mine = l0[u] if lc == 0 else up[int(g.up_off[u]) + lc - 1]
                if u in gone:
                    assert mine == []                        # every list of every row of U becomes empty
                else:
                    new = int(LR.rank(n, ids)[u])
                    assert mine == [int(kept[x]) for x in R.old_list(c, new, lc)]
                    assert not gone & set(mine)              # no edge leads into U


# ---- the data sets of the GPU tests ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["closest", "heuristic"])
@pytest.mark.parametrize("dim", U.DIMS)
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_gpu_data_meets_its_conditions(oracle, metric, dim, name):
    O = oracle
    base, pool, _ = U.rows(O, dim)
    g = _graph(O, dim, metric, name)
    ids = U.main_ids(g)
    vals, new_base = U.new_values(base, pool, ids)
    assert len(ids) == 150 == len(set(ids.tolist())) and g.n - 1 in ids and g.entry in ids and list(ids) != sorted(ids)
    _, c = U.update(O, new_base, O.METRICS[metric], g, ids, U.EFC, H.flag_bits(O, name))
    print("counters", c)
    assert c[U.REPAIRED_UPPER] >= 1, "no repaired list on an upper layer"
    assert c[U.EMPTIED_THEN_LINKED] >= 1, "no list that the unlink empties and a reverse edge fills again"
    assert c[U.PRUNED] >= 1, "no over-full list pruned during the re-insertion"
    assert c[U.BATCHES] > 1, "one insertion batch only"
    assert c[U.ENTRY_IN_U] == 1 and c[U.ENTRY_TAKEN_BACK] >= 1, "the entry point is not in U, or no re-inserted row takes it back"
    # ties: at most two rows equal any one row, before and after; a duplicated pair across the border; a new value equal to a row outside U
    in_u = np.zeros(g.n, bool)
    in_u[ids] = True
    for rows in (base, new_base):
        _, counts = np.unique(rows, axis=0, return_counts=True)
        assert counts.max() == 2
    assert in_u[100] and not in_u[300] and np.array_equal(base[100], base[300])
    assert not in_u[7] and any(np.array_equal(v, base[7]) for v in vals)


# ---- the symbol -----------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_bound_and_declared(native_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", native_lib.SO], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^[0-9a-f]+ T hnswgpu_hnsw_update$", nm, re.M), "hnswgpu_hnsw_update is not an exported function"
    assert "hnswgpu_hnsw_update" in native_lib.EXPORTS
    assert native_lib._SIGS["hnswgpu_hnsw_update"] == ["p", "p", "p", "i64", "i32"]
    with open(os.path.join(ROOT, "include", "hnswgpu.h")) as f:
        hdr = f.read()
    assert re.search(r"^int hnswgpu_hnsw_update\(hnswgpu_index \*idx, const int32_t \*ids, const float \*rows, int64_t m, "
                     r"int32_t ef_construction\);$", hdr, re.M)
    assert "updates of an HNSW graph" not in hdr             # struck from hnswgpu_ivf_update's out-of-scope list


def test_null_handle_is_refused_without_gpu(native_lib):
    L = native_lib.lib()
    ids, rows = (ctypes.c_int32 * 4)(), (ctypes.c_float * 16)()
    for args in ((ids, rows, 1, 200), (ids, rows, 0, 200), (None, None, -1, 200), (None, None, 0, 0), (ids, rows, 1, 0)):
        assert L.hnswgpu_hnsw_update(None, *args) == -1      # the handle comes before m == 0 and before ef_construction
        assert b"idx is null" in L.hnswgpu_last_error()


def test_bindings_exist():
    from hnsw_clj_amd import engine, ultra_fast

    assert callable(engine.Index.hnsw_update) and callable(ultra_fast.update_vectors)
    assert "Update existing vectors" in ultra_fast.update_vectors.__doc__ and "hnswgpu_hnsw_update" in ultra_fast.update_vectors.__doc__


# ---- the mirror over a stand-in handle ------------------------------------------------------------------------------------------
class _Handle:
    """In engine.Index's place: every hnsw_update call recorded."""

    def __init__(self, n):
        self.n = n
        self.calls = []

    def hnsw_update(self, ids, rows, ef_construction):
        self.calls.append((np.asarray(ids).tolist(), np.asarray(rows).tolist(), ef_construction))


def test_mirror_update_vectors_checks_its_arguments():
    from hnsw_clj_amd import ultra_fast as F

    h = _Handle(5)
    graph = F.UltraGraph(h, ["a", "b", "c", "d", "b"], 4, 20, F.cosine_distance_ultra)
    graph._route = "stale"
    assert F.update_vectors(graph, [("d", [1.0, 2.0]), ("a", [3.0, 4.0])]) is graph
    assert h.calls == [([3, 0], [[1.0, 2.0], [3.0, 4.0]], 20)]           # rows by the caller's ids, the graph's ef_construction
    assert graph.ids == ["a", "b", "c", "d", "b"] and "_route" not in graph.__dict__
    with pytest.raises(KeyError):
        F.update_vectors(graph, [("a", [0.0, 1.0]), ("z", [0.0, 1.0])])     # unknown: nothing is updated, not even "a"
    with pytest.raises(ValueError, match="names 2 rows"):
        F.update_vectors(graph, [("b", [0.0, 1.0])])
    with pytest.raises(ValueError, match="appears twice"):
        F.update_vectors(graph, [("c", [0.0, 1.0]), ("c", [1.0, 1.0])])
    with pytest.raises(ValueError, match="differ in length"):
        F.update_vectors(graph, [("c", [0.0, 1.0]), ("d", [1.0])])
    assert F.update_vectors(graph, []) is graph and len(h.calls) == 1    # empty input does not call it


def test_engine_update_checks_the_row_count(native_lib):
    """engine.Index.hnsw_update refuses m ids for another number of rows before the library is called (no handle is needed)."""
    from hnsw_clj_amd import engine

    ix = engine.Index.__new__(engine.Index)
    ix.dim, ix._h = 4, None
    with pytest.raises(ValueError, match="2 ids for 1 rows"):
        ix.hnsw_update([1, 2], np.zeros((1, 4), np.float32))
