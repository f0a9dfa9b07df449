"""hnswgpu_ivf_update without a GPU: the numpy model of an update against hand-written cases and its invariants on random input, the
symbol exported, bound and declared, a null handle refused before any HIP call, and the mirror's update_vectors over a stand-in
handle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ivf_update_model as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# lists: 0 = [4, 1], 1 = [], 2 = [0, 5, 2], 3 = [3]
OFF, IDS = [0, 2, 2, 5, 6], [4, 1, 0, 5, 2, 3]


def _lists(n, nlist, seed, empty=()):
    """Random lists over n rows: every row in one list, the members of a list in a random order; the lists in `empty` get none."""
    rng = np.random.default_rng(seed)
    live = [l for l in range(nlist) if l not in empty]
    a = rng.choice(live, n)
    order = rng.permutation(n)
    ids = order[np.argsort(a[order], kind="stable")].astype(np.int32)
    off = np.zeros(nlist + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(a, minlength=nlist))
    return rng, off, ids


# ---- the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,assign,off1,ids1", [
    ([5], [2], [0, 2, 2, 5, 6], [4, 1, 0, 5, 2, 3]),                    # a stayer: nothing moves, it keeps its position
    ([5], [0], [0, 3, 3, 5, 6], [4, 1, 5, 0, 2, 3]),                    # a mover: list 2 closes up, list 0 gets it at its end
    ([3], [2], [0, 2, 2, 6, 6], [4, 1, 0, 5, 2, 3]),                    # an emptied list stays, with two equal offsets
    ([0], [1], [0, 2, 3, 5, 6], [4, 1, 0, 5, 2, 3]),                    # the empty list gets its first member
    ([5, 0], [0, 0], [0, 4, 4, 5, 6], [4, 1, 0, 5, 2, 3]),              # two movers into one list, named in descending order:
    ([0, 5], [0, 0], [0, 4, 4, 5, 6], [4, 1, 0, 5, 2, 3]),              # ... ascending by row id behind the old members, either way
    ([4, 2, 3], [0, 3, 1], [0, 2, 3, 5, 6], [4, 1, 3, 0, 5, 2]),        # a stayer, a mover into an emptied list, one into the empty one
    ([], [], [0, 2, 2, 5, 6], [4, 1, 0, 5, 2, 3]),
])
def test_model_hand_cases(rows, assign, off1, ids1):
    go, gi = U.updated_lists(OFF, IDS, rows, assign)
    assert go.tolist() == off1 and gi.tolist() == ids1
    assert go.dtype == np.int64 and gi.dtype == np.int32


def test_model_split_over_calls_differs_from_one_call():
    one = U.updated_lists(OFF, IDS, [5, 0], [0, 0])
    two = U.updated_lists(*U.updated_lists(OFF, IDS, [5], [0]), [0], [0])
    assert one[1].tolist() == [4, 1, 0, 5, 2, 3] and two[1].tolist() == [4, 1, 5, 0, 2, 3]
    assert one[0].tolist() == two[0].tolist()


@pytest.mark.parametrize("nlist", [1, 7, 64])
def test_model_invariants(nlist):
    n = 2500
    rng, off, ids = _lists(n, nlist, 20 + nlist, empty=(2, 5, 63) if nlist > 1 else ())
    list_of = np.empty(n, np.int64)
    list_of[ids] = np.repeat(np.arange(nlist), np.diff(off))
    for m in (1, 33, 700, n):
        rows = rng.choice(n, m, replace=False)
        assign = np.where(rng.random(m) < 0.5, list_of[rows], rng.integers(0, nlist, m))   # about half stay
        off1, ids1 = U.updated_lists(off, ids, rows, assign)
        assert off1[0] == 0 and off1[-1] == n and (np.diff(off1) >= 0).all()
        assert sorted(ids1.tolist()) == list(range(n)), "ids1 is a permutation of ids"
        new_of = list_of.copy()
        new_of[rows] = assign
        np.testing.assert_array_equal(np.repeat(np.arange(nlist), np.diff(off1)), new_of[ids1], err_msg="a row is not in its list")
        updated = np.zeros(n, bool)
        updated[rows] = True
        moved = new_of != list_of
        for l in range(nlist):
            old, new = ids[off[l]:off[l + 1]], ids1[off1[l]:off1[l + 1]]
            kept = old[~moved[old]]                              # non-updated members and stayers, in their old order
            np.testing.assert_array_equal(new[:len(kept)], kept, err_msg="kept members keep their order and the stayers their index")
            joined = new[len(kept):]
            assert moved[joined].all() and (np.diff(joined) > 0).all(), "the movers stand behind them, ascending by row id"
            np.testing.assert_array_equal(old[~updated[old]], new[~updated[new]][:int((~updated[old]).sum())])
        # the order in which the call names its rows does not matter
        p = rng.permutation(m)
        a2 = U.updated_lists(off, ids, rows[p], assign[p])
        np.testing.assert_array_equal(a2[0], off1)
        np.testing.assert_array_equal(a2[1], ids1)
        # rows that all stay change nothing
        s0, s1 = U.updated_lists(off, ids, rows, list_of[rows])
        np.testing.assert_array_equal(s0, off)
        np.testing.assert_array_equal(s1, ids)


def test_model_refuses_a_row_named_twice():
    with pytest.raises(AssertionError):
        U.updated_lists(OFF, IDS, [5, 5], [0, 2])


# ---- the symbol -----------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_bound_and_declared(native_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", native_lib.SO], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^[0-9a-f]+ T hnswgpu_ivf_update$", nm, re.M), "hnswgpu_ivf_update is not an exported function"
    assert "hnswgpu_ivf_update" in native_lib.EXPORTS
    assert native_lib._SIGS["hnswgpu_ivf_update"] == ["p", "p", "p", "i64"]
    with open(os.path.join(ROOT, "include", "hnswgpu.h")) as f:
        hdr = f.read()
    assert re.search(r"^int hnswgpu_ivf_update\(hnswgpu_index \*idx, const int32_t \*ids, const float \*rows, int64_t m\);$", hdr, re.M)
    assert "update rows in batches" in " ".join(hdr.split()).replace("* ", "").replace("-- ", "")


def test_version_stays_104(native_lib):
    assert native_lib.lib().hnswgpu_version() == 104


def test_null_handle_is_refused_without_gpu(native_lib):
    L = native_lib.lib()
    ids = (ctypes.c_int32 * 4)()
    rows = (ctypes.c_float * 4)()
    for m in (1, 0, -1):                                                 # the handle comes before m == 0 and before m < 0
        assert L.hnswgpu_ivf_update(None, ids, rows, m) == -1
        assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_ivf_update(None, None, None, 0) == -1
    assert b"idx is null" in L.hnswgpu_last_error()


def test_bindings_exist():
    from hnsw_clj_amd import engine, ivf_flat

    assert callable(engine.Index.ivf_update) and callable(ivf_flat.update_vectors)
    assert "Update existing vectors" in ivf_flat.update_vectors.__doc__
    with open(os.path.join(ROOT, "clj", "native", "hnswgpu_jni.c")) as f:
        assert "Java_hnsw_gpu_Native_ivfUpdate" in f.read()
    with open(os.path.join(ROOT, "clj", "src", "hnsw", "gpu.clj")) as f:
        assert "(defn update-ivf-vectors!" in f.read()


# ---- the mirror over a stand-in handle --------------------------------------------------------------------------------------
class _Handle:
    """In engine.Index's place: every call recorded, nothing computed."""

    def __init__(self, n):
        self.n = n
        self.calls = []

    def ivf_update(self, ids, rows):
        self.calls.append((np.asarray(ids).tolist(), np.asarray(rows).copy()))


def test_mirror_update_vectors_raises_before_touching_the_index():
    from hnsw_clj_amd import ivf_flat as F

    h = _Handle(5)
    names = ["a", "b", "c", "b", "e"]
    index = F.IVFFlatIndex(h, list(names), F.cosine_distance_ultra, 2)
    v = np.arange(3, dtype=np.float32)
    assert F.update_vectors(index, [("e", v), ("a", v + 1)]) is index
    assert len(h.calls) == 1 and h.calls[0][0] == [4, 0]                 # row ids, in the caller's order
    np.testing.assert_array_equal(h.calls[0][1], np.stack([v, v + 1]))
    assert h.calls[0][1].dtype == np.float32
    assert index.ids == names and h.n == 5                               # ids and n are unchanged
    with pytest.raises(KeyError):
        F.update_vectors(index, [("a", v), ("zz", v)])                   # an unknown id: nothing is updated, not even "a"
    with pytest.raises(ValueError, match="names 2 rows"):
        F.update_vectors(index, [("c", v), ("b", v)])                    # an id of several rows
    with pytest.raises(ValueError, match="twice"):
        F.update_vectors(index, [("c", v), ("a", v), ("c", v + 1)])      # an id twice in the data
    assert len(h.calls) == 1 and index.ids == names
    assert F.update_vectors(index, []) is index and len(h.calls) == 1    # empty input does not call it
