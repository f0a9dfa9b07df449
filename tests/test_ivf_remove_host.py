"""hnswgpu_ivf_remove without a GPU: the numpy model of a removal against a per-list loop, the symbol exported, bound and declared,
a null handle refused before any HIP call, and the mirror's remove_vectors over a stand-in handle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ivf_remove_model as R
from ivf_add_model import merged_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model ------------------------------------------------------------------------------------------------------------
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


def _brute(off, ids, rows):
    """The per-list loop: a list's kept members, in their order, under their new ids."""
    n = len(ids)
    keep, new_id = np.ones(n, bool), R.rank(n, rows)
    keep[np.asarray(rows, np.int64).reshape(-1)] = False
    lists = [[int(new_id[r]) for r in ids[off[l]:off[l + 1]] if keep[r]] for l in range(len(off) - 1)]
    off1 = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return off1, np.array([r for x in lists for r in x], np.int32)


def _assert_compact(off, ids, rows):
    go, gi = R.compact_lists(off, ids, rows)
    eo, ei = _brute(off, ids, rows)
    np.testing.assert_array_equal(go, eo)
    np.testing.assert_array_equal(gi, ei)
    assert go.dtype == np.int64 and gi.dtype == np.int32
    n1 = len(R.kept(len(ids), rows))
    assert go[0] == 0 and go[-1] == n1 and sorted(gi.tolist()) == list(range(n1))
    return go, gi


@pytest.mark.parametrize("nlist", [1, 7, 64])
def test_model_equals_the_per_list_loop(nlist):
    n = 2500
    rng, off, ids = _lists(n, nlist, 10 + nlist, empty=(2, 5, 63) if nlist > 1 else ())
    assert nlist == 1 or (np.diff(off) == 0).any()
    for m in (1, 33, 700, n - 1):
        rows = rng.choice(n, m, replace=False)
        go, _ = _assert_compact(off, ids, rows)
        assert go[-1] == n - m


def test_model_edges():
    n = 77                                                   # n is no multiple of 32
    rng, off, ids = _lists(n, 5, 7, empty=(3,))
    # duplicates and an unsorted list are the set they name
    a = R.compact_lists(off, ids, [70, 3, 3, 76, 0, 70])
    b = R.compact_lists(off, ids, [0, 3, 70, 76])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    _assert_compact(off, ids, [70, 3, 3, 76, 0, 70])
    # a list emptied whole: its two offsets coincide, the others keep their members
    gone = ids[off[1]:off[2]]
    assert len(gone) > 0
    go, _ = _assert_compact(off, ids, gone)
    assert go[1] == go[2] and go[-1] == n - len(gone)
    assert np.array_equal(np.diff(go)[[0, 2, 3, 4]], np.diff(off)[[0, 2, 3, 4]])
    # the first row alone, the last row alone, and the last partial mask word of 13 rows
    _assert_compact(off, ids, [0])
    _assert_compact(off, ids, [n - 1])
    _assert_compact(off, ids, np.arange(64, n))
    # everything removed
    go, gi = R.compact_lists(off, ids, np.arange(n)[::-1])
    assert gi.shape == (0,) and not go.any() and len(go) == 6


def test_model_hand_example():
    # lists: 0 = [4, 1], 1 = [], 2 = [0, 5, 2], 3 = [3]; rows 1 and 5 leave -> old 0 2 3 4 become 0 1 2 3
    go, gi = R.compact_lists([0, 2, 2, 5, 6], [4, 1, 0, 5, 2, 3], [5, 1, 5])
    assert go.tolist() == [0, 1, 1, 3, 4] and gi.tolist() == [3, 0, 1, 2]


def test_model_undoes_the_add_model():
    rng, off0, ids0 = _lists(300, 6, 3, empty=(4,))
    assign = rng.integers(0, 6, 90)
    off, ids = merged_lists(off0, ids0, assign)
    go, gi = R.compact_lists(off, ids, 300 + rng.permutation(90))
    np.testing.assert_array_equal(go, off0)
    np.testing.assert_array_equal(gi, ids0)


# ---- the symbol -----------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_bound_and_declared(native_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", native_lib.SO], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^[0-9a-f]+ T hnswgpu_ivf_remove$", nm, re.M), "hnswgpu_ivf_remove is not an exported function"
    assert "hnswgpu_ivf_remove" in native_lib.EXPORTS
    assert native_lib._SIGS["hnswgpu_ivf_remove"] == ["p", "p", "i64", "p"]
    with open(os.path.join(ROOT, "include", "hnswgpu.h")) as f:
        hdr = f.read()
    assert re.search(r"^int hnswgpu_ivf_remove\(hnswgpu_index \*idx, const int32_t \*rows, int64_t m, int64_t \*n_after\);$", hdr, re.M)


def test_version_stays_104(native_lib):
    assert native_lib.lib().hnswgpu_version() == 104


def test_null_handle_is_refused_without_gpu(native_lib):
    L = native_lib.lib()
    buf = (ctypes.c_int32 * 4)()
    out = ctypes.c_int64(-7)
    assert L.hnswgpu_ivf_remove(None, buf, 1, ctypes.byref(out)) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_ivf_remove(None, buf, 0, ctypes.byref(out)) == -1          # the handle comes before m == 0
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_ivf_remove(None, None, -1, None) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_ivf_remove(None, None, 0, None) == -1
    assert out.value == -7


def test_bindings_exist():
    from hnsw_clj_amd import engine, ivf_flat

    assert callable(engine.Index.ivf_remove) and callable(ivf_flat.remove_vectors)
    assert "no remove" in ivf_flat.remove_vectors.__doc__ and "137-211" in ivf_flat.remove_vectors.__doc__


# ---- the mirror over a stand-in handle --------------------------------------------------------------------------------------
class _Handle:
    """In engine.Index's place: ivf_remove by the model, every call recorded."""

    def __init__(self, n):
        self.n = n
        self.calls = []

    def ivf_remove(self, rows):
        self.calls.append(np.asarray(rows).tolist())
        k = R.kept(self.n, rows)
        self.n = len(k)
        return k


def test_mirror_remove_vectors_keeps_ids_in_step():
    from hnsw_clj_amd import ivf_flat as F

    h = _Handle(6)
    index = F.IVFFlatIndex(h, ["a", "b", "c", "d", "e", "f"], F.cosine_distance_ultra, 2)
    assert F.remove_vectors(index, ["e", "b", "e"]) is index
    assert index.ids == ["a", "c", "d", "f"] and h.n == 4
    assert sorted(set(h.calls[0])) == [1, 4] and len(h.calls) == 1
    F.remove_vectors(index, ["f"])
    assert index.ids == ["a", "c", "d"] and h.calls[1] == [3]           # in the CURRENT numbering
    with pytest.raises(KeyError):
        F.remove_vectors(index, ["a", "b"])                             # "b" is gone: nothing is removed, not even "a"
    assert len(h.calls) == 2 and index.ids == ["a", "c", "d"]
    assert F.remove_vectors(index, []) is index and len(h.calls) == 2   # empty input does not call it
    H2 = _Handle(4)
    twice = F.IVFFlatIndex(H2, ["x", "y", "x", "z"], F.cosine_distance_ultra, 2)
    F.remove_vectors(twice, ["x"])                                      # an id of several rows removes them all
    assert twice.ids == ["y", "z"] and sorted(H2.calls[0]) == [0, 2]
    F.remove_vectors(index, ["d", "a", "c"])
    assert index.ids == [] and h.n == 0
