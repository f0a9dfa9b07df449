"""hnswgpu_lsh_remove without a GPU: the numpy model of a removal against the counting sort of the kept codes, the symbol exported,
bound and declared, a null handle refused before any HIP call, and the mirror's remove_vectors over a stand-in handle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lsh_model as M
import lsh_remove_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model ------------------------------------------------------------------------------------------------------------
def _tables(n, tables, bits, seed):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 1 << bits, (n, tables)).astype(np.uint16)
    off, ids = M.buckets(codes, bits)
    return rng, codes, off, ids


def _assert_compact(codes, off, ids, rows, bits):
    k = R.kept(len(codes), rows)
    gc, go, gi = R.compact(codes, off, ids, rows)
    eo, ei = M.buckets(codes[k], bits)
    np.testing.assert_array_equal(gc, codes[k])
    np.testing.assert_array_equal(go, eo)
    np.testing.assert_array_equal(gi, ei)
    return k, go, gi


@pytest.mark.parametrize("tables,bits", [(1, 1), (3, 5), (8, 6), (8, 12), (2, 16), (16, 1), (16, 16)])
def test_model_compact_equals_the_counting_sort_of_the_kept_codes(tables, bits):
    n = 2500
    rng, codes, off, ids = _tables(n, tables, bits, 100 * tables + bits)
    for m in (1, 33, 700, n - 1):
        rows = rng.choice(n, m, replace=False)
        k, _, _ = _assert_compact(codes, off, ids, rows, bits)
        assert len(k) == n - m


def test_model_kept_and_rank():
    assert R.kept(5, [3, 1, 3]).tolist() == [0, 2, 4] and R.kept(5, [3, 1, 3]).dtype == np.int64
    assert R.rank(5, [3, 1, 3]).tolist() == [0, -1, 1, -1, 2]
    assert R.kept(3, []).tolist() == [0, 1, 2] and R.rank(3, []).tolist() == [0, 1, 2]
    assert R.kept(3, [2, 0, 1]).tolist() == [] and R.rank(3, [0, 1, 2]).tolist() == [-1, -1, -1]


def test_model_edges():
    n, bits = 77, 3                                          # n is no multiple of 32
    rng, codes, off, ids = _tables(n, 4, bits, 7)
    # duplicates and an unsorted list are the set they name
    a = R.compact(codes, off, ids, [70, 3, 3, 76, 0, 70])
    b = R.compact(codes, off, ids, [0, 3, 70, 76])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    _assert_compact(codes, off, ids, [70, 3, 3, 76, 0, 70], bits)
    # an emptied bucket: its two offsets coincide, the others keep their members
    b0 = int(codes[5, 0])
    gone = ids[0, off[0, b0]:off[0, b0 + 1]]
    _, go, _ = _assert_compact(codes, off, ids, gone, bits)
    assert go[0, b0] == go[0, b0 + 1] and go[0, -1] == n - len(gone)
    # the last row alone, and the last partial word of 13 rows
    _assert_compact(codes, off, ids, [n - 1], bits)
    _assert_compact(codes, off, ids, np.arange(64, n), bits)
    # an emptied index
    gc, go, gi = R.compact(codes, off, ids, np.arange(n)[::-1])
    assert gc.shape == (0, 4) and gi.shape == (4, 0) and not go.any()
    # the hand example of lsh_model: rows 1 and 4 leave -> table 0: bucket 1 = [3], 2 = [2, 4], 3 = [0, 1]
    off, ids = M.buckets(M.HAND_CODES, 2)
    _, go, gi = R.compact(M.HAND_CODES, off, ids, [4, 1])
    assert go[0].tolist() == [0, 0, 1, 3, 5] and gi[0].tolist() == [3, 2, 4, 0, 1]
    assert go[1].tolist() == [0, 0, 0, 1, 5] and gi[1].tolist() == [1, 0, 2, 3, 4]


# ---- the symbol -----------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_bound_and_declared(native_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", native_lib.SO], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^[0-9a-f]+ T hnswgpu_lsh_remove$", nm, re.M), "hnswgpu_lsh_remove is not an exported function"
    assert "hnswgpu_lsh_remove" in native_lib.EXPORTS
    assert native_lib._SIGS["hnswgpu_lsh_remove"] == ["p", "p", "i64", "p"]
    with open(os.path.join(ROOT, "include", "hnswgpu.h")) as f:
        hdr = f.read()
    assert re.search(r"^int hnswgpu_lsh_remove\(hnswgpu_index \*idx, const int32_t \*rows, int64_t m, int64_t \*n_after\);$", hdr, re.M)


def test_version_stays_104(native_lib):
    assert native_lib.lib().hnswgpu_version() == 104


def test_null_handle_is_refused_without_gpu(native_lib):
    L = native_lib.lib()
    buf = (ctypes.c_int32 * 4)()
    out = ctypes.c_int64(-7)
    assert L.hnswgpu_lsh_remove(None, buf, 1, ctypes.byref(out)) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_lsh_remove(None, buf, 0, ctypes.byref(out)) == -1          # the handle comes before m == 0
    assert L.hnswgpu_lsh_remove(None, None, -1, None) == -1
    assert out.value == -7


def test_bindings_exist():
    from hnsw_clj_amd import engine
    from hnsw_clj_amd import hybrid_lsh as H

    assert callable(engine.Index.lsh_remove) and callable(H.remove_vectors)
    assert "no remove" in H.remove_vectors.__doc__ and "105-129" in H.remove_vectors.__doc__


# ---- the mirror over a stand-in handle --------------------------------------------------------------------------------------
class _Handle:
    """In engine.Index's place: lsh_remove by the model, every call recorded."""

    def __init__(self, n):
        self.n = n
        self.calls = []

    def lsh_remove(self, rows):
        self.calls.append(np.asarray(rows).tolist())
        k = R.kept(self.n, rows)
        self.n = len(k)
        return k


def test_mirror_remove_vectors_keeps_ids_in_step():
    from hnsw_clj_amd import hybrid_lsh as H

    h = _Handle(6)
    index = H.HybridIndex(h, ["a", "b", "c", "d", "e", "f"], H.cosine_distance_ultra)
    assert H.remove_vectors(index, ["e", "b", "e"]) is index
    assert index.ids == ["a", "c", "d", "f"] and h.n == 4
    assert sorted(set(h.calls[0])) == [1, 4] and len(h.calls) == 1
    H.remove_vectors(index, ["f"])
    assert index.ids == ["a", "c", "d"] and h.calls[1] == [3]           # in the CURRENT numbering
    with pytest.raises(KeyError):
        H.remove_vectors(index, ["a", "b"])                             # "b" is gone: nothing is removed, not even "a"
    assert len(h.calls) == 2 and index.ids == ["a", "c", "d"]
    assert H.remove_vectors(index, []) is index and len(h.calls) == 2   # empty input does not call it
    H.remove_vectors(index, ["d", "a", "c"])
    assert index.ids == [] and h.n == 0
