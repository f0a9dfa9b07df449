"""hnswgpu_lsh_update without a GPU: the numpy model of an update -- applied one row at a time -- against the counting sort of the
new codes, for random updates, split calls and shuffled ids; the symbol exported, bound and declared; a null handle refused before
any HIP call; and the mirror's update_vectors over a stand-in handle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lsh_model as M
import lsh_update_model as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model ------------------------------------------------------------------------------------------------------------
def _tables(n, tables, bits, seed):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 1 << bits, (n, tables)).astype(np.uint16)
    off, ids = U.tables(codes, bits)
    return rng, codes, off, ids


def _new_codes(rng, codes, rows, bits):
    """New codes for `rows`: a third of the entries keep their code (a row moves in some tables and stays in others)."""
    new = rng.integers(0, 1 << bits, (len(rows), codes.shape[1])).astype(np.uint16)
    stay = rng.random(new.shape) < 1 / 3
    new[stay] = codes[rows][stay]
    return new


def _assert_is_the_counting_sort(got, codes, rows, new, bits):
    want = codes.copy()
    want[rows] = new
    eo, ei = M.buckets(want, bits)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], eo)
    np.testing.assert_array_equal(got[2], ei)
    for t in range(codes.shape[1]):                            # rows ascending inside every bucket
        for b in np.unique(new[:, t]):
            seg = got[2][t, got[1][t, b]:got[1][t, b + 1]]
            assert (np.diff(seg) > 0).all()


@pytest.mark.parametrize("tables,bits", [(1, 1), (3, 5), (8, 6), (2, 12), (16, 1)])
def test_model_merge_equals_the_counting_sort_of_the_new_codes(tables, bits):
    n = 700
    rng, codes, off, ids = _tables(n, tables, bits, 100 * tables + bits)
    for m in (1, 33, 257, n):
        rows = rng.choice(n, m, replace=False)
        new = _new_codes(rng, codes, rows, bits)
        _assert_is_the_counting_sort(U.merge(codes, off, ids, rows, new), codes, rows, new, bits)


def test_model_split_calls_and_shuffled_ids_give_one_result():
    n, bits = 500, 4
    rng, codes, off, ids = _tables(n, 4, bits, 9)
    rows = rng.choice(n, 120, replace=False)
    new = _new_codes(rng, codes, rows, bits)
    one = U.merge(codes, off, ids, rows, new)
    state = (codes, off, ids)
    for a, b in ((0, 1), (1, 70), (70, 120)):                  # three calls
        state = U.merge(*state, rows[a:b], new[a:b])
    perm = rng.permutation(len(rows))
    shuffled = U.merge(codes, off, ids, rows[perm], new[perm])
    by_id = np.argsort(rows)[::-1]
    descending = U.merge(codes, off, ids, rows[by_id], new[by_id])
    for other in (state, shuffled, descending):
        assert all(np.array_equal(x, y) for x, y in zip(one, other))
    _assert_is_the_counting_sort(one, codes, rows, new, bits)


def test_model_edges():
    # the hand example of lsh_model: table 0: bucket 1 = [5], 2 = [3, 4, 6], 3 = [0, 1, 2]; table 1: 2 = [2], 3 = [0, 1, 3, 4, 5, 6]
    off, ids = M.buckets(M.HAND_CODES, 2)
    # row 4 moves in table 0 only, between 0 and 1 ... and row 0 moves in both tables, to the front of [3, 6] and of [2]
    c, o, i = U.merge(M.HAND_CODES, off, ids, [4, 0], [[3, 3], [2, 2]])
    assert o[0].tolist() == [0, 0, 1, 4, 7] and i[0].tolist() == [5, 0, 3, 6, 1, 2, 4]
    assert o[1].tolist() == [0, 0, 0, 2, 7] and i[1].tolist() == [0, 2, 1, 3, 4, 5, 6]
    assert c[4].tolist() == [3, 3] and c[0].tolist() == [2, 2]
    # the same codes again change nothing
    same = U.merge(M.HAND_CODES, off, ids, [6, 2], M.HAND_CODES[[6, 2]])
    assert np.array_equal(same[0], M.HAND_CODES) and np.array_equal(same[1], off) and np.array_equal(same[2], ids)
    # bucket 1 of table 0 empties and the empty bucket 0 is filled; rows 2 and 3 swap buckets
    c, o, i = U.merge(M.HAND_CODES, off, ids, [5, 2, 3], [[0, 3], [2, 2], [3, 3]])
    assert o[0].tolist() == [0, 1, 1, 4, 7] and i[0].tolist() == [5, 2, 4, 6, 0, 1, 3]
    eo, ei = M.buckets(c, 2)
    assert np.array_equal(o, eo) and np.array_equal(i, ei)


def test_model_apply():
    base = np.arange(12, dtype=np.float32).reshape(4, 3)
    out = U.apply(base, [3, 0], [[1, 1, 1], [2, 2, 2]])
    assert out.tolist() == [[2, 2, 2], [3, 4, 5], [6, 7, 8], [1, 1, 1]] and base[0, 0] == 0 and out.dtype == np.float32
    with pytest.raises(AssertionError):
        U.apply(base, [1, 1], [[0, 0, 0], [1, 1, 1]])


# ---- the symbol -----------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_bound_and_declared(native_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", native_lib.SO], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^[0-9a-f]+ T hnswgpu_lsh_update$", nm, re.M), "hnswgpu_lsh_update is not an exported function"
    assert "hnswgpu_lsh_update" in native_lib.EXPORTS
    assert native_lib._SIGS["hnswgpu_lsh_update"] == ["p", "p", "p", "i64"]
    with open(os.path.join(ROOT, "include", "hnswgpu.h")) as f:
        hdr = f.read()
    assert re.search(r"^int hnswgpu_lsh_update\(hnswgpu_index \*idx, const int32_t \*ids, const float \*rows, int64_t m\);$", hdr, re.M)
    flat = " ".join(hdr.split()).replace("* ", "")
    assert "in any split of calls, or in any order of `ids`" in flat       # the independence of the split is part of the contract
    assert "LSH tables take new values through hnswgpu_lsh_update" in flat  # ... and hnswgpu_ivf_update's header points here


def test_version_stays_104(native_lib):
    assert native_lib.lib().hnswgpu_version() == 104


def test_null_handle_is_refused_without_gpu(native_lib):
    L = native_lib.lib()
    ids = (ctypes.c_int32 * 4)()
    rows = (ctypes.c_float * 4)()
    for m in (1, 0, -1):                                                 # the handle comes before m == 0 and before m < 0
        assert L.hnswgpu_lsh_update(None, ids, rows, m) == -1
        assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_lsh_update(None, None, None, 0) == -1
    assert b"idx is null" in L.hnswgpu_last_error()


def test_bindings_exist():
    from hnsw_clj_amd import engine
    from hnsw_clj_amd import hybrid_lsh as H

    assert callable(engine.Index.lsh_update) and callable(H.update_vectors)
    assert "Update existing vectors" in H.update_vectors.__doc__
    with open(os.path.join(ROOT, "clj", "native", "hnswgpu_jni.c")) as f:
        assert "Java_hnsw_gpu_Native_lshUpdate" in f.read()
    with open(os.path.join(ROOT, "clj", "src", "hnsw", "gpu.clj")) as f:
        assert "(defn update-lsh-vectors!" in f.read()


# ---- the mirror over a stand-in handle --------------------------------------------------------------------------------------
class _Handle:
    """In engine.Index's place: every call recorded, nothing computed."""

    def __init__(self, n):
        self.n = n
        self.calls = []

    def lsh_update(self, ids, rows):
        self.calls.append((np.asarray(ids).tolist(), np.asarray(rows).copy()))


def test_mirror_update_vectors_raises_before_touching_the_index():
    from hnsw_clj_amd import hybrid_lsh as H

    h = _Handle(5)
    names = ["a", "b", "c", "b", "e"]
    index = H.HybridIndex(h, list(names), H.cosine_distance_ultra)
    v = np.arange(3, dtype=np.float32)
    assert H.update_vectors(index, [("e", v), ("a", v + 1)]) is index
    assert len(h.calls) == 1 and h.calls[0][0] == [4, 0]                 # row ids, in the caller's order
    np.testing.assert_array_equal(h.calls[0][1], np.stack([v, v + 1]))
    assert h.calls[0][1].dtype == np.float32
    assert index.ids == names and h.n == 5                               # ids and n are unchanged
    with pytest.raises(KeyError):
        H.update_vectors(index, [("a", v), ("zz", v)])                   # an unknown id: nothing is updated, not even "a"
    with pytest.raises(ValueError, match="names 2 rows"):
        H.update_vectors(index, [("c", v), ("b", v)])                    # an id of several rows
    with pytest.raises(ValueError, match="twice"):
        H.update_vectors(index, [("c", v), ("a", v), ("c", v + 1)])      # an id twice in the data
    assert len(h.calls) == 1 and index.ids == names
    assert H.update_vectors(index, []) is index and len(h.calls) == 1    # empty input does not call it
