"""No-GPU checks of hnswgpu_ivf_add: the entry point exists, is bound and refuses a null handle before any HIP call; the Python
seams exist; the numpy model of merged lists the GPU tests expect, on a hand-written case."""
import ctypes
import subprocess

import numpy as np

from ivf_add_model import merged_lists


def test_ivf_add_symbol_is_exported_and_bound(native_lib):
    syms = subprocess.run(["nm", "-D", native_lib.SO], check=True, capture_output=True, text=True).stdout
    assert any(line.split()[-1] == "hnswgpu_ivf_add" and " T " in line for line in syms.splitlines()), "nm -D: no hnswgpu_ivf_add"
    assert "hnswgpu_ivf_add" in native_lib.EXPORTS
    assert native_lib._SIGS["hnswgpu_ivf_add"] == ["p", "p", "i64"]     # idx rows m
    assert native_lib.lib().hnswgpu_ivf_add.argtypes is not None
    assert native_lib.lib().hnswgpu_version() == 104                    # the new symbol is additive


def test_ivf_add_refuses_a_null_handle_with_a_message(native_lib):
    L = native_lib.lib()
    p = np.zeros(4, np.float32)
    assert L.hnswgpu_ivf_add(None, p.ctypes.data_as(ctypes.c_void_p), 1) == -1
    assert b"idx is null" in L.hnswgpu_last_error()


def test_python_seams_exist():
    from hnsw_clj_amd import engine, ivf_flat

    assert callable(engine.Index.ivf_add)
    assert callable(ivf_flat.add_vectors)


def test_merged_lists_model_on_a_hand_written_case():
    # three lists over rows 0..5: [4, 0] [] [2, 5, 1, 3]; rows 6..10 go to lists 2, 1, 0, 1, 2
    off, ids = merged_lists([0, 2, 2, 6], [4, 0, 2, 5, 1, 3], [2, 1, 0, 1, 2])
    assert off.dtype == np.int64 and ids.dtype == np.int32
    assert off.tolist() == [0, 3, 5, 11]
    assert ids.tolist() == [4, 0, 8, 7, 9, 2, 5, 1, 3, 6, 10]
    # nothing added: the lists as they were
    off, ids = merged_lists([0, 2, 2, 6], [4, 0, 2, 5, 1, 3], [])
    assert off.tolist() == [0, 2, 2, 6] and ids.tolist() == [4, 0, 2, 5, 1, 3]
    # adding in two calls is adding in one
    o1, i1 = merged_lists([0, 2, 2, 6], [4, 0, 2, 5, 1, 3], [2, 1])
    o2, i2 = merged_lists(o1, i1, [0, 1, 2])
    assert o2.tolist() == [0, 3, 5, 11] and i2.tolist() == [4, 0, 8, 7, 9, 2, 5, 1, 3, 6, 10]
    # an identity layout stays one while every new row falls into the last list that has members
    off, ids = merged_lists([0, 2, 4, 4], [0, 1, 2, 3], [2, 2])
    assert ids.tolist() == [0, 1, 2, 3, 4, 5] and off.tolist() == [0, 2, 4, 6]
