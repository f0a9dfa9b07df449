"""No-GPU checks of the forest calls (several HNSW sub-graphs on one handle: include/hnswgpu.h, hnswgpu_set_graph_parts and
friends): the header declares and the library exports them, and the Python helper that lays per-partition row lists out as the
rows of one handle does what the mirrors rely on."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["hnswgpu_set_graph_parts", "hnswgpu_hnsw_build_parts", "hnswgpu_graph_parts", "hnswgpu_hnsw_search_parts",
           "hnswgpu_hnsw_search_parts_dev"]


def test_header_declares_and_library_exports_the_five_symbols(native_lib):
    hdr = open(os.path.join(ROOT, "include", "hnswgpu.h")).read()
    L = ctypes.CDLL(native_lib.SO)
    for name in SYMBOLS:
        assert re.search(r"^int %s\(hnswgpu_index \*idx|^int %s\(const hnswgpu_index \*idx" % (name, name), hdr, re.M), name
        assert hasattr(L, name), "%s is declared in hnswgpu.h but not exported" % name
        assert name in native_lib.EXPORTS
    assert L.hnswgpu_version() == 104          # the forest changes no file format and no existing call


def test_null_handle_is_an_argument_error(native_lib):
    """Every one of the five checks its handle before it touches a device."""
    L = native_lib.lib()
    n = ctypes.c_int32(7)
    assert L.hnswgpu_set_graph_parts(None, None, None, 4, None, None, 2, 1, None, None, None) == -1
    assert L.hnswgpu_hnsw_build_parts(None, 1, None, 8, 50, 42, 0) == -1
    assert L.hnswgpu_graph_parts(None, ctypes.byref(n), None, None, None) == -1
    assert L.hnswgpu_hnsw_search_parts(None, None, 1, 3, 0, None, 0, 3, None, None, None) == -1
    assert L.hnswgpu_hnsw_search_parts_dev(None, None, 1, 3, 0, None, 0, 3, None, None, None, None) == -1
    assert b"idx is null" in L.hnswgpu_last_error()


def test_parts_layout_groups_rows_by_part():
    from hnsw_clj_amd import engine

    base = np.arange(10 * 3, dtype=np.float32).reshape(10, 3)
    rows = [np.array([7, 2], np.int32), np.array([], np.int32), [9], np.array([0, 1, 3, 4, 5, 6, 8])]
    grouped, part_off, pos = engine.parts_layout(base, rows)
    assert part_off.dtype == np.int64 and part_off.tolist() == [0, 2, 2, 3, 10]          # the empty part: off[1] == off[2]
    assert pos.dtype == np.int32 and pos.tolist() == [7, 2, 9, 0, 1, 3, 4, 5, 6, 8]
    assert grouped.dtype == np.float32 and grouped.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(grouped, base[pos])
    for p, r in enumerate(rows):                                                         # handle row -> data position, part by part
        assert pos[part_off[p]:part_off[p + 1]].tolist() == list(np.asarray(r).tolist())
    # a handle row that a search returns maps back through pos; -1 stays -1 in the mirrors
    assert base[pos[2], 0] == 27.0


def test_parts_layout_edges():
    from hnsw_clj_amd import engine

    base = np.ones((4, 2), np.float32)
    grouped, part_off, pos = engine.parts_layout(base, [[], []])
    assert grouped.shape == (0, 2) and part_off.tolist() == [0, 0, 0] and len(pos) == 0
    grouped, part_off, pos = engine.parts_layout(base, [[3, 3]])                          # a row may repeat: the caller's business
    assert part_off.tolist() == [0, 2] and pos.tolist() == [3, 3]
    with pytest.raises(ValueError):
        engine.parts_layout(base, [[0, 4]])
    with pytest.raises(ValueError):
        engine.parts_layout(base, [[-1]])


def test_graph_parts_tables():
    from hnsw_clj_amd import engine

    t = engine.GraphParts([0, 2, 2, 5], [1, -1, 4], [3, 0, 1])
    assert t.nparts == 3 and t.part_off.dtype == np.int64 and t.part_entry.dtype == np.int32 and t.part_max_level.dtype == np.int32


def test_mirrors_keep_the_composition_as_default():
    """The existing mirror tests read index.partitions: one_handle is opt-in."""
    import inspect

    from hnsw_clj_amd import ivf_hnsw, partitioned_hnsw

    assert inspect.signature(partitioned_hnsw.build_partitioned_hnsw).parameters["one_handle"].default is False
    assert inspect.signature(ivf_hnsw.build_ivf_hnsw_index).parameters["one_handle"].default is False
