"""No-GPU checks of the range search under an allow-mask: the four C entry points are exported, declared and bound, and the
Python wrappers reject masks and radii of the wrong shape before any call into the library."""
import ctypes
import os

import numpy as np
import pytest

NAMES = ["hnswgpu_range_search_filtered", "hnswgpu_range_search_filtered_dev", "hnswgpu_range_search_filtered_each",
         "hnswgpu_range_search_filtered_each_dev"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hnswgpu.h")


def test_symbols_are_exported_declared_and_bound(native_lib):
    L, hdr = ctypes.CDLL(native_lib.SO), open(HEADER).read()
    for name in NAMES:
        assert hasattr(L, name), "libhnswgpu.so does not export %s" % name
        assert "int %s(hnswgpu_index *idx" % name in hdr
        assert name in native_lib.EXPORTS
    plain = native_lib._SIGS["hnswgpu_range_search"]                    # ... radius flags | mask | lims ids dist cap
    assert native_lib._SIGS[NAMES[0]] == native_lib._SIGS[NAMES[2]] == plain[:5] + ["p"] + plain[5:]
    assert native_lib._SIGS[NAMES[1]] == native_lib._SIGS[NAMES[3]] == native_lib._SIGS[NAMES[0]] + ["p"]
    one = ctypes.c_void_p(8)           # a non-null token; never dereferenced on these paths
    for name in NAMES:
        tail = (None,) if name.endswith("_dev") else ()
        assert getattr(native_lib.lib(), name)(None, one, 1, one, 0, one, one, one, one, 4, *tail) == -1
        assert b"idx is null" in native_lib.lib().hnswgpu_last_error()


class _Handle:
    """An Index without a device: the wrappers check shapes before they touch the handle."""
    n, dim, _h = 70, 4, None


def test_wrappers_reject_wrong_shapes(native_lib):
    from hnsw_clj_amd import engine

    idx, Q = _Handle(), np.zeros((3, 4), np.float32)
    single = lambda *a: engine.Index.range_search_filtered(idx, *a)
    each = lambda *a: engine.Index.range_search_filtered_each(idx, *a)
    idx._radii = lambda r, nq: engine.Index._radii(idx, r, nq)
    idx._range_filtered = lambda *a: engine.Index._range_filtered(idx, *a)
    for call, bad_mask in ((single, np.zeros(2, np.uint32)), (single, np.zeros(3, np.int32)), (single, np.zeros((3, 3), np.uint32)),
                           (each, np.zeros((2, 3), np.uint32)), (each, np.zeros((3, 2), np.uint32)), (each, np.zeros(3, np.uint32))):
        with pytest.raises(ValueError):
            call(Q, 0.5, bad_mask)
    for call, mask in ((single, np.zeros(3, np.uint32)), (each, np.zeros((3, 3), np.uint32))):
        with pytest.raises(ValueError):
            call(Q, np.zeros(2, np.float32), mask)                      # one radius per query, or a scalar
