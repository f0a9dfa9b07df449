"""No-GPU checks of the range search through the IVF lists: the two C entry points are exported, declared and bound, a null
handle is refused, and the Python wrapper rejects radii and probe tables of the wrong shape before any call into the library."""
import ctypes
import os

import numpy as np
import pytest

NAMES = ["hnswgpu_ivf_range_search", "hnswgpu_ivf_range_search_dev"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hnswgpu.h")


def test_symbols_are_exported_declared_and_bound(native_lib):
    L, hdr = ctypes.CDLL(native_lib.SO), open(HEADER).read()
    for name in NAMES:
        assert hasattr(L, name), "libhnswgpu.so does not export %s" % name
        assert "int %s(hnswgpu_index *idx" % name in hdr
        assert name in native_lib.EXPORTS
    plain = native_lib._SIGS["hnswgpu_range_search"]                    # ... radius | nprobe probes | flags lims ids dist cap | out_probes
    assert native_lib._SIGS[NAMES[0]] == plain[:4] + ["i32", "p"] + plain[4:] + ["p"]
    assert native_lib._SIGS[NAMES[1]] == native_lib._SIGS[NAMES[0]] + ["p"]
    one = ctypes.c_void_p(8)           # a non-null token; never dereferenced on these paths
    for name in NAMES:
        tail = (None,) if name.endswith("_dev") else ()
        assert getattr(native_lib.lib(), name)(None, one, 1, one, 2, None, 0, one, one, one, 4, None, *tail) == -1
        assert b"idx is null" in native_lib.lib().hnswgpu_last_error()


class _Handle:
    """An Index without a device: the wrapper checks shapes before it touches the handle."""
    n, dim, _h = 70, 4, None


def test_wrapper_rejects_wrong_shapes(native_lib):
    from hnsw_clj_amd import engine

    idx, Q = _Handle(), np.zeros((3, 4), np.float32)
    idx._radii = lambda r, nq: engine.Index._radii(idx, r, nq)
    for radius, probes in ((np.zeros(2, np.float32), None), (np.zeros((3, 1), np.float32), None),   # a scalar or one per query
                           (0.5, np.zeros((2, 4), np.int32)), (0.5, np.zeros(3, np.int32)), (0.5, np.zeros((3, 0), np.int32))):
        with pytest.raises(ValueError):
            engine.Index.ivf_range_search(idx, Q, radius, 4, probes=probes)
