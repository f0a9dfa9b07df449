"""No-GPU checks of the IVF-FLAT filtered search: the two C entry points exist, are bound and validate their arguments before
any HIP call; the protocol mirror."""
import ctypes

IVF_FILTERED = ["hnswgpu_ivf_search_filtered", "hnswgpu_ivf_search_filtered_dev"]


def test_ivf_filtered_symbols_are_exported_and_bound(native_lib):
    L = ctypes.CDLL(native_lib.SO)
    for name in IVF_FILTERED:
        assert hasattr(L, name), "libhnswgpu.so does not export %s" % name
        assert name in native_lib.EXPORTS and name in native_lib._SIGS
        assert getattr(native_lib.lib(), name).argtypes is not None
    assert len(native_lib._SIGS["hnswgpu_ivf_search_filtered"]) == 9       # idx Q nq k nprobe allow ids dist probes
    assert len(native_lib._SIGS["hnswgpu_ivf_search_filtered_dev"]) == 9   # idx Q nq k nprobe allow ids dist stream
    assert native_lib.lib().hnswgpu_version() == 104                        # the new symbols are additive


def test_ivf_filtered_entry_points_check_arguments_before_any_hip_call(native_lib):
    L = native_lib.lib()
    one = ctypes.c_void_p(8)           # a non-null token; never dereferenced on these paths
    # a stand-in for a handle: zeroed memory, larger than the handle.  The argument checks return before they look at it,
    # and if one did, it would find a handle without lists (-3) -- never a HIP call, never a wild pointer
    blank = ctypes.create_string_buffer(1 << 16)
    h = ctypes.cast(blank, ctypes.c_void_p)
    for fn, tail in ((L.hnswgpu_ivf_search_filtered, (None,)), (L.hnswgpu_ivf_search_filtered_dev, (None,))):
        assert fn(None, one, 1, 1, 1, one, one, one, *tail) == -1
        assert b"idx is null" in L.hnswgpu_last_error()
        assert fn(h, one, 1, 1, 1, None, one, one, *tail) == -1             # a null mask
        assert b"allow is null" in L.hnswgpu_last_error()
        assert fn(h, None, 1, 1, 1, one, one, one, *tail) == -1             # null queries
        assert b"null argument" in L.hnswgpu_last_error()
        assert fn(h, one, 1, 1, 1, one, None, one, *tail) == -1             # null ids
        assert fn(h, one, 1, 1, 1, one, one, None, *tail) == -1             # null distances
        assert fn(h, one, 1, 0, 1, one, one, one, *tail) == -1              # k < 1
        assert b"k >= 1" in L.hnswgpu_last_error()
        assert fn(h, one, 1, 1, 0, one, one, one, *tail) == -1              # nprobe < 1
        assert fn(h, one, -1, 1, 1, one, one, one, *tail) == -1             # nq < 0
        assert fn(h, one, 1, 1025, 1, one, one, one, *tail) == -5           # the unfiltered call's limits
        assert fn(h, one, 1, 1, 1025, one, one, one, *tail) == -5


def test_filterable_ivf_index_is_a_filterable_index():
    from hnsw_clj_amd import ivf_flat, protocol

    assert issubclass(protocol.GpuFilterableIvfFlatIndex, protocol.FilterableIndex)
    assert issubclass(protocol.GpuFilterableIvfFlatIndex, protocol.GpuIvfFlatIndex)
    assert protocol.supports_filtering(protocol.GpuFilterableIvfFlatIndex(None)) is True
    assert protocol.supports_batch_search(protocol.GpuFilterableIvfFlatIndex(None))
    assert protocol.GpuFilterableIvfFlatIndex(None).index_type_star() == "ivf-flat"
    # the reference's IVF index has no FilterableIndex, and its mirror still has none
    assert protocol.supports_filtering(protocol.GpuIvfFlatIndex(None)) is False
    assert not issubclass(protocol.GpuIvfFlatIndex, protocol.FilterableIndex)
    assert callable(ivf_flat.search_knn_filtered) and callable(ivf_flat.search_batch_filtered)
