"""No-GPU checks of the filtered search: the four C entry points exist, are bound and validate their arguments before any HIP
call; the mask packing; the scan / graph rule; the protocol mirror."""
import ctypes

import numpy as np
import pytest

FILTERED = ["hnswgpu_exact_knn_filtered", "hnswgpu_exact_knn_filtered_dev", "hnswgpu_hnsw_search_filtered",
            "hnswgpu_hnsw_search_filtered_dev"]


def test_filtered_symbols_are_exported_and_bound(native_lib):
    L = ctypes.CDLL(native_lib.SO)
    for name in FILTERED:
        assert hasattr(L, name), "libhnswgpu.so does not export %s" % name
        assert name in native_lib.EXPORTS and name in native_lib._SIGS
        assert getattr(native_lib.lib(), name).argtypes is not None


def test_filtered_entry_points_check_arguments_before_any_hip_call(native_lib):
    L = native_lib.lib()
    one = ctypes.c_void_p(8)           # a non-null token; never dereferenced on these paths
    assert L.hnswgpu_exact_knn_filtered(None, one, 1, 1, one, one, one) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_exact_knn_filtered_dev(None, one, 1, 1, one, one, one, None) == -1
    assert L.hnswgpu_hnsw_search_filtered(None, one, 1, 1, 0, one, one, one, None) == -1
    assert L.hnswgpu_hnsw_search_filtered_dev(None, one, 1, 1, 0, one, one, one, None, None) == -1


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 1000])
def test_pack_mask(n):
    from hnsw_clj_amd.engine import pack_mask

    rng = np.random.default_rng(n)
    bits = rng.random(n) < 0.4
    bits[n - 1] = True
    for src in (bits, np.flatnonzero(bits), [int(i) for i in np.flatnonzero(bits)], iter(np.flatnonzero(bits).tolist())):
        m = pack_mask(src, n)
        assert m.dtype == np.uint32 and m.shape == ((n + 31) // 32,)
        for i in range(n):
            assert ((int(m[i >> 5]) >> (i & 31)) & 1) == int(bits[i]), (n, i)
        for i in range(n, 32 * len(m)):                       # padded with zeros to whole words
            assert ((int(m[i >> 5]) >> (i & 31)) & 1) == 0
    assert not pack_mask(np.zeros(n, bool), n).any() and not pack_mask([], n).any()
    assert int(sum(bin(int(w)).count("1") for w in pack_mask(np.ones(n, bool), n))) == n
    with pytest.raises(ValueError):
        pack_mask(np.ones(n + 1, bool), n)
    with pytest.raises(ValueError):
        pack_mask([n], n)


def test_filtered_plan_boundaries():
    from hnsw_clj_amd.ultra_fast import filtered_plan

    ceil = lambda a, b: -(-a // b)  # noqa: E731
    # nothing passes: scan
    assert filtered_plan(1000, 0, 10) == ("scan", 50)
    assert filtered_plan(1000, 0, 10, ef=200) == ("scan", 200)
    # one row past it, p = 1, is below every list length: still the scan (p <= ef')
    assert filtered_plan(1000, 1, 10)[0] == "scan"
    # ef_need > 1024, the list the take kernel can see: k = 10, p = 3000 -- n = 102,400 needs exactly 1024 entries
    assert ceil(3 * 10 * 102400, 3000) == 1024 and ceil(3 * 10 * 102401, 3000) == 1025
    assert filtered_plan(102401, 3000, 10) == ("scan", 1025)
    assert filtered_plan(102400, 3000, 10) == ("graph", 1024)
    # p <= ef': n = 1000, k = 10 -- 173 passing rows need a list of 174 entries, 174 rows one of 173
    assert ceil(30000, 173) == 174 and ceil(30000, 174) == 173
    assert filtered_plan(1000, 173, 10) == ("scan", 174)
    assert filtered_plan(1000, 174, 10) == ("graph", 173)
    # the caller's ef counts where it is the larger one, on both sides of p <= ef'
    assert filtered_plan(1000, 500, 10) == ("graph", 60)
    assert filtered_plan(1000, 500, 10, ef=200) == ("graph", 200)
    assert filtered_plan(1000, 500, 10, ef=500) == ("scan", 500)
    assert filtered_plan(1000, 501, 10, ef=500) == ("graph", 500)
    assert filtered_plan(1000, 1000, 10) == ("graph", 50)           # everything passes: ef = max(k, 50), 3k = 30 below it
    assert filtered_plan(1000, 1000, 100) == ("graph", 300)         # 3k is the reference's over-fetch
    # the headline set, k = 10: the boundary lies near 3 % selectivity (p^2 > 30 n from p = 968; ef_need <= 1024 from p = 914)
    assert filtered_plan(31173, 913, 10) == ("scan", 1025) and filtered_plan(31173, 914, 10) == ("scan", 1024)
    assert filtered_plan(31173, 967, 10) == ("scan", 968) and filtered_plan(31173, 968, 10) == ("graph", 967)


def test_supports_filtering():
    from hnsw_clj_amd import protocol

    assert protocol.supports_filtering(protocol.GpuHnswIndex(None)) is True
    assert protocol.supports_filtering(protocol.GpuIvfFlatIndex(None)) is False
    assert issubclass(protocol.GpuHnswIndex, protocol.FilterableIndex)
    assert not issubclass(protocol.GpuIvfFlatIndex, protocol.FilterableIndex)
    with pytest.raises(NotImplementedError):
        protocol.FilterableIndex().search_knn_filtered_star([0.0], 1, lambda i: True, None)
    # the default helper still serves an index without the protocol (protocol.clj:96-101)

    class Three(protocol.ANNIndex):
        def search_knn_star(self, query, k, mode):
            return [{"id": i, "distance": float(i)} for i in range(k)]

    assert [r["id"] for r in protocol.default_filtered_search(Three(), None, 2, lambda i: i % 2 == 1, None)] == [1, 3]
