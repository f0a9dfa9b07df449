"""No-GPU checks of the range search: the C entry points validate their arguments before any HIP call; the host logic of
search_radius / search_radius_batch against a stubbed handle."""
import ctypes

import numpy as np


def test_range_entry_points_check_arguments_before_any_hip_call(native_lib):
    L = native_lib.lib()
    one = ctypes.c_void_p(8)           # a non-null token; never dereferenced on these paths
    assert L.hnswgpu_range_search(None, one, 1, one, 0, one, one, one, 4) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_range_search_dev(None, one, 1, one, 0, one, one, one, 4, None) == -1
    # the other checks need no handle's contents either: a fake non-null handle is never dereferenced before they fail
    for fn, tail in ((L.hnswgpu_range_search, ()), (L.hnswgpu_range_search_dev, (None,))):
        assert fn(one, one, -1, one, 0, one, one, one, 4, *tail) == -1          # nq < 0
        assert fn(one, one, 1, one, 2, one, one, one, 4, *tail) == -1           # unknown flag bits
        assert fn(one, one, 1, one, 0, one, one, one, -1, *tail) == -1          # cap < 0
        assert fn(one, one, 1, one, 0, one, one, None, 4, *tail) == -1          # exactly one output array
        assert fn(one, one, 1, one, 0, one, None, one, 4, *tail) == -1
        assert fn(one, one, 1, one, 0, one, None, None, 4, *tail) == -1         # count only takes cap == 0
        assert fn(one, None, 1, one, 0, one, one, one, 4, *tail) == -1          # null Q / radius / lims
        assert fn(one, one, 1, None, 0, one, one, one, 4, *tail) == -1
        assert fn(one, one, 1, one, 0, None, one, one, 4, *tail) == -1
        assert fn(one, None, 0, None, 1, None, None, None, 0, *tail) == 0       # no queries: nothing to do


class _StubIndex:
    n, dim = 6, 4

    def range_search(self, Q, radius, by_distance=False):
        self.call = (np.array(Q), radius, by_distance)
        return (np.array([0, 2, 2, 3], np.int64), np.array([4, 1, 0], np.int32), np.array([0.25, 0.5, 0.75], np.float32))


class _StubGraph:
    def __init__(self):
        self.index, self.ids = _StubIndex(), ["a", "b", "c", "d", "e", "f"]


def test_search_radius_formatting():
    from hnsw_clj_amd import ultra_fast

    g = _StubGraph()
    out = ultra_fast.search_radius_batch(g, np.zeros((3, 4), np.float32), 0.8)
    assert out == [[{"id": "e", "distance": 0.25}, {"id": "b", "distance": 0.5}], [], [{"id": "a", "distance": 0.75}]]
    assert g.index.call[1] == 0.8 and g.index.call[2] is True             # sorted on the device, not here
    assert ultra_fast.search_radius(g, np.zeros(4, np.float32), 0.8) == out[0] and g.index.call[0].shape == (1, 4)
    assert ultra_fast.search_radius_batch(g, np.zeros((0, 4), np.float32), 0.8) == []
    g.index.n = 0
    assert ultra_fast.search_radius_batch(g, np.zeros((2, 4), np.float32), 0.8) == [[], []] and ultra_fast.search_radius(g, np.zeros(4), 0.8) == []
