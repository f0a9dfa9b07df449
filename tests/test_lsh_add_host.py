"""hnswgpu_lsh_add without a GPU: the symbol is exported, bound and declared, a null handle is refused before any HIP call, and
the mirror's add_vectors does not touch the device for empty data."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_bound_and_declared(native_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", native_lib.SO], capture_output=True, text=True, check=True).stdout
    assert re.search(r"^[0-9a-f]+ T hnswgpu_lsh_add$", nm, re.M), "hnswgpu_lsh_add is not an exported function"
    assert "hnswgpu_lsh_add" in native_lib.EXPORTS
    assert native_lib._SIGS["hnswgpu_lsh_add"] == ["p", "p", "i64"]
    with open(os.path.join(ROOT, "include", "hnswgpu.h")) as f:
        hdr = f.read()
    assert re.search(r"^int hnswgpu_lsh_add\(hnswgpu_index \*idx, const float \*rows, int64_t m\);$", hdr, re.M)


def test_null_handle_is_refused_without_gpu(native_lib):
    L = native_lib.lib()
    buf = (ctypes.c_float * 16)()
    assert L.hnswgpu_lsh_add(None, buf, 1) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_lsh_add(None, buf, 0) == -1          # the handle comes before m == 0
    assert L.hnswgpu_lsh_add(None, None, -1) == -1


class _NoDevice:
    """In the handle's place: any call at all is a failure."""

    def __getattr__(self, name):
        raise AssertionError("add_vectors with empty data touched the handle (%s)" % name)


def test_mirror_add_vectors_with_empty_data_calls_nothing():
    from hnsw_clj_amd import hybrid_lsh as H

    index = H.HybridIndex(_NoDevice(), ["a", "b"], H.cosine_distance_ultra)
    assert H.add_vectors(index, []) is index
    assert index.ids == ["a", "b"]
    assert "no add" in H.add_vectors.__doc__ and "105-129" in H.add_vectors.__doc__


def test_engine_binding_exists():
    from hnsw_clj_amd import engine

    assert callable(engine.Index.lsh_add)
