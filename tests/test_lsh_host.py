"""Hybrid LSH without a GPU: the numpy model (lsh_model.py) against examples worked by hand, java.util.Random's nextGaussian
in javarandom.hpp through a stand-alone program, the mirror's mode table and clamping, and the argument codes that need no
device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import lsh_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random(42).nextGaussian(), from the JDK's documented algorithm restated in Python (polar method, second value cached)
GAUSSIAN_42 = [1.141905315473055, 0.919407948982788, -0.9498666368908959, -1.1069902863993377]


def test_model_hash_and_buckets_by_hand():
    codes = M.hash_codes(M.HAND_ROWS, M.HAND_PLANES)
    assert np.array_equal(codes, M.HAND_CODES)
    assert np.array_equal(M.hash_codes(M.HAND_QUERY[None, :], M.HAND_PLANES), [[3, 3]])
    off, ids = M.buckets(codes, 2)
    assert off.tolist() == [[0, 0, 1, 4, 7], [0, 0, 0, 1, 7]]
    assert ids.tolist() == [[5, 3, 4, 6, 0, 1, 2], [2, 0, 1, 3, 4, 5, 6]]
    # a dot of exactly zero, of either sign, sets the bit (>= 0.0)
    assert M.codes_from_dots(np.array([[[0.0, -0.0, -1e-30, 1e-30]]])).tolist() == [[0b1011]]


def test_model_probe_order():
    assert M.probe_sequence([5, 6], 3, 2, 2) == [(0, 5, True), (0, 4, False), (0, 7, False), (1, 6, True), (1, 7, False), (1, 4, False)]
    assert M.probe_sequence([5, 6], 3, 9, 9) == [(0, 5, True), (0, 4, False), (0, 7, False), (0, 1, False),
                                                 (1, 6, True), (1, 7, False), (1, 4, False), (1, 2, False)]   # clamped to tables, bits
    assert M.probe_sequence([5, 6], 3, 1, 0) == [(0, 5, True)]


@pytest.mark.parametrize("case", M.HAND_CASES, ids=lambda c: "k%d_p%d_r%d_t%d_%d" % c[0])
def test_model_search_by_hand(case):
    (k, probes, radius, take_main, take_flip), want = case
    off, ids = M.buckets(M.HAND_CODES, 2)
    got = M.search(M.hand_distances(), [3, 3], off, ids, 2, k, probes, radius, take_main, take_flip)
    assert got == want


def test_truncation_comes_before_the_dedup():
    """The first hand case, against the tempting wrong statement: the k nearest DISTINCT rows of the probed buckets."""
    (k, probes, radius, take_main, take_flip), want = M.HAND_CASES[0]
    off, ids = M.buckets(M.HAND_CODES, 2)
    d = M.hand_distances()
    probed = sorted({int(r) for t, b, _ in M.probe_sequence([3, 3], 2, probes, radius) for r in ids[t, off[t, b]:off[t, b + 1]]},
                    key=lambda r: (d[r], r))
    assert probed[:k] == [0, 1, 4] and want == [0, 1]


def test_java_random_next_gaussian(tmp_path):
    src = tmp_path / "gauss.cpp"
    src.write_text('#include <stdio.h>\n#include "javarandom.hpp"\n'
                   'int main() { hg::JavaRandom r(42); for (int i = 0; i < 5; i++) printf("%.17g\\n", r.next_gaussian());\n'
                   '  hg::JavaRandom s(7); s.next_gaussian(); printf("%d\\n", s.next_int(1000)); return 0; }\n')
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "gauss"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "hnsw-clj_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    got = [float(x) for x in out[:5]]
    for g, w in zip(got, GAUSSIAN_42):
        assert abs(g - w) <= 1e-15 * abs(w), (g, w)
    # the cached second value does not advance the generator: the draw behind ONE nextGaussian is the draw behind the pair's
    # four or more next() calls -- an independent restatement agrees on it and on the fifth value
    from oracle import oracle as O

    O.build()
    r = O.JavaRandom(42)
    ref = [r.next_gaussian() for _ in range(5)]
    assert all(abs(g - w) <= 1e-15 * abs(w) for g, w in zip(got, ref))
    s = O.JavaRandom(7)
    s.next_gaussian()
    assert int(out[5]) == s.next_int(1000)


def test_mode_table_and_clamping():
    from hnsw_clj_amd import hybrid_lsh as H

    assert H.MODE_CONFIGS == M.MODES == {"turbo": (2, 1), "fast": (4, 1), "balanced": (6, 2), "accurate": (8, 3), "precise": (8, 4)}
    assert H.mode_config(None) == H.mode_config("balanced") == H.mode_config("no-such-mode") == (6, 2)    # :363-364
    assert (H.NUM_HASH_TABLES, H.NUM_HASH_BITS, H.PROJECTION_DIM, H.SEED) == (8, 12, 64, 42)
    assert H.clamp_probes(6, 2) == (6, 2)
    assert H.clamp_probes(20, 40) == (8, 12)
    assert H.clamp_probes(8, 4, tables=3, bits=2) == (3, 2)
    # what the model probes is what the clamped numbers say
    for probes, radius in [(1, 0), (6, 2), (20, 40)]:
        p, r = H.clamp_probes(probes, radius, tables=8, bits=12)
        assert len(M.probe_sequence([0] * 8, 12, probes, radius)) == p * (1 + r)


def test_protocol_type():
    from hnsw_clj_amd import protocol

    idx = protocol.GpuHybridLshIndex(None)
    assert idx.index_type_star() == "hybrid-lsh"
    assert protocol.supports_batch_search(idx) and not protocol.supports_persistence(idx) and not protocol.supports_filtering(idx)


def test_lsh_error_codes_without_gpu(native_lib):
    """A null handle is refused before any HIP call."""
    L = native_lib.lib()
    buf = (ctypes.c_float * 16)()
    out = (ctypes.c_int32 * 16)()
    assert L.hnswgpu_lsh_build(None, 8, 12, 64, 42) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_set_lsh(None, buf, 2, 2) == -1
    assert L.hnswgpu_lsh_sizes(None, None, None) == -1
    assert L.hnswgpu_lsh_get(None, None, None, None, None) == -1
    assert L.hnswgpu_lsh_hash(None, buf, 1, out) == -1
    assert L.hnswgpu_lsh_search(None, buf, 1, 1, 1, 0, 1, 1, out, buf) == -1
    assert L.hnswgpu_lsh_search_dev(None, buf, 1, 1, 1, 0, 1, 1, out, buf, None) == -1
    for name in ("hnswgpu_lsh_build", "hnswgpu_set_lsh", "hnswgpu_lsh_sizes", "hnswgpu_lsh_get", "hnswgpu_lsh_hash",
                 "hnswgpu_lsh_search", "hnswgpu_lsh_search_dev"):
        assert name in native_lib._SIGS
