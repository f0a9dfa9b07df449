"""hnswgpu_load's judgement of the 64-byte header (hnsw-clj_amd/csrc/persist.hip), and the numpy restatement of the file
layout checked against itself.  No GPU: the header is judged -- against the documented limits and against the size of the
file -- before the first HIP call, so every case here ends at that judgement."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_file as IF  # noqa: E402

EINVAL = -1
KMAXDEG = 64                      # kernels.hpp: kMaxDeg
BUILD_KNOWN = 1 | 2 | 4 | 8       # include/hnswgpu.h: HNSWGPU_BUILD_SEQUENTIAL | _HEURISTIC | _SYMMETRIC | _EXTEND


def _tiny(rs, n=6, dim=4, M=2, nlist=2):
    """Sections of a small, valid index: base, a graph (every node on layer 0, node 0 also on layer 1), two lists."""
    base = rs.standard_normal((n, dim)).astype(np.float32)
    levels = np.zeros(n, np.int32)
    levels[0] = 1
    l0 = np.full((n, 2 * M), -1, np.int32)
    for i in range(n):
        l0[i, 0], l0[i, 1] = (i + 1) % n, (i + n - 1) % n
    up_off = np.concatenate([[0], np.cumsum(levels)]).astype(np.int64)
    up_adj = np.full(int(up_off[-1]) * M, -1, np.int32)
    graph = dict(levels=levels, l0_adj=l0, up_off=up_off, up_adj=up_adj, M=M, entry=0, max_level=1)
    ivf = dict(centroids=rs.standard_normal((nlist, dim)).astype(np.float32),
               list_off=np.array([0, 4, n], np.int64), list_ids=rs.permutation(n).astype(np.int32))
    return base, graph, ivf


def test_numpy_writer_and_reader_agree(tmp_path):
    """write_index_file -> read_index_file gives back every section and header field, the size formula holds for the four
    combinations of sections, and a stated header field is written as stated."""
    rs = np.random.default_rng(3)
    base, graph, ivf = _tiny(rs)
    for name, sections, flags in (("bare", {}, 0), ("graph", graph, 1), ("ivf", ivf, 2), ("both", dict(graph, **ivf), 3)):
        path = str(tmp_path / (name + ".bin"))
        hdr = IF.write_index_file(path, base, 1, builder=2 if flags & 1 else 0, **sections)
        back = IF.read_index_file(path)
        assert back["size"] == os.path.getsize(path) == IF.expected_size(**hdr)
        assert (back["magic"], back["version"], back["metric"], back["n"], back["dim"], back["flags"]) == (b"HNSWGPU1", 1, 1, 6, 4, flags)
        assert back["base"].tobytes() == base.tobytes()
        if flags & 1:
            assert (back["M"], back["M0"], back["entry"], back["max_level"], back["up_blocks"], back["builder"]) == (2, 4, 0, 1, 1, 2)
            for key in ("levels", "l0_adj", "up_off", "up_adj"):
                np.testing.assert_array_equal(back[key], graph[key], err_msg=key)
                assert back[key].dtype == graph[key].dtype
        else:
            assert "levels" not in back and back["builder"] == 0
        if flags & 2:
            assert back["nlist"] == 2
            for key in ("centroids", "list_off", "list_ids"):
                np.testing.assert_array_equal(back[key], ivf[key], err_msg=key)
        else:
            assert "centroids" not in back and back["nlist"] == 0
    # the header bytes sit where the layout says (a reader in another language reads them by offset)
    raw = open(str(tmp_path / "both.bin"), "rb").read()
    assert raw[:8] == b"HNSWGPU1" and int.from_bytes(raw[16:24], "little") == 6 and int.from_bytes(raw[24:28], "little") == 4
    assert int.from_bytes(raw[48:56], "little") == 1 and int.from_bytes(raw[56:60], "little") == 2
    assert int.from_bytes(raw[60:64], "little") == 2
    off = IF.section_offsets(IF.unpack_header(raw))
    assert off["levels"] == 64 + 6 * 4 * 4 and off["end"] == len(raw)
    assert np.frombuffer(raw, "<i8", 3, off["list_off"]).tolist() == [0, 4, 6]
    # a stated field wins over the derived one, and the reader refuses what does not add up
    IF.write_index_file(str(tmp_path / "lie.bin"), base, 0, n=7)
    assert IF.unpack_header(open(str(tmp_path / "lie.bin"), "rb").read())["n"] == 7
    with pytest.raises(ValueError, match="implies"):
        IF.read_index_file(str(tmp_path / "lie.bin"))


def _header_cases(tmp_path):
    """name -> (path, message class).  Each file is valid except for what its name says."""
    rs = np.random.default_rng(5)
    base, graph, ivf = _tiny(rs)
    both = dict(graph, **ivf)
    cases = {}

    def case(name, want, sections, metric=0, cut=None, extra=b"", **header):
        path = str(tmp_path / (name.replace(" ", "_").replace(">", "gt").replace("<", "lt") + ".bin"))
        IF.write_index_file(path, base, metric, **dict(sections, **header))
        if cut is not None or extra:
            raw = open(path, "rb").read()
            open(path, "wb").write((raw if cut is None else raw[:cut]) + extra)
        cases[name] = (path, want)

    case("wrong magic", "not an HNSWGPU1 index file", both, magic=b"HNSWGPU2")
    case("version 2", "not an HNSWGPU1 index file", both, version=2)
    case("metric 3", "corrupt header", both, metric=3)
    case("n = -1", "corrupt header", both, n=-1)
    case("dim 0", "corrupt header", both, dim=0)
    case("dim 3073", "corrupt header", both, dim=3073)
    case("M above kMaxDeg", "corrupt header", both, M=KMAXDEG + 1)
    case("M0 above kMaxDeg", "corrupt header", both, M0=KMAXDEG + 1)
    case("graph flag with M = 0", "corrupt header", both, M=0)
    case("ivf flag with nlist = 0", "corrupt header", both, nlist=0)
    case("up_blocks > 31 n", "corrupt header", both, up_blocks=31 * 6 + 1)
    case("up_blocks < 0", "corrupt header", both, up_blocks=-1)
    case("a 40-byte file", "truncated", both, cut=40)
    case("a header alone", r"truncated: 64 bytes, its header implies %d\b" % IF.expected_size(6, 4, 3, 2, 4, 1, 2), both, cut=64)
    huge = 64 + (2 ** 31 - 2) * 3072 * 4
    case("n = 2^31 - 2, dim = 3072", r"truncated: 64 bytes, its header implies %d\b" % huge, {}, cut=64, n=2 ** 31 - 2, dim=3072)
    size = IF.expected_size(6, 4, 3, 2, 4, 1, 2)
    case("one byte too many", r"corrupt: %d bytes, its header implies %d\b" % (size + 1, size), both, extra=b"\0")
    # new with the builder word: the header is judged whole, unknown bits are not skipped
    case("flags bit 2", "corrupt header", both, flags=3 | 4)
    case("flags bit 31", "corrupt header", {}, flags=-2 ** 31)
    case("builder bit 4", "corrupt header", both, builder=16)
    case("builder word negative", "corrupt header", both, builder=-1)
    case("builder without a graph", "corrupt header", ivf, builder=2)
    case("builder qualifier without the heuristic", "corrupt header", both, builder=4)
    return cases


def test_load_judges_every_header_field(native_lib, tmp_path):
    """Table-driven over hnswgpu_load: the return code, the class of the message, and *out left null.  (The two header tests of
    test_abi_and_host.py stay; this table names every field and the messages.)"""
    import re

    L = native_lib.lib()
    cases = _header_cases(tmp_path)
    assert len(cases) == 22
    failed = []
    for name, (path, want) in cases.items():
        h = ctypes.c_void_p(None)
        rc = L.hnswgpu_load(path.encode(), 0, ctypes.byref(h))
        msg = L.hnswgpu_last_error().decode("utf-8", "replace")
        if h.value is not None:                  # (only a wrongly accepted file on a machine with a GPU gets here)
            L.hnswgpu_destroy(h)
        if not (rc == EINVAL and re.search(want, msg) and h.value is None):
            failed.append("%s: rc %d, out %s, message %r (want /%s/)" % (name, rc, h.value, msg, want))
    assert not failed, "\n".join(failed)


def test_known_builder_words_pass_the_header(native_lib, tmp_path):
    """The other side of the table: every word hnswgpu_hnsw_build_ex accepts passes the header's judgement.  Without a GPU
    that is all that can be seen of a good file, so the file is one byte short: the size check, which comes after the
    header's, must be what refuses it."""
    L = native_lib.lib()
    base, graph, _ = _tiny(np.random.default_rng(5))
    for word in (0, 1, 2, 3, 2 | 4, 2 | 8, 2 | 4 | 8, 1 | 2 | 4 | 8):
        assert word & ~BUILD_KNOWN == 0
        path = str(tmp_path / ("builder_%d.bin" % word))
        IF.write_index_file(path, base, 0, builder=word, **graph)
        raw = open(path, "rb").read()
        open(path, "wb").write(raw[:-1])
        h = ctypes.c_void_p(None)
        assert L.hnswgpu_load(path.encode(), 0, ctypes.byref(h)) == EINVAL and h.value is None
        assert b"truncated" in L.hnswgpu_last_error(), (word, L.hnswgpu_last_error())
