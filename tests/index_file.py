"""The index file of hnswgpu_save / hnswgpu_load, restated in numpy from the layout comment at the top of
hnsw-clj_amd/csrc/persist.hip -- a helper of the tests, not a test, and a third party: it imports nothing of the product.

Little endian throughout.  64-byte header:

    offset  0  magic      8 bytes   b"HNSWGPU1"
            8  version    int32     1
           12  metric     int32     0 cosine, 1 L2, 2 dot
           16  n          int64
           24  dim        int32
           28  flags      int32     bit 0: graph section, bit 1: ivf section
           32  M          int32
           36  M0         int32
           40  entry      int32
           44  max_level  int32
           48  up_blocks  int64
           56  nlist      int32
           60  builder    int32     HNSWGPU_BUILD_* of the graph (0 without one)

then   base       n * dim float32 (unpadded rows)
       graph      levels[n] int32, l0_adj[n * M0] int32, up_off[n + 1] int64, up_adj[up_blocks * M] int32
       ivf        centroids[nlist * dim] float32, list_off[nlist + 1] int64, list_ids[n] int32
"""
import struct

import numpy as np

HEADER = struct.Struct("<8siiqiiiiiiqii")
HEADER_FIELDS = ("magic", "version", "metric", "n", "dim", "flags", "M", "M0", "entry", "max_level", "up_blocks", "nlist", "builder")
MAGIC = b"HNSWGPU1"
FLAG_GRAPH, FLAG_IVF = 1, 2
assert HEADER.size == 64


def pack_header(**fields):
    """The 64 header bytes; every field must be given (no default hides a value from the test that states it)."""
    assert set(fields) == set(HEADER_FIELDS), sorted(set(fields) ^ set(HEADER_FIELDS))
    return HEADER.pack(*(fields[f] for f in HEADER_FIELDS))


def unpack_header(raw):
    return dict(zip(HEADER_FIELDS, HEADER.unpack(bytes(raw[:64]))))


def expected_size(n, dim, flags, M, M0, up_blocks, nlist, **_):
    """Bytes of a well-formed file with this header."""
    sz = 64 + n * dim * 4
    if flags & FLAG_GRAPH:
        sz += n * 4 + n * M0 * 4 + (n + 1) * 8 + up_blocks * M * 4
    if flags & FLAG_IVF:
        sz += nlist * dim * 4 + (nlist + 1) * 8 + n * 4
    return sz


def section_offsets(hdr):
    """Byte offset of every section a header announces: {"base": .., "levels": .., "l0_adj": .., "up_off": .., "up_adj": ..,
    "centroids": .., "list_off": .., "list_ids": .., "end": ..} (the keys of absent sections are missing)."""
    n, dim = hdr["n"], hdr["dim"]
    out = {"base": 64}
    o = 64 + n * dim * 4
    if hdr["flags"] & FLAG_GRAPH:
        for name, size in (("levels", n * 4), ("l0_adj", n * hdr["M0"] * 4), ("up_off", (n + 1) * 8),
                           ("up_adj", hdr["up_blocks"] * hdr["M"] * 4)):
            out[name] = o
            o += size
    if hdr["flags"] & FLAG_IVF:
        for name, size in (("centroids", hdr["nlist"] * dim * 4), ("list_off", (hdr["nlist"] + 1) * 8), ("list_ids", n * 4)):
            out[name] = o
            o += size
    out["end"] = o
    return out


def read_index_file(path):
    """-> dict: the header fields, "base" (n, dim) float32, and, where the flags announce them, "levels", "l0_adj" (n, M0),
    "up_off", "up_adj" (up_blocks * M,), "centroids" (nlist, dim), "list_off", "list_ids"; "size" = bytes of the file.
    Raises ValueError on a file that is not laid out as its header says."""
    raw = open(path, "rb").read()
    if len(raw) < 64:
        raise ValueError("shorter than a header")
    out = unpack_header(raw)
    if out["magic"] != MAGIC or out["version"] != 1:
        raise ValueError("not an HNSWGPU1 file")
    off = section_offsets(out)
    if off["end"] != len(raw):
        raise ValueError("%d bytes, the header implies %d" % (len(raw), off["end"]))
    n, dim = out["n"], out["dim"]

    def arr(name, dtype, count):
        return np.frombuffer(raw, np.dtype(dtype).newbyteorder("<"), count, off[name]).astype(dtype)

    out["base"] = arr("base", np.float32, n * dim).reshape(n, dim)
    if out["flags"] & FLAG_GRAPH:
        out["levels"] = arr("levels", np.int32, n)
        out["l0_adj"] = arr("l0_adj", np.int32, n * out["M0"]).reshape(n, out["M0"])
        out["up_off"] = arr("up_off", np.int64, n + 1)
        out["up_adj"] = arr("up_adj", np.int32, out["up_blocks"] * out["M"])
    if out["flags"] & FLAG_IVF:
        out["centroids"] = arr("centroids", np.float32, out["nlist"] * dim).reshape(out["nlist"], dim)
        out["list_off"] = arr("list_off", np.int64, out["nlist"] + 1)
        out["list_ids"] = arr("list_ids", np.int32, n)
    out["size"] = len(raw)
    return out


def write_index_file(path, base, metric, levels=None, l0_adj=None, up_off=None, up_adj=None, M=0, entry=0, max_level=0,
                     centroids=None, list_off=None, list_ids=None, builder=0, **header):
    """Write the sections that are given.  Every header field is derived from them unless `header` states it (magic,
    version, n, dim, flags, M0, up_blocks, nlist; metric, M, entry, max_level and builder are arguments anyway): a test
    states a wrong one that way.  The body is written as given, whatever the header says."""
    base = np.ascontiguousarray(base, "<f4")
    graph, ivf = levels is not None, centroids is not None
    hdr = dict(magic=MAGIC, version=1, metric=metric, n=base.shape[0], dim=base.shape[1],
               flags=(FLAG_GRAPH if graph else 0) | (FLAG_IVF if ivf else 0), M=M, M0=0, entry=entry, max_level=max_level,
               up_blocks=0, nlist=0, builder=builder)
    body = [base.tobytes()]
    if graph:
        l0_adj = np.ascontiguousarray(l0_adj, "<i4")
        up_off = np.ascontiguousarray(up_off, "<i8")
        hdr["M0"] = l0_adj.shape[1] if l0_adj.ndim == 2 else 2 * M
        hdr["up_blocks"] = int(up_off[-1])
        body += [np.ascontiguousarray(levels, "<i4").tobytes(), l0_adj.tobytes(), up_off.tobytes(),
                 np.ascontiguousarray(up_adj, "<i4").tobytes()]
    if ivf:
        centroids = np.ascontiguousarray(centroids, "<f4")
        hdr["nlist"] = centroids.shape[0]
        body += [centroids.tobytes(), np.ascontiguousarray(list_off, "<i8").tobytes(),
                 np.ascontiguousarray(list_ids, "<i4").tobytes()]
    unknown = set(header) - set(HEADER_FIELDS)
    assert not unknown, unknown
    hdr.update(header)
    with open(path, "wb") as f:
        f.write(pack_header(**hdr))
        for b in body:
            f.write(b)
    return hdr
