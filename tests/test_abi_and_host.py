"""No-GPU checks of the product: the C-ABI library builds for gfx950, loads, and exports every symbol
include/hnswgpu.h declares; host-side logic of the Python mirror; the product never touches oracle/."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    hdr = open(os.path.join(ROOT, "include", "hnswgpu.h")).read()
    return sorted(set(re.findall(r"\b(hnswgpu_[a-z0-9_]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol(native_lib):
    L = ctypes.CDLL(native_lib.SO)
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(L, n), "libhnswgpu.so does not export %s" % n
    L.hnswgpu_version.restype = ctypes.c_int
    assert L.hnswgpu_version() == 104


def test_python_binding_covers_header(native_lib):
    assert set(native_lib.EXPORTS) == set(_declared())


def test_no_torch_types_or_oracle_in_product():
    pkg = os.path.join(ROOT, "hnsw-clj_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("oracle/oracle.c", "").replace("oracle.c", "") or f in ("kernels.hpp",), \
                    "%s mentions the oracle: the product must not depend on it" % f
                assert "import oracle" not in src and "from oracle" not in src
    hdr = open(os.path.join(ROOT, "include", "hnswgpu.h")).read()
    assert "torch" not in hdr.replace("torch tensor's", "") and "at::" not in hdr


def test_library_reads_no_environment_on_search_paths(native_lib):
    """The switches of rounds 1-3 were 45 HNSWGPU_* environment names, 20 of them read by getenv on every IVF search and two
    that made results wrong on purpose.  Now: hnswgpu_set_tuning for all of them, six documented names read once when the
    library is loaded, the ablation switches in -DHG_DIAG builds only (<= 10 strings, no getenv on the search
    path)."""
    import re
    import subprocess

    blob = open(native_lib.SO, "rb").read()
    names = sorted(set(m.decode() for m in re.findall(rb"HNSWGPU_[A-Z0-9_]+", blob)))
    env = {"HNSWGPU_BUILD_THREADS", "HNSWGPU_IVF_CALIBRATE", "HNSWGPU_IVF_HALF", "HNSWGPU_PREFETCH", "HNSWGPU_PREFILTER",
           "HNSWGPU_TILE_PAIRS"}
    api_constants_in_messages = {"HNSWGPU_BUILD_HEURISTIC", "HNSWGPU_BUILD_SYMMETRIC"}   # an error text names the flags
    assert env <= set(names) and set(names) <= env | api_constants_in_messages and len(names) <= 10, names
    assert b"STREAM_DBG" not in blob and b"TILE_DBG" not in blob and b"hnswgpu_debug_set_ablation" not in blob
    src = "".join(open(os.path.join(ROOT, "hnsw-clj_amd", "csrc", f)).read()
                  for f in os.listdir(os.path.join(ROOT, "hnsw-clj_amd", "csrc")) if f.endswith((".hip", ".hpp")))
    assert src.count("getenv(") == 1, "getenv belongs in engine.hip's load-time TuneInit only"
    nm = subprocess.run(["nm", "-D", "--defined-only", native_lib.SO], capture_output=True, text=True).stdout
    assert "hnswgpu_set_tuning" in nm and "hnswgpu_get_tuning" in nm


def test_tuning_table_roundtrip(native_lib):
    """hnswgpu_set_tuning / hnswgpu_get_tuning need no GPU: set, read back, restore the default, reject unknown keys; the
    header's key numbers are the wrapper's."""
    import re

    N = native_lib
    hdr = open(os.path.join(ROOT, "include", "hnswgpu.h")).read()
    keys = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define HNSWGPU_TUNE_([A-Z0-9_]+) (\d+) ", hdr))
    count = keys.pop("COUNT") if "COUNT" in keys else int(re.search(r"#define HNSWGPU_TUNE_COUNT (\d+)", hdr).group(1))
    assert [k for k, _ in sorted(keys.items(), key=lambda kv: kv[1])] == N.TUNE_KEYS and count == len(N.TUNE_KEYS)
    was = N.get_tuning("STREAM_CAP")
    N.set_tuning("stream_cap", 7)
    assert N.get_tuning("STREAM_CAP") == 7
    N.set_tuning("STREAM_CAP", None)
    assert N.get_tuning("STREAM_CAP") is None
    N.set_tuning("STREAM_CAP", was)
    assert N.lib().hnswgpu_set_tuning(count, 1) == -1 and N.lib().hnswgpu_set_tuning(-1, 1) == -1


def test_missing_library_fails_loudly(monkeypatch, native_lib):
    monkeypatch.setattr(native_lib, "SO", "/nonexistent/libhnswgpu.so")
    monkeypatch.setattr(native_lib, "_lib", None)
    with pytest.raises(ImportError, match="no CPU fallback"):
        native_lib.lib()


def test_error_codes_without_gpu(native_lib):
    """Argument validation happens before any HIP call, so it is testable here."""
    L = native_lib.lib()
    assert L.hnswgpu_create(None, 0, 4, 0, 0, None) != 0
    assert b"out is null" in L.hnswgpu_last_error()
    h = ctypes.c_void_p()
    assert L.hnswgpu_create(None, 5, 4, 0, 0, ctypes.byref(h)) == -1          # base null
    assert L.hnswgpu_create(None, 0, 4000, 0, 0, ctypes.byref(h)) == -5        # dim > 3072
    assert L.hnswgpu_create(None, 0, 4, 7, 0, ctypes.byref(h)) == -1           # unknown metric
    assert L.hnswgpu_destroy(None) == 0


def test_mirror_host_logic():
    from hnsw_clj_amd import ivf_flat, ultra_fast

    ids, base = ultra_fast._split([["a", [1, 2, 3]], ["b", np.array([4.0, 5.0, 6.0])]])
    assert ids == ["a", "b"] and base.dtype == np.float32 and base.shape == (2, 3)
    with pytest.raises(ValueError):
        ultra_fast._split([["a", [1, 2, 3]], ["b", [1, 2]]])
    with pytest.raises(ValueError, match="distance-fn"):
        ultra_fast._metric_of(lambda a, b: 0.0)
    assert ultra_fast.cosine_distance_ultra.metric == 0 and ultra_fast.euclidean_distance_ultra.metric == 1
    assert ivf_flat.MODE_CONFIGS["balanced"]["num_probes"] == 4      # ivf_flat.clj:243-247
    assert ivf_flat.MODE_CONFIGS["precise"]["num_probes"] == 12
    assert ivf_flat.MODE_CONFIGS["turbo"]["use_centroids"] is False


def test_shard_ranges():
    from hnsw_clj_amd.sharded import shard_range

    for n in (0, 1, 7, 31173, 10_000_000):
        for w in (1, 2, 3, 8):
            rs = [shard_range(n, r, w) for r in range(w)]
            assert rs[0][0] == 0 and rs[-1][1] == n
            assert all(rs[i][1] == rs[i + 1][0] for i in range(w - 1))
            sizes = [b - a for a, b in rs]
            assert max(sizes) - min(sizes) <= 1


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus N` without a launcher spawns N child ranks (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*),
    relays rank 0's single JSON line and returns the worst exit code -- the driver's invocation (no GPU needed here)."""
    import json
    import subprocess

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--launch-selftest"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    assert json.loads(lines[0]) == {"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "3", "MASTER_ADDR": "127.0.0.1"}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-selftest"],
                       env=dict(env, HNSWGPU_SELFTEST_FAIL_RANK="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 3                               # a failing rank fails the run
    # under torch.distributed.run (WORLD_SIZE set) it runs as the rank it is and spawns nothing
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-selftest"],
                       env=dict(env, RANK="1", WORLD_SIZE="2", LOCAL_RANK="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == ""


def test_bench_dump_outputs(tmp_path):
    """bench.py --dump-outputs: the last timed step's ids (float64, exact) and distances (float32) as .npy files; a batch
    whose results pass 64 MB is written as a fixed, sorted sample of query rows (the same rows on every run), indices
    beside it (no GPU needed: the tensors are the caller's)."""
    import torch

    import bench

    ids = torch.arange(50, dtype=torch.int32).reshape(5, 10) + (1 << 30)
    d = torch.linspace(0, 1, 50, dtype=torch.float32).reshape(5, 10)
    bench.dump_outputs(str(tmp_path / "a"), ids, d, 0, 1)
    got_i, got_d = np.load(tmp_path / "a" / "hnsw_ids.npy"), np.load(tmp_path / "a" / "hnsw_distances.npy")
    assert got_i.dtype == np.float64 and got_d.dtype == np.float32
    assert np.array_equal(got_i, ids.numpy()) and np.array_equal(got_d, d.numpy())
    assert not (tmp_path / "a" / "hnsw_rows.npy").exists()
    n = 600_000                                             # 600k x 10 results x 12 B = 72 MB
    ids = torch.arange(n * 10, dtype=torch.int32).reshape(n, 10)
    d = torch.zeros((n, 10), dtype=torch.float32)
    for sub in ("b", "c"):
        bench.dump_outputs(str(tmp_path / sub), ids, d, 1, 2)
    total = sum(f.stat().st_size for f in (tmp_path / "b").iterdir())
    assert 2 * total <= 64 << 20                            # two ranks' files within the limit
    rows = np.load(tmp_path / "b" / "hnsw_rows_rank1.npy")
    assert rows.dtype == np.float64 and (np.diff(rows) > 0).all() and rows[-1] < n
    assert np.array_equal(np.load(tmp_path / "b" / "hnsw_ids_rank1.npy"), ids.numpy()[rows.astype(np.int64)])
    assert np.array_equal(rows, np.load(tmp_path / "c" / "hnsw_rows_rank1.npy"))


def test_load_rejects_damaged_headers_before_touching_anything(native_lib, tmp_path):
    """hnswgpu_load validates the 64-byte header against the documented limits and against the file size BEFORE it
    sizes a single read from it (no GPU involved up to that point): garbage row counts, dims, degrees and list counts
    come back as HNSWGPU_EINVAL with a message -- never an overflowed size, a bad_alloc through the C boundary or an
    over-read."""
    import struct

    L = native_lib.lib()

    def header(n=10, dim=4, flags=0, M=0, M0=0, entry=0, max_level=0, up_blocks=0, nlist=0, metric=0, magic=b"HNSWGPU1", version=1):
        return struct.pack("<8siiqiiiiiiqii", magic, version, metric, n, dim, flags, M, M0, entry, max_level, up_blocks, nlist, 0)

    assert len(header()) == 64
    body = b"\0" * (10 * 4 * 4)
    cases = {
        "not an index": header(magic=b"NOTANIDX") + body,
        "rows": header(n=1 << 40) + body,
        "negative rows": header(n=-5) + body,
        "dim": header(dim=100000) + body,
        "degree": header(flags=1, M=16, M0=1000) + body,
        "up blocks": header(flags=1, M=16, M0=32, up_blocks=1 << 50) + body,
        "lists": header(flags=2, nlist=-3) + body,
        "metric": header(metric=9) + body,
        "short": header() + body[:-8],
        "long": header() + body + b"xx",
        "version": header(version=7) + body,
    }
    for name, blob in cases.items():
        path = str(tmp_path / (name.replace(" ", "_") + ".bin"))
        open(path, "wb").write(blob)
        h = ctypes.c_void_p(None)
        rc = L.hnswgpu_load(path.encode(), 0, ctypes.byref(h))
        assert rc == -1, "%s: rc %d (%s)" % (name, rc, L.hnswgpu_last_error())       # HNSWGPU_EINVAL
        assert h.value is None and L.hnswgpu_last_error()
    open(str(tmp_path / "tiny.bin"), "wb").write(b"HNSW")
    assert L.hnswgpu_load(str(tmp_path / "tiny.bin").encode(), 0, ctypes.byref(ctypes.c_void_p(None))) == -1


def test_multi_gpu_entry_points_validate_their_arguments(native_lib):
    """The entry points of the sharded IVF path refuse bad sizes and null pointers with a code and a message before any
    device call (so this runs without a GPU): nothing crosses the C boundary as a crash."""
    L = native_lib.lib()
    one = ctypes.c_void_p(8)           # a non-null token; never dereferenced on these paths
    assert L.hnswgpu_merge_keyed_dev(0, one, one, one, 0, 4, 10, one, one, None) == -1        # nshard < 1
    assert L.hnswgpu_merge_keyed_dev(0, one, one, one, 2, 4, 0, one, one, None) == -1         # k < 1
    assert L.hnswgpu_merge_keyed_dev(0, one, one, one, 2, 4, 2000, one, one, None) == -5      # k > 1024: HNSWGPU_ELIMIT
    assert b"1024" in L.hnswgpu_last_error()
    assert L.hnswgpu_merge_keyed_dev(0, one, one, one, 2, 0, 10, one, one, None) == 0         # no queries: nothing to do
    assert L.hnswgpu_merge_keyed_dev(0, None, one, one, 2, 4, 10, one, one, None) == -1       # null input
    assert L.hnswgpu_merge_topk_dev(0, one, one, 0, 4, 10, one, one, None) == -1
    assert L.hnswgpu_set_ivf_shard(None, one, 4, one, one, one) == -1                         # null handle / lengths
    assert L.hnswgpu_list_sums(None, 4, one, one, one) == -1
    assert L.hnswgpu_ivf_search_shard_dev(None, one, 1, 1, 1, one, one, one, None) == -1
