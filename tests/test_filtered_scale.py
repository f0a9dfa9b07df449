"""Filtered search where its kernels and host code split their work, against the unmodified oracle (ids identical, distance
bits identical; expectations built as test_filtered_search.py and test_ivf_filtered_search.py build them).

A. Masks past one compaction block: mask_count_kernel / mask_scatter_kernel take 1024 mask words (32,768 rows) per workgroup
   and mask_scan_kernel turns the workgroups' counts into the offsets blk[].  65,570 rows are 2,050 words: three workgroups,
   the last holding two words.  Each mask is chosen for what it does to blk[].
B. One handle of 1025 * 32768 + 37 rows: 1,026 compaction workgroups, so mask_scan_kernel's loop makes a second trip and carries
   its sum into it; and a mask with more than 2^20 passing rows under 513 queries, so the filtered exact scan runs its
   queries in more than one slice of its dense scratch.
C. Handles that changed: rows added by hnsw_add after a first, shorter filtered call has sized the filtered scratch, and a
   handle that came back from a file."""
import ctypes as C
import types

import numpy as np
import pytest

from test_filtered_search import _take
from test_ivf_filtered_search import _dev_mask, _expect, _garbage_past_n, _om
from util import assert_exact

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "l2", "dot"]
BLOCK = 32768                 # rows per compaction workgroup: 1024 words of 32 bits


def _nblk(n):
    return ((n + 31) // 32 + 1023) // 1024


def _expect_exact(O, base, Q, bits, om, k, nthreads=1):
    """O.exact_knn over base[pid], pid = flatnonzero(bits), ids mapped back through pid; -1 / +inf where fewer than k pass."""
    pid = np.flatnonzero(bits)
    oi, od, _ = O.exact_knn(base[pid], Q, k, metric=om, mode=O.MODE_DEV, nthreads=nthreads)
    return np.where(oi >= 0, pid[np.maximum(oi, 0)], -1).astype(np.int32), od


def _same_padding(gi, gd, ei, ed, what):
    assert np.array_equal(gi == -1, ei == -1), what + ": the -1 padding is not where the expectation has it"
    assert np.array_equal(np.isinf(gd), np.isinf(ed)), what + ": the +inf padding is not where the expectation has it"


def _run_exact(torch, idx, Q, Qd, nq, k, mask, md, side):
    """-> [(entry point, ids, distances)] of the host call and of the _dev call on a side stream"""
    gi, gd = idx.exact_knn_filtered(Q[:nq], k, mask)
    with torch.cuda.stream(side):
        di, dd = idx.exact_knn_filtered_dev(Qd[:nq], k, md)
    side.synchronize()
    return [("host", gi, gd), ("dev", di.cpu().numpy(), dd.cpu().numpy())]


# ---- A. three compaction workgroups ------------------------------------------------------------------------------------------
N_A, DIM_A, NLIST_A, NPROBE_A = 65570, 8, 32, 8
NQS = [1, 12, 33]
KS = [1, 10, 64, 100]         # 64: the last register list, 100: the first LDS list
NQ_MAX, K_MAX = 33, 100
MASKS_A = ["ones", "edges", "hole", "only_last_block", "half", "sparse", "list_edges"]
EDGE_ROWS = [0, BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK, N_A - 1]


def _bits_a(name, seed, lids):
    rng = np.random.default_rng(seed)
    b = np.zeros(N_A, np.bool_)
    if name == "ones":                # every block full
        b[:] = True
    elif name == "edges":             # the last bit of a block, the first of the next, the two-word tail block
        b[EDGE_ROWS] = True
    elif name == "hole":              # block 1 contributes 0: block 2's offset equals block 0's end
        b = rng.random(N_A) < 0.5
        b[BLOCK:2 * BLOCK] = False
    elif name == "only_last_block":   # blk[2] = 0 behind two empty blocks
        b[2 * BLOCK:] = True
    elif name == "half":
        b = rng.random(N_A) < 0.5
    elif name == "sparse":
        b = rng.random(N_A) < 0.03
    elif name == "list_edges":        # the block edges of the LIST-order mask, whatever the row ids there are
        b[lids[EDGE_ROWS]] = True
    return b


@pytest.fixture(scope="module")
def blocks3(native_lib, oracle):
    """65,570 x 8, 33 queries, 32 oracle-built lists (built once; every handle takes them as given), one handle per metric."""
    import torch

    from hnsw_clj_amd import datagen, engine

    O = oracle
    assert engine.device_count() >= 1, "no GPU visible"
    assert (N_A + 31) // 32 == 2050 and _nblk(N_A) == 3 and N_A & 31 == 2
    base = datagen.generate_dataset(N_A, DIM_A)
    Q = datagen.generate_dataset(NQ_MAX, DIM_A, seed=43)
    _, cen, assign = O.ivf_build_dev(base, NLIST_A, max_iterations=3, metric=O.COSINE)
    off, lids = O.lists_from_assign(assign, NLIST_A)
    handles = {}
    for metric in METRICS:
        handles[metric] = engine.Index(base, metric, 0)
        handles[metric].set_ivf(cen, off, lids)
    Qd = torch.from_numpy(Q).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    unfiltered = {}

    def unf(metric):                  # the unfiltered oracle search, once per metric
        if metric not in unfiltered:
            unfiltered[metric] = O.ivf_search(base, cen, off, lids, Q, K_MAX, NPROBE_A, metric=_om(O, metric), mode=O.MODE_DEV)
        return unfiltered[metric]

    yield types.SimpleNamespace(base=base, Q=Q, Qd=Qd, cen=cen, off=off, lids=lids, handles=handles, unfiltered=unf)
    for h in handles.values():
        h.close()


def _mask_a(engine, name, mi, lids):
    bits = _bits_a(name, 100 + mi, lids)
    mask = _garbage_past_n(engine.pack_mask(bits, N_A), N_A, 7 + mi)
    assert mask[-1] >> 2, "no garbage above n in the last word"
    return bits, mask


@pytest.mark.parametrize("name", MASKS_A)
def test_exact_knn_filtered_over_three_mask_blocks(blocks3, oracle, name):
    import torch

    from hnsw_clj_amd import engine

    O, s = oracle, blocks3
    mi = MASKS_A.index(name)
    metric = METRICS[mi % 3]
    idx = s.handles[metric]
    bits, mask = _mask_a(engine, name, mi, s.lids)
    p = int(bits.sum())
    if name in ("edges", "list_edges"):
        assert p == 6
    if name == "edges":               # ... and they are where the kernels split: words 0, 1023 | 1024, 2047 | 2048, 2049
        w = engine.pack_mask(bits, N_A)
        assert np.flatnonzero(w).tolist() == [0, 1023, 1024, 2047, 2048, 2049]
        assert [int(x) for x in w[[0, 1023, 1024, 2047, 2048, 2049]]] == [1, 1 << 31, 1, 1 << 31, 1, 2]
    if name == "hole":
        assert not bits[BLOCK:2 * BLOCK].any() and bits[:BLOCK].any() and bits[2 * BLOCK:].any()
    if name == "only_last_block":
        assert p == N_A - 2 * BLOCK == 34 and not bits[:2 * BLOCK].any()
    ei, ed = _expect_exact(O, s.base, s.Q, bits, _om(O, metric), K_MAX)
    md = _dev_mask(torch, mask)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for j, k in enumerate(KS):
        nq = NQS[(mi + j) % len(NQS)]
        for entry, gi, gd in _run_exact(torch, idx, s.Q, s.Qd, nq, k, mask, md, side):
            what = "%s mask %s (p %d) nq %d k %d %s" % (metric, name, p, nq, k, entry)
            assert_exact(gi, gd, ei[:nq, :k], ed[:nq, :k], what)
            _same_padding(gi, gd, ei[:nq, :k], ed[:nq, :k], what)
            assert bits[gi[gi >= 0]].all(), what + ": a failing row was returned"
            if k > p:
                assert (gi[:, :p] >= 0).all() and (gi[:, p:] == -1).all(), what
                assert all(sorted(r[:p]) == np.flatnonzero(bits).tolist() for r in gi), what + ": not every passing row came back"


@pytest.mark.parametrize("name", MASKS_A)
def test_ivf_search_filtered_over_three_mask_blocks(blocks3, oracle, name):
    """The compaction runs over the L = n list positions of the mask turned into list order."""
    import torch

    from hnsw_clj_amd import engine

    O, s = oracle, blocks3
    mi = MASKS_A.index(name)
    metric = METRICS[mi % 3]
    om = _om(O, metric)
    idx = s.handles[metric]
    bits, mask = _mask_a(engine, name, mi, s.lids)
    p = int(bits.sum())
    ui, ud, uprobes = s.unfiltered(metric)
    ei, ed, epr, _ = _expect(O, s.base, s.cen, s.off, s.lids, s.Q, bits, NPROBE_A, om)
    assert np.array_equal(epr, uprobes), "the oracle's routing saw the mask"
    if name == "ones":
        assert np.array_equal(ui, ei) and np.array_equal(ud, ed, equal_nan=True)
    keep = bits[s.lids]                                                # the mask in list order
    if name == "list_edges":
        assert np.flatnonzero(keep).tolist() == EDGE_ROWS
    per_list = np.diff(np.concatenate([[0], np.cumsum(keep)])[s.off])  # passing rows of every list
    probed_empty = int((per_list[uprobes] == 0).sum())
    if name in ("edges", "list_edges"):   # 6 passing rows: at most 6 of the 8 lists a query probes hold one
        assert probed_empty >= 2 * NQ_MAX, "no probed list is left without a passing row"
    md = _dev_mask(torch, mask)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for j, k in enumerate(KS):
        nq = NQS[(mi + j) % len(NQS)]
        what = "%s mask %s (p %d) nq %d k %d" % (metric, name, p, nq, k)
        gi, gd, gp = idx.ivf_search_filtered(s.Q[:nq], k, NPROBE_A, mask, want_probes=True)
        assert np.array_equal(gp, uprobes[:nq]), what + ": probes"
        with torch.cuda.stream(side):
            di, dd = idx.ivf_search_filtered_dev(s.Qd[:nq], k, NPROBE_A, md)
        side.synchronize()
        for entry, ri, rd in (("host", gi, gd), ("dev", di.cpu().numpy(), dd.cpu().numpy())):
            assert_exact(ri, rd, ei[:nq, :k], ed[:nq, :k], what + " " + entry)
            _same_padding(ri, rd, ei[:nq, :k], ed[:nq, :k], what + " " + entry)
            assert bits[ri[ri >= 0]].all(), what + " " + entry + ": a failing row was returned"


# ---- B. one large handle ---------------------------------------------------------------------------------------------------
N_B, DIM_B = 1025 * BLOCK + 37, 4


@pytest.fixture(scope="module")
def large(native_lib, oracle):
    """33,587,237 x 4 (0.5 GB on the device), l2.  Rows from numpy's generator: the Java-compatible one is too slow here."""
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    assert _nblk(N_B) == 1026 and N_B & 31 == 5
    base = np.random.default_rng(0).random((N_B, DIM_B), dtype=np.float32)
    idx = engine.Index(base, "l2", 0)
    yield idx, base
    idx.close()


def test_mask_scan_carries_past_1024_blocks(large, oracle):
    """mask_scan_kernel scans 1024 block counts per trip: blocks 1024 and 1025 get their offsets in the second trip, from the
    sum the first one carried over."""
    import torch

    from hnsw_clj_amd import engine

    O = oracle
    idx, base = large
    rng = np.random.default_rng(1)
    rows = [0, BLOCK - 1, BLOCK, 1023 * BLOCK - 1, 1023 * BLOCK, 1024 * BLOCK - 1, 1024 * BLOCK, 1024 * BLOCK + 1, 1025 * BLOCK, N_B - 1]
    bits = np.zeros(N_B, np.bool_)
    bits[rows] = True
    bits[rng.choice(N_B, 300, replace=False)] = True
    pid = np.flatnonzero(bits)
    p = len(pid)
    assert 300 <= p <= 310 and (pid >= 1024 * BLOCK).sum() >= 4 and (pid < 1024 * BLOCK).sum() >= 6
    mask = _garbage_past_n(engine.pack_mask(bits, N_B), N_B, 11)
    assert mask[-1] >> 5, "no garbage above n in the last word"
    Q = rng.random((12, DIM_B), dtype=np.float32)
    dev = torch.device("cuda", 0)
    Qd, md = torch.from_numpy(Q).to(dev), _dev_mask(torch, mask)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for k in (10, 512):               # 512 > p: every passing row id comes back, those of blocks 1024 and 1025 included
        ei, ed = _expect_exact(O, base, Q, bits, O.L2, k)
        for entry, gi, gd in _run_exact(torch, idx, Q, Qd, 12, k, mask, md, side):
            what = "k %d %s" % (k, entry)
            assert_exact(gi, gd, ei, ed, what)
            _same_padding(gi, gd, ei, ed, what)
            assert bits[gi[gi >= 0]].all(), what + ": a failing row was returned"
            if k > p:
                assert (gi[:, p:] == -1).all() and np.isinf(gd[:, p:]).all(), what
                assert all(np.array_equal(np.sort(r[:p]), pid) for r in gi), what + ": not every passing row came back"


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_filtered_exact_scan_in_query_slices(large, oracle, metric):
    """filtered_chain bounds the single-mask form's dense [queries][passing rows] scratch to 2 GiB: with p >= 2^20 passing rows a slice
    holds at most 512 queries, so 513 queries run in more than one slice, and every slice offsets the padded queries, their
    norms and the result arrays by its first query.  The 513 queries are three distinct ones of three different norms: every
    result row equals the oracle's for the query it repeats, wherever the slices are cut.  Two orders: the three repeated
    cyclically, and an order that differs from itself shifted by s for every s in 1 .. 512 -- a slice that starts at a
    multiple of three finds the right queries at the start of a cyclic batch too, in this order a slice that reads its
    queries from anywhere but its own offset returns another query's bits.  l2 reads no query norm (filtered_group_kernel
    takes q_norms for cosine only), so a cosine handle over the same rows runs the same cases."""
    import torch

    from hnsw_clj_amd import engine

    O = oracle
    om = _om(O, metric)
    l2_idx, base = large
    nq, k = 513, 10
    bits = np.zeros(N_B, np.bool_)
    bits[::32] = True
    p = int(bits.sum())
    assert p == 1049602 and p >= 1 << 20 and nq > (2 << 30) // (4 << 20)   # 2 GiB / (4 bytes x 2^20 rows) = 512 queries
    mask = _garbage_past_n(engine.pack_mask(bits, N_B), N_B, 12)
    Q3 = base[np.sort(np.random.default_rng(2).choice(N_B, 3, replace=False))].copy()
    Q3 *= np.array([[1.0], [2.0], [0.5]], np.float32)
    assert len(np.unique(Q3, axis=0)) == 3 and len(np.unique(np.linalg.norm(Q3, axis=1))) == 3
    ei, ed = _expect_exact(O, base, Q3, bits, om, k, nthreads=3)
    assert len(np.unique(ei[:, 0])) == 3, "the three queries are not told apart by their results"
    cyclic = np.arange(nq) % 3
    aperiodic = np.random.default_rng(5).integers(0, 3, nq)
    assert all((aperiodic[s:] != aperiodic[:nq - s]).any() for s in range(1, nq)), "the order repeats itself under a shift"
    dev = torch.device("cuda", 0)
    md = _dev_mask(torch, mask)
    side = torch.cuda.Stream()
    idx = l2_idx if metric == "l2" else engine.Index(base, metric, 0)
    try:
        for order, rep in (("cyclic", cyclic), ("aperiodic", aperiodic)):
            Q = np.ascontiguousarray(Q3[rep])
            Qd = torch.from_numpy(Q).to(dev)
            torch.cuda.synchronize()
            # The gathered scan is the only launch of this call timed under PROF_IVF_SCAN, once per slice (filtered_chain):
            # the count of timed launches is the number of slices.  Should anything else come to be timed there, count anew.
            idx.set_profiling(True)
            idx.get_profile(engine.PROF_IVF_SCAN, reset=True)
            try:
                gi, gd = idx.exact_knn_filtered(Q, k, mask)
                _, slices = idx.get_profile(engine.PROF_IVF_SCAN, reset=True)
            finally:
                idx.set_profiling(False)
            assert slices >= 2, "the %d queries ran in %d slice(s)" % (nq, slices)
            assert_exact(gi, gd, ei[rep], ed[rep], "%s, 513 queries, %s, host" % (metric, order))
            with torch.cuda.stream(side):
                di, dd = idx.exact_knn_filtered_dev(Qd, k, md)
            side.synchronize()
            assert_exact(di.cpu().numpy(), dd.cpu().numpy(), ei[rep], ed[rep], "%s, 513 queries, %s, dev" % (metric, order))
        Q3d = torch.from_numpy(Q3).to(dev)
        torch.cuda.synchronize()
        for q in range(3):            # a query's bits never depend on its batch
            for entry, si, sd in _run_exact(torch, idx, Q3[q:q + 1], Q3d[q:q + 1], 1, k, mask, md, side):
                assert_exact(si, sd, ei[q:q + 1], ed[q:q + 1], "%s, query %d alone, %s" % (metric, q, entry))
    finally:
        if idx is not l2_idx:
            idx.close()


# ---- C. handles that changed -------------------------------------------------------------------------------------------------
def _handle_n(idx):
    from hnsw_clj_amd import _native

    n = C.c_int64(-1)
    _native.check(_native.lib().hnswgpu_info(idx._h, C.byref(n), None, None, None, None))
    return n.value


def _check_exact_filtered(torch, O, idx, base, Q, Qd, bits, om, ks, nqs, what, seed=3):
    """exact_knn_filtered, host and _dev, against the oracle over the passing rows of base[:idx.n] -> {(nq, k, entry): result}"""
    from hnsw_clj_amd import engine

    n = idx.n
    p = int(bits.sum())
    mask = _garbage_past_n(engine.pack_mask(bits, n), n, seed)
    md = _dev_mask(torch, mask)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ei, ed = _expect_exact(O, base[:n], Q, bits, om, max(ks))
    got = {}
    for k in ks:
        for nq in nqs:
            for entry, gi, gd in _run_exact(torch, idx, Q, Qd, nq, k, mask, md, side):
                w = "%s: exact, n %d p %d nq %d k %d %s" % (what, n, p, nq, k, entry)
                assert_exact(gi, gd, ei[:nq, :k], ed[:nq, :k], w)
                assert bits[gi[gi >= 0]].all(), w + ": a failing row was returned"
                if k >= p:            # exactly the passing rows, padded
                    assert all(sorted(r[:p]) == np.flatnonzero(bits).tolist() for r in gi), w
                    assert (gi[:, p:] == -1).all() and np.isinf(gd[:, p:]).all(), w
                got[(nq, k, entry)] = (gi, gd)
    return got


def _check_hnsw_filtered(torch, O, idx, base, g, Q, Qd, bits, om, ks, nqs, efs, what, seed=4):
    """hnsw_search_filtered, host and _dev, against _take over the oracle's unfiltered list on the graph g, stats included"""
    from hnsw_clj_amd import engine

    n = idx.n
    mask = _garbage_past_n(engine.pack_mask(bits, n), n, seed)
    md = _dev_mask(torch, mask)
    side = torch.cuda.Stream()
    got = {}
    for ef in efs:
        kk = min(ef, 1024)
        oi, od, ost, _ = O.hnsw_search(base[:n], g, Q, kk, ef=ef, metric=om, mode=O.MODE_DEV)
        for k in ks:
            ei, ed, _ = _take(oi, od, bits, k)
            for nq in nqs:
                w = "%s: hnsw, n %d nq %d k %d ef %d" % (what, n, nq, k, ef)
                gi, gd, gs = idx.hnsw_search_filtered(Q[:nq], k, mask, ef, want_stats=True)
                assert_exact(gi, gd, ei[:nq], ed[:nq], w + " host")
                assert np.array_equal(gs, ost[:nq]), w + " host: stats"
                stats = torch.zeros((nq, 2), dtype=torch.int64, device=Qd.device)
                torch.cuda.synchronize()
                with torch.cuda.stream(side):
                    di, dd = idx.hnsw_search_filtered_dev(Qd[:nq], k, md, ef, stats=stats)
                side.synchronize()
                assert_exact(di.cpu().numpy(), dd.cpu().numpy(), ei[:nq], ed[:nq], w + " dev")
                assert np.array_equal(stats.cpu().numpy(), ost[:nq]), w + " dev: stats"
                assert bits[gi[gi >= 0]].all(), w + ": a failing row was returned"
                got[(nq, k, ef, "host")] = (gi, gd)
                got[(nq, k, ef, "dev")] = (di.cpu().numpy(), dd.cpu().numpy())
    return got


def _check_ivf_filtered(torch, O, idx, base, lists, Q, Qd, bits, om, nprobe, ks, nqs, what, seed=5):
    """ivf_search_filtered, host and _dev, against the oracle over the lists restricted to the passing rows"""
    from hnsw_clj_amd import engine

    n = idx.n
    cen, off, lids = lists
    mask = _garbage_past_n(engine.pack_mask(bits, n), n, seed)
    md = _dev_mask(torch, mask)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    _, _, uprobes = O.ivf_search(base[:n], cen, off, lids, Q, 1, nprobe, metric=om, mode=O.MODE_DEV)
    ei, ed, _, _ = _expect(O, base[:n], cen, off, lids, Q, bits, nprobe, om, k=max(ks))
    got = {}
    for k in ks:
        for nq in nqs:
            w = "%s: ivf, n %d nq %d k %d" % (what, n, nq, k)
            gi, gd, gp = idx.ivf_search_filtered(Q[:nq], k, nprobe, mask, want_probes=True)
            assert np.array_equal(gp, uprobes[:nq]), w + ": probes"
            with torch.cuda.stream(side):
                di, dd = idx.ivf_search_filtered_dev(Qd[:nq], k, nprobe, md)
            side.synchronize()
            for entry, ri, rd in (("host", gi, gd), ("dev", di.cpu().numpy(), dd.cpu().numpy())):
                assert_exact(ri, rd, ei[:nq, :k], ed[:nq, :k], w + " " + entry)
                assert bits[ri[ri >= 0]].all(), w + " " + entry + ": a failing row was returned"
                got[(nq, k, entry)] = (ri, rd)
    return got


@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("dim", [24, 30])     # ld == dim / ld = 32: padded rows
def test_filtered_search_on_a_grown_handle(native_lib, oracle, dim, metric):
    """include/hnswgpu.h: "after hnswgpu_hnsw_add the next call simply brings a longer mask".  The first filtered calls come
    BEFORE the first hnsw_add and size the filtered scratch for 500 rows; hnsw_add then replaces d_base / d_norms and grows n
    by 1, 31 and 64 rows (16 -> 16 -> 17 -> 19 mask words, n & 31 != 0 throughout)."""
    import torch

    from hnsw_clj_amd import datagen, engine

    O = oracle
    om = _om(O, metric)
    n0, adds = 500, (1, 31, 64)
    n1 = n0 + sum(adds)
    assert n1 == 596 and n1 & 31 and (n0 + 31) // 32 < (n1 + 31) // 32
    base = datagen.generate_dataset(n1, dim)
    Q = datagen.generate_dataset(33, dim, seed=43)
    Qd = torch.from_numpy(Q).to(torch.device("cuda", 0))
    rng = np.random.default_rng(dim)
    with engine.Index(base[:n0], metric, 0) as idx:
        idx.hnsw_build(8, 40, 42)

        def check(what, added):
            n = idx.n
            g = idx.get_graph()
            assert _handle_n(idx) == n and g.n == n
            np.testing.assert_array_equal(idx.norms().view(np.uint32), O.norms(base[:n], O.MODE_DEV).view(np.uint32), err_msg=what)
            tail = np.arange(max(n - 70, 0), n, dtype=np.int32)       # the newest rows, and the old ones just below them
            want = np.array([O.distance_dev(om, Q[0], base[i]) for i in tail], np.float32)
            np.testing.assert_array_equal(idx.batch_distances(Q[0], tail).view(np.uint32), want.view(np.uint32), err_msg=what)
            ui, ud = idx.exact_knn(Q[:12], 10)
            oi, od, _ = O.exact_knn(base[:n], Q[:12], 10, metric=om, mode=O.MODE_DEV)
            assert_exact(ui, ud, oi, od, what + ": exact_knn")
            some_old = rng.random(n) < 0.3                              # some old rows and every added one
            some_old[n0:] = True
            only_new = np.zeros(n, np.bool_)
            only_new[n0:] = True
            for name, bits in (("some old and all new", some_old), ("only the added rows", only_new)):
                if not bits.any():
                    continue                                            # (before the first add there is no added row)
                w = "%s, mask %s" % (what, name)
                ex = _check_exact_filtered(torch, O, idx, base, Q, Qd, bits, om, [10, 100], [1, 33], w)
                hn = _check_hnsw_filtered(torch, O, idx, base, g, Q, Qd, bits, om, [10], [1, 33], [50, 1500], w)
                if name == "only the added rows":
                    for (nq, k, entry), (gi, gd) in ex.items():
                        if k >= added:
                            assert (np.sort(gi[:, :added], axis=1) == np.arange(n0, n)).all() and (gi[:, added:] == -1).all(), w
                    for (gi, gd) in hn.values():
                        assert ((gi == -1) | (gi >= n0)).all(), w

        check("before the first add", 0)                                # the filtered scratch is now sized for 500 rows
        n = n0
        for m in adds:
            ids = idx.hnsw_add(base[n:n + m], 40, 42)
            assert ids[0] == n and len(ids) == m
            n += m
            assert idx.n == n
            check("after adding %d rows" % (n - n0), n - n0)
        assert n == n1
        idx.ivf_build(8, 3, 42)                                         # lists over all 596 rows, as the handle reports them
        lists = idx.get_ivf()
        assert lists[1][-1] == n1 and sorted(lists[2].tolist()) == list(range(n1))
        for name, bits in (("half", rng.random(n1) < 0.5), ("only the added rows", np.arange(n1) >= n0)):
            _check_ivf_filtered(torch, O, idx, base, lists, Q, Qd, bits, om, 4, [10, 100], [1, 33], "grown handle, mask " + name)


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_filtered_search_on_a_reloaded_handle(native_lib, oracle, tmp_path, metric):
    """A handle that came back from hnswgpu_load serves the three filtered searches with the oracle's bits, which are the
    bits of the handle that was saved."""
    import torch

    from hnsw_clj_amd import datagen, engine

    O = oracle
    om = _om(O, metric)
    n, dim = 1000, 30
    base = datagen.generate_dataset(n, dim)
    Q = datagen.generate_dataset(33, dim, seed=43)
    Qd = torch.from_numpy(Q).to(torch.device("cuda", 0))
    path = str(tmp_path / "index.bin")
    with engine.Index(base, metric, 0) as idx:
        idx.hnsw_build(8, 40, 42)
        idx.ivf_build(8, 3, 42)
        g, lists = idx.get_graph(), idx.get_ivf()
        idx.save(path)
        with engine.Index.load(path, 0) as back:
            assert (back.n, back.dim, back.metric) == (n, dim, idx.metric) and back.nlist == 8 and back.has_graph
            g2, lists2 = back.get_graph(), back.get_ivf()
            for a, b in zip((g.levels, g.l0_adj, g.up_off, g.up_adj) + tuple(lists), (g2.levels, g2.l0_adj, g2.up_off, g2.up_adj) + tuple(lists2)):
                np.testing.assert_array_equal(a, b)
            assert (g.entry, g.max_level, g.M) == (g2.entry, g2.max_level, g2.M)
            for name, density in (("half", 0.5), ("sparse", 0.03)):
                bits = np.random.default_rng(int(density * 100)).random(n) < density
                got = []
                for what, h in (("saved", idx), ("loaded", back)):      # each against the oracle ...
                    w = "%s handle, mask %s" % (what, name)
                    got.append((_check_exact_filtered(torch, O, h, base, Q, Qd, bits, om, [10, 100], [1, 33], w),
                                _check_hnsw_filtered(torch, O, h, base, g, Q, Qd, bits, om, [10, 100], [1, 33], [200], w),
                                _check_ivf_filtered(torch, O, h, base, lists, Q, Qd, bits, om, 4, [10, 100], [1, 33], w)))
                for mine, theirs in zip(*got):                          # ... and so against each other, stated
                    assert mine.keys() == theirs.keys()
                    for key in mine:
                        assert np.array_equal(mine[key][0], theirs[key][0]), (name, key)
                        assert np.array_equal(mine[key][1].view(np.uint32), theirs[key][1].view(np.uint32)), (name, key)
