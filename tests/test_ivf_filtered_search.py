"""IVF-FLAT filtered search on the device against the unmodified oracle (ids identical, distance bits identical).

Expected, with pid = flatnonzero(bits): every list restricted to its passing rows, renumbered into base[pid], the centroids
kept -- O.ivf_search(base[pid], cen, off', lids', Q, K_MAX, nprobe, metric, MODE_DEV), ids mapped back through pid.  That is the
oracle's full candidate stream with the failing rows dropped, first K.  One expectation per (shape, metric, mask) at the largest
nq and k: a smaller nq is a prefix of its rows, a smaller k a prefix of its columns.  Lists that become empty are legal."""
import numpy as np
import pytest

from util import assert_exact

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "l2", "dot"]
# (n, dim, nlist, nprobe): lists shorter than a wave's rows in flight / the ordinary case / every list probed / 157 mask words
# in ONE compaction block (of 1024 words; several blocks: test_filtered_scale.py) and empty filtered lists / the widest row loaders
SHAPES = [(33, 7, 3, 2), (1000, 128, 16, 4), (300, 768, 7, 7), (5000, 96, 64, 8), (70, 1536, 4, 2), (70, 3072, 4, 2)]
MASKS = ["ones", "zeros", "last", "every32", "half", "sparse", "one_list", "hand"]
NQS = [1, 12, 70]
KS = [1, 10, 64, 100]         # 64: the last register list, 100: the first LDS list
NQ_MAX, K_MAX = 70, 100


def _om(O, metric):
    return {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]


def _lists(O, base, nlist, om):
    _, cen, assign = O.ivf_build_dev(base, nlist, max_iterations=3, metric=om)
    off, lids = O.lists_from_assign(assign, nlist)
    return cen, off, lids


def _bits(name, n, seed, off, lids, probes0):
    rng = np.random.default_rng(seed)
    b = np.zeros(n, np.bool_)
    if name == "ones":
        b[:] = True
    elif name == "last":
        b[n - 1] = True
    elif name == "every32":
        b[::32] = True
    elif name == "half":
        b = rng.random(n) < 0.5
    elif name == "sparse":
        b = rng.random(n) < 0.03
    elif name == "one_list":          # exactly the rows of the list query 0 probes first
        l = int(probes0[0])
        b[lids[off[l]:off[l + 1]]] = True
    elif name == "hand":              # 1, 8 and 9 passing rows in lists query 0 probes: the rows-in-flight boundary, the clamped lane
        for l, c in zip(probes0[:3], (1, 8, 9)):
            b[lids[off[l]:off[l + 1]][:c]] = True
    return b


def _garbage_past_n(mask, n, seed):
    """Random bits at the positions >= n of the last word: the library must ignore them."""
    m = mask.copy()
    if n & 31:
        g = np.random.default_rng(seed).integers(0, 1 << 32, dtype=np.uint64)
        m[-1] |= np.uint32((int(g) >> (n & 31)) << (n & 31) & 0xFFFFFFFF)
    return m


def _expect(O, base, cen, off, lids, Q, bits, nprobe, om, k=K_MAX):
    """-> ids, distances, probes (None when nothing passes: the oracle is not asked about an empty base), empty lists"""
    nq, nlist = len(Q), len(off) - 1
    pid = np.flatnonzero(bits)
    if len(pid) == 0:
        return np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf, np.float64), None, nlist
    keep = bits[lids]                                                # per list position
    lids2 = np.searchsorted(pid, lids[keep]).astype(np.int32)       # passing rows renumbered into base[pid], list order kept
    off2 = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)[off]   # passing positions below every list's first
    oi, od, pr = O.ivf_search(base[pid], cen, off2, lids2, Q, k, nprobe, metric=om, mode=O.MODE_DEV)
    ids = np.where(oi >= 0, pid[np.maximum(oi, 0)], -1).astype(np.int32)
    return ids, od, pr, int((np.diff(off2) == 0).sum())


def _dev_mask(torch, mask):
    return torch.from_numpy(mask.view(np.int32).copy()).to(torch.device("cuda", 0))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("metric", METRICS)
def test_ivf_search_filtered_matches_the_oracle_on_the_passing_rows(native_lib, oracle, metric, shape):
    import torch

    from hnsw_clj_amd import datagen, engine

    O = oracle
    om = _om(O, metric)
    n, dim, nlist, nprobe = shape
    base = datagen.generate_dataset(n, dim)
    Q = datagen.generate_dataset(NQ_MAX, dim, seed=43)
    cen, off, lids = _lists(O, base, nlist, om)
    ui, ud, uprobes = O.ivf_search(base, cen, off, lids, Q, K_MAX, nprobe, metric=om, mode=O.MODE_DEV)   # unfiltered
    Qd = torch.from_numpy(Q).to(torch.device("cuda", 0))
    side = torch.cuda.Stream()
    seen_empty = seen_short = 0
    with engine.Index(base, metric, 0) as idx:
        idx.set_ivf(cen, off, lids)
        for mi, name in enumerate(MASKS):
            bits = _bits(name, n, 100 + mi, off, lids, uprobes[0])
            p = int(bits.sum())
            mask = engine.pack_mask(bits, n)
            if (n, dim) in ((33, 7), (1000, 128)):
                mask = _garbage_past_n(mask, n, 7 + mi)
            ei, ed, epr, empty = _expect(O, base, cen, off, lids, Q, bits, nprobe, om)
            seen_empty = max(seen_empty, empty if p else 0)
            if epr is not None:
                assert np.array_equal(epr, uprobes), "the oracle's routing saw the mask"
            if name == "ones":
                assert np.array_equal(ui, ei) and np.array_equal(ud, ed, equal_nan=True)
            if name == "zeros":
                assert p == 0 and (ei == -1).all() and np.isinf(ed).all()
            if name == "hand":
                assert p == sum(min(c, int(off[l + 1] - off[l])) for l, c in zip(uprobes[0][:3], (1, 8, 9)))
            md = _dev_mask(torch, mask)
            torch.cuda.synchronize()
            for j, k in enumerate(KS):
                nq = NQS[(mi + j) % len(NQS)]
                what = "%s %dx%d mask %s (p %d) nq %d k %d" % (metric, n, dim, name, p, nq, k)
                gi, gd, gp = idx.ivf_search_filtered(Q[:nq], k, nprobe, mask, want_probes=True)
                assert_exact(gi, gd, ei[:nq, :k], ed[:nq, :k], what + " host")
                assert np.array_equal(gp, uprobes[:nq]), what + ": probes"
                valid = (ei[:nq, :k] >= 0).sum(axis=1)              # the padding, stated: c results, then -1 / +inf
                for q in range(nq):
                    c = int(valid[q])
                    assert (gi[q, :c] >= 0).all() and (gi[q, c:] == -1).all() and np.isinf(gd[q, c:]).all(), what
                    assert not np.isinf(gd[q, :c]).any(), what
                    seen_short += c < k
                assert bits[gi[gi >= 0]].all(), what + ": a failing row was returned"
                gi2, gd2 = idx.ivf_search_filtered(Q[:nq], k, nprobe, mask)   # without the probes (the zeros mask's short cut)
                assert_exact(gi2, gd2, ei[:nq, :k], ed[:nq, :k], what + " host, no probes")
                with torch.cuda.stream(side):
                    di, dd = idx.ivf_search_filtered_dev(Qd[:nq], k, nprobe, md)
                side.synchronize()
                assert_exact(di.cpu().numpy(), dd.cpu().numpy(), ei[:nq, :k], ed[:nq, :k], what + " dev")
                if name == "ones" and (nq == 1 or metric == "l2"):   # where ivf_search runs a GEMV-order path: that call, bit for bit
                    vi, vd = idx.ivf_search(Q[:nq], k, nprobe)
                    assert_exact(gi, gd, vi, vd.astype(np.float64), what + " against ivf_search")
        if (n, dim) == (5000, 96):                                   # one k = 1024 case: the LDS list at its largest
            bits = _bits("half", n, 104, off, lids, uprobes[0])
            ei, ed, _, _ = _expect(O, base, cen, off, lids, Q[:12], bits, nprobe, om, k=1024)
            gi, gd = idx.ivf_search_filtered(Q[:12], 1024, nprobe, engine.pack_mask(bits, n))
            assert_exact(gi, gd, ei, ed, "%s k 1024" % metric)
            assert (gi >= 0).any() and (gi == -1).any()
    assert seen_short > 0, "the padded case is not exercised"
    if (n, dim) == (5000, 96):
        assert seen_empty > 0, "no filtered list became empty"


# ---- one index for the remaining properties --------------------------------------------------------------------------------
N, DIM, NLIST, NPROBE, K = 1000, 128, 16, 4, 10


@pytest.fixture(scope="module")
def ivf(native_lib, oracle):
    import torch

    from hnsw_clj_amd import datagen, engine

    O = oracle
    assert engine.device_count() >= 1, "no GPU visible"
    base = datagen.generate_dataset(N, DIM)
    Q = datagen.generate_dataset(NQ_MAX, DIM, seed=43)
    cen, off, lids = _lists(O, base, NLIST, O.COSINE)
    idx = engine.Index(base, "cosine", 0)
    idx.set_ivf(cen, off, lids)
    Qd = torch.from_numpy(Q).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    yield idx, base, Q, Qd, cen, off, lids
    idx.close()


def test_a_null_mask_and_a_handle_without_lists(ivf):
    import ctypes as C

    from hnsw_clj_amd import _native, datagen, engine

    idx, base, Q, Qd, cen, off, lids = ivf
    L = _native.lib()
    ids, d = np.empty((1, K), np.int32), np.empty((1, K), np.float32)
    q = np.ascontiguousarray(Q[:1])
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.hnswgpu_ivf_search_filtered(idx._h, p(q), 1, K, NPROBE, None, p(ids), p(d), None) == -1
    assert b"allow is null" in L.hnswgpu_last_error()
    mask = engine.pack_mask(np.ones(50, np.bool_), 50)
    with engine.Index(datagen.generate_dataset(50, DIM), "cosine", 0) as bare:
        with pytest.raises(_native.HnswGpuError) as e:
            bare.ivf_search_filtered(Q[:1], K, NPROBE, mask)
        assert e.value.code == -3


@pytest.mark.parametrize("metric", METRICS)
def test_ivf_filtered_ties_keep_the_list_order(native_lib, oracle, metric):
    from hnsw_clj_amd import datagen, engine

    O = oracle
    om = _om(O, metric)
    base = datagen.generate_dataset(N, DIM).copy()
    cen, off, lids = _lists(O, base, NLIST, om)
    l = int(np.argmax(np.diff(off)))
    a, b, c = (int(r) for r in lids[off[l]:off[l + 1]][[5, 1, 3]])   # three rows of one list; in list order: b, c, a
    base[b] = base[a]
    base[c] = base[a]
    in_list_order = [b, c, a]
    Q = np.concatenate([base[a:a + 1], datagen.generate_dataset(11, DIM, seed=43)])
    bits = np.ones(N, np.bool_)
    bits[::7] = False
    bits[[a, b, c]] = True
    ei, ed, _, _ = _expect(O, base, cen, off, lids, Q, bits, NLIST, om)
    with engine.Index(base, metric, 0) as idx:
        idx.set_ivf(cen, off, lids)                                  # the caller's lists and centroids, as given
        gi, gd = idx.ivf_search_filtered(Q, K, NLIST, engine.pack_mask(bits, N))
    assert_exact(gi, gd, ei[:, :K], ed[:, :K], metric + " ties")
    for q in range(len(Q)):                                          # wherever the three equal rows appear, they appear in list order
        got = [int(r) for r in gi[q] if r in (a, b, c)]
        assert got == in_list_order[:len(got)], (metric, q, got)
    if metric != "dot":
        assert list(gi[0, :3]) == in_list_order                      # the query is the row itself


def test_ivf_filtered_bits_do_not_depend_on_the_batch(ivf):
    from hnsw_clj_amd import engine

    idx, base, Q, Qd, cen, off, lids = ivf
    bits = np.random.default_rng(5).random(N) < 0.3
    mask = engine.pack_mask(bits, N)
    gi, gd = idx.ivf_search_filtered(Q, K, NPROBE, mask)
    for q in range(NQ_MAX):
        si, sd = idx.ivf_search_filtered(Q[q:q + 1], K, NPROBE, mask)
        assert np.array_equal(si[0], gi[q]) and np.array_equal(sd[0].view(np.uint32), gd[q].view(np.uint32)), "query %d" % q


def test_ivf_filtered_bits_do_not_depend_on_the_compact_copies(ivf, tune):
    from hnsw_clj_amd import engine

    idx, base, Q, Qd, cen, off, lids = ivf
    bits = np.random.default_rng(6).random(N) < 0.3
    mask = engine.pack_mask(bits, N)
    got = []
    for mode in (0, 2):                                              # new handles without / with the int8 and half copies
        tune.set("PREFILTER", mode)
        with engine.Index(base, "cosine", 0) as h:
            h.set_ivf(cen, off, lids)
            got.append([h.ivf_search_filtered(Q[:nq], K, NPROBE, mask) for nq in NQS])
    for (i0, d0), (i2, d2) in zip(*got):
        assert np.array_equal(i0, i2) and np.array_equal(d0.view(np.uint32), d2.view(np.uint32))
    ri, rd = idx.ivf_search_filtered(Q, K, NPROBE, mask)
    assert np.array_equal(got[0][-1][0], ri) and np.array_equal(got[0][-1][1].view(np.uint32), rd.view(np.uint32))


def test_ivf_filtered_call_between_unfiltered_calls_on_two_streams(ivf):
    """hg::Call orders the handle's scratch buffers across streams: an unfiltered search, a filtered one, an unfiltered one
    again and a filtered exact scan, back to back on two streams without a synchronise, each return the bits of the call
    run alone."""
    import torch

    from hnsw_clj_amd import engine

    idx, base, Q, Qd, cen, off, lids = ivf
    nq = 64
    bits = np.random.default_rng(7).random(N) < 0.5
    md = _dev_mask(torch, engine.pack_mask(bits, N))
    dev = Qd.device

    def out(k=K):
        return torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev)

    calls = [
        lambda o: idx.ivf_search_dev(Qd[:nq], K, NPROBE, out=o),
        lambda o: idx.ivf_search_filtered_dev(Qd[:nq], K, NPROBE, md, out=o),
        lambda o: idx.ivf_search_dev(Qd[:nq], K, 2 * NPROBE, out=o),
        lambda o: idx.exact_knn_filtered_dev(Qd[:nq], K, md, out=o),
    ]
    alone = []
    for c in calls:
        o = out()
        c(o)
        torch.cuda.synchronize()
        alone.append(o)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    reps = 5
    got = [[out() for _ in calls] for _ in range(reps)]
    torch.cuda.synchronize()
    for r in range(reps):
        for j, c in enumerate(calls):
            with torch.cuda.stream(streams[(j + r) % 2]):
                c(got[r][j])
    torch.cuda.synchronize()
    for r in range(reps):
        for j in range(len(calls)):
            assert torch.equal(got[r][j][0], alone[j][0]), "repetition %d, call %d: ids" % (r, j)
            assert torch.equal(got[r][j][1].view(torch.int32), alone[j][1].view(torch.int32)), "repetition %d, call %d: bits" % (r, j)


# ---- the mirror --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mirror(ivf):
    from hnsw_clj_amd import engine, ivf_flat
    from hnsw_clj_amd.ultra_fast import cosine_distance_ultra

    idx, base, Q, Qd, cen, off, lids = ivf
    h = engine.Index(base, "cosine", 0)
    h.set_ivf(cen, off, lids)
    index = ivf_flat.IVFFlatIndex(h, ["v%d" % i for i in range(N)], cosine_distance_ultra, NLIST)
    yield index
    index.close()


def test_ivf_flat_search_batch_filtered(ivf, mirror):
    from hnsw_clj_amd import engine, ivf_flat, protocol

    idx, base, Q, Qd, cen, off, lids = ivf
    pred = lambda s: int(s[1:]) % 2 == 0  # noqa: E731  (a predicate on the caller's String ids)
    bits = np.arange(N) % 2 == 0
    res = ivf_flat.search_batch_filtered(mirror, Q[:12], K, pred)                 # "balanced": 4 probes
    gi, gd = idx.ivf_search_filtered(Q[:12], K, 4, engine.pack_mask(bits, N))
    assert len(res) == 12
    for q in range(12):
        assert [r["id"] for r in res[q]] == ["v%d" % i for i in gi[q] if i >= 0]
        assert [np.float32(r["distance"]) for r in res[q]] == [d for i, d in zip(gi[q], gd[q]) if i >= 0]
        assert all(pred(r["id"]) for r in res[q])
    assert ivf_flat.search_batch_filtered(mirror, Q[:12], K, bits) == res         # a bool array instead of the predicate
    assert ivf_flat.search_knn_filtered(mirror, Q[3], K, pred) == res[3]
    gi8, _ = idx.ivf_search_filtered(Q[:2], K, 8, engine.pack_mask(bits, N))
    res8 = ivf_flat.search_batch_filtered(mirror, Q[:2], K, bits, mode="accurate")
    assert [[r["id"] for r in rs] for rs in res8] == [["v%d" % i for i in row if i >= 0] for row in gi8]
    # a sparse mask: the scan of the passing rows finds what "search 3k, drop, keep k" cannot
    sparse = np.random.default_rng(105).random(N) < 0.03
    spred = lambda s: bool(sparse[int(s[1:])])  # noqa: E731
    mine = sum(len(r) for r in ivf_flat.search_batch_filtered(mirror, Q[:12], K, spred))
    plain = protocol.GpuIvfFlatIndex(mirror)
    default = sum(len(protocol.default_filtered_search(plain, Q[q], K, spred, "balanced")) for q in range(12))
    assert mine > default, "filtered scan returned %d results over 12 queries, the default helper %d" % (mine, default)


def test_protocol_filterable_ivf_index(ivf, mirror):
    from hnsw_clj_amd import protocol

    idx, base, Q, Qd, cen, off, lids = ivf
    index = protocol.GpuFilterableIvfFlatIndex(mirror)
    assert protocol.supports_filtering(index) and not protocol.supports_filtering(protocol.GpuIvfFlatIndex(mirror))
    pred = lambda s: int(s[1:]) % 3 == 0  # noqa: E731
    res = index.search_knn_filtered_star(Q[0], K, pred, "balanced")
    assert len(res) == K and all(set(r) == {"id", "distance"} and pred(r["id"]) for r in res)
    ds = [r["distance"] for r in res]
    assert ds == sorted(ds)
