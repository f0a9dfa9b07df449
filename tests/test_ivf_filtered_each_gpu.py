"""IVF-FLAT filtered search with one allow-mask per query (hnswgpu_ivf_search_filtered_each) on the device: ids identical and
distance bits identical to two yardsticks that do not run the code under test --

  the unmodified oracle, once per DISTINCT mask (ivf_each_model.expect_each: the lists restricted to the passing rows,
  O.ivf_search(..., MODE_DEV), ids mapped back), and
  the device's own single-mask call, one query at a time.

The inputs and what they are chosen for live in ivf_each_model.py; test_ivf_filtered_each_host.py checks there, without a GPU,
that they cover what the asserts below rely on."""
import numpy as np
import pytest

import ivf_each_model as M
from util import assert_exact

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "l2", "dot"]
# (n, dim, nlist, nprobe): the single-mask test's shapes -- W = 2 and lists shorter than one 64-block / the ordinary case / every
# list probed / 157 mask words and empty filtered lists / the widest row loaders -- and n = 64: W exact, no tail bits
SHAPES = [(33, 7, 3, 2), (1000, 128, 16, 4), (300, 768, 7, 7), (5000, 96, 64, 8), (70, 1536, 4, 2), (70, 3072, 4, 2), (64, 16, 2, 2)]
NQS = [1, 12, 70]
KS = [1, 10, 64, 100]         # 64: the last register list, 100: the first LDS list
NQ_MAX, K_MAX = 70, 100


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(torch.device("cuda", 0))


def _bits_equal(gi, gd, ri, rd, what):
    assert np.array_equal(gi, ri), what + ": ids"
    assert np.array_equal(np.asarray(gd, np.float32).view(np.uint32), np.asarray(rd, np.float32).view(np.uint32)), what + ": distance bits"


def _singles(idx, Q, k, nprobe, masks, which):
    """The device's single-mask call, one query at a time."""
    out = [idx.ivf_search_filtered(Q[q:q + 1], k, nprobe, masks[which[q]]) for q in range(len(Q))]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def _check_rows(gi, gd, ei, bits_list, which, what):
    """Nothing with a clear bit for ITS query, and the padding: c results, then -1 / +inf.  -> rows with fewer than k results"""
    short = 0
    for q in range(len(gi)):
        c = int((ei[q] >= 0).sum())
        assert (gi[q, :c] >= 0).all() and (gi[q, c:] == -1).all() and np.isinf(gd[q, c:]).all(), what
        assert not np.isinf(gd[q, :c]).any(), what
        assert bits_list[which[q]][gi[q, :c]].all(), "%s: query %d got a row its mask does not allow" % (what, q)
        short += c < gi.shape[1]
    return short


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("metric", METRICS)
def test_ivf_search_filtered_each_matches_the_oracle_and_the_single_mask_call(native_lib, oracle, metric, shape):
    import torch

    from hnsw_clj_amd import datagen, engine

    O = oracle
    o_metric = M.om(O, metric)
    n, dim, nlist, nprobe = shape
    base = datagen.generate_dataset(n, dim)
    Q = datagen.generate_dataset(NQ_MAX, dim, seed=43)
    cen, off, lids = M.lists(O, base, nlist, o_metric)
    _, _, uprobes = O.ivf_search(base, cen, off, lids, Q, 1, nprobe, metric=o_metric, mode=O.MODE_DEV)   # the unfiltered routing
    bits_list = M.parity_bits(n, 100, off, lids, uprobes[0])
    which = M.deal(NQ_MAX, len(bits_list))                           # a prefix of the batch keeps its masks
    ei, ed = M.expect_each(O, base, cen, off, lids, Q, bits_list, which, nprobe, o_metric, K_MAX)
    clean = engine.pack_masks(bits_list, n)
    packed = M.garbage_past_n(clean, n, 7)                           # garbage past n in every row (where n & 31)
    assert (n & 31 == 0) == np.array_equal(packed, clean)
    rows = np.ascontiguousarray(packed[which])
    Qd, rows_d = torch.from_numpy(Q).to(torch.device("cuda", 0)), _dev(torch, rows)
    side = torch.cuda.Stream()
    seen_short = 0
    with engine.Index(base, metric, 0) as idx:
        idx.set_ivf(cen, off, lids)
        si, sd = _singles(idx, Q, K_MAX, nprobe, packed, which)
        assert_exact(si, sd, ei, ed, "%s %dx%d: the single-mask call per query" % (metric, n, dim))
        torch.cuda.synchronize()
        for nq in NQS:
            for k in KS:
                what = "%s %dx%d nq %d k %d" % (metric, n, dim, nq, k)
                gi, gd, gp = idx.ivf_search_filtered_each(Q[:nq], k, nprobe, rows[:nq], want_probes=True)
                assert_exact(gi, gd, ei[:nq, :k], ed[:nq, :k], what + " host")
                _bits_equal(gi, gd, si[:nq, :k], sd[:nq, :k], what + " host against the single-mask calls")
                assert np.array_equal(gp, uprobes[:nq]), what + ": probes"
                seen_short += _check_rows(gi, gd, ei[:nq, :k], bits_list, which, what)
                gi2, gd2 = idx.ivf_search_filtered_each(Q[:nq], k, nprobe, rows[:nq])
                _bits_equal(gi2, gd2, gi, gd, what + " host, no probes")
                with torch.cuda.stream(side):
                    di, dd = idx.ivf_search_filtered_each_dev(Qd[:nq], k, nprobe, rows_d[:nq])
                side.synchronize()
                assert_exact(di.cpu().numpy(), dd.cpu().numpy(), ei[:nq, :k], ed[:nq, :k], what + " dev")
        gi, gd, gp = idx.ivf_search_filtered_each(Q[:12], 10, nlist + 3, rows[:12], want_probes=True)   # nprobe > nlist: -1 padded
        assert (gp[:, nlist:] == -1).all() and (gp[:, :nlist] >= 0).all()
        if (n, dim) == (5000, 96):                                   # one k = 1024 case: the LDS list at its largest
            xi, xd = M.expect_each(O, base, cen, off, lids, Q[:12], bits_list, which[:12], nprobe, o_metric, 1024)
            gi, gd = idx.ivf_search_filtered_each(Q[:12], 1024, nprobe, rows[:12])
            assert_exact(gi, gd, xi, xd, "%s k 1024" % metric)
            assert (gi >= 0).any() and (gi == -1).any()
    assert seen_short > 0, "the padded case is not exercised"


# ---- block and queue edges: crafted lists, masks placed by list position -----------------------------------------------------------
# RB = 8 here: dim 32 is one 256-float chunk per row, and launch_ivf_filtered_scan's dispatch gives that width 8 register rows.
@pytest.mark.parametrize("case", ["edge", "long_walk"])
@pytest.mark.parametrize("metric", METRICS)
def test_block_and_queue_edges(native_lib, oracle, tune, metric, case):
    import torch

    from hnsw_clj_amd import engine

    O = oracle
    o_metric = M.om(O, metric)
    E = M.edge_case() if case == "edge" else M.long_walk_case()
    ei, ed = M.expect_each(O, E.base, E.cen, E.off, E.lids, E.Q, E.masks, E.which, E.nprobe, o_metric, E.k)
    packed = M.garbage_past_n(engine.pack_masks(E.masks, E.n), E.n, 9)
    rows = np.ascontiguousarray(packed[E.which])
    Qd, rows_d = torch.from_numpy(E.Q).to(torch.device("cuda", 0)), _dev(torch, rows)
    with engine.Index(E.base, metric, 0) as idx:
        idx.set_ivf(E.cen, E.off, E.lids)
        for blocks in (1, None):                                     # one chunk per pair (whole 64-blocks, several per wave), the default chunks
            if blocks:
                tune.set("SCAN_BLOCKS", blocks)
            else:
                tune.unset("SCAN_BLOCKS")
            # (one workgroup per pair: the single-mask kernel walks several tiles of a segment longer than the mean)
            si, sd = _singles(idx, E.Q, E.k, E.nprobe, packed, E.which)
            assert_exact(si, sd, ei, ed, "%s %s SCAN_BLOCKS %s: the single-mask call per query" % (metric, case, blocks))
            for k in (E.k, 10, 1):
                what = "%s %s SCAN_BLOCKS %s k %d" % (metric, case, blocks, k)
                gi, gd = idx.ivf_search_filtered_each(E.Q, k, E.nprobe, rows)
                assert_exact(gi, gd, ei[:, :k], ed[:, :k], what)
                _check_rows(gi, gd, ei[:, :k], E.masks, E.which, what)
                di, dd = idx.ivf_search_filtered_each_dev(Qd, k, E.nprobe, rows_d)
                torch.cuda.synchronize()
                assert_exact(di.cpu().numpy(), dd.cpu().numpy(), ei[:, :k], ed[:, :k], what + " dev")
    if case == "edge":
        assert ((ei >= 0).sum(axis=1) < E.k).any() and ((ei >= 0).sum(axis=1) > 64).any()


# ---- several chunks per pair ------------------------------------------------------------------------------------------------------
# 20000 x 32 in 2 lists, nprobe 2, ONE query: npairs = 2, so plan_chunks aims at max(512, 8 * 2) = 512 workgroups, 256 per pair;
# a chunk is at least one trip of the four waves' 8 register rows (32 positions), so at most ceil(mean / 32) = 313 chunks fit and
# 256 stay; chunk_rows = ceil(10000 / 256) = 40, rounded up to 64; nchunks = ceil(longest list / 64) >= 157 > 1.  (Two queries:
# 128 chunks per pair wanted, chunk_rows 96.)  The model restates the rule; the assert below keeps the derivation honest.
def test_several_chunks_per_pair(native_lib, oracle):
    from hnsw_clj_amd import datagen, engine

    O = oracle
    n, dim, nlist, nprobe, k = 20000, 32, 2, 2, 10
    base = datagen.generate_dataset(n, dim)
    Q = datagen.generate_dataset(2, dim, seed=43)
    cen, off, lids = M.lists(O, base, nlist, O.COSINE)
    longest = int(np.diff(off).max())
    assert M.plan_chunks(dim, longest, n // nlist, 1 * nprobe) == (64, -(-longest // 64)) and longest > 64
    assert M.plan_chunks(dim, longest, n // nlist, 2 * nprobe)[1] > 1
    rng = np.random.default_rng(21)
    bits_list = [rng.random(n) < 0.5, rng.random(n) < 0.03]
    packed = engine.pack_masks(bits_list, n)
    with engine.Index(base, "cosine", 0) as idx:
        idx.set_ivf(cen, off, lids)
        for m, bits in enumerate(bits_list):
            ei, ed, _ = M.expect_single(O, base, cen, off, lids, Q[:1], bits, nprobe, O.COSINE, k)
            gi, gd = idx.ivf_search_filtered_each(Q[:1], k, nprobe, packed[m:m + 1])
            assert_exact(gi, gd, ei, ed, "one query, mask %d" % m)
            si, sd = idx.ivf_search_filtered(Q[:1], k, nprobe, packed[m])
            _bits_equal(gi, gd, si, sd, "one query, mask %d against the single-mask call" % m)
        ei, ed = M.expect_each(O, base, cen, off, lids, Q, bits_list, [0, 1], nprobe, O.COSINE, k)
        gi, gd = idx.ivf_search_filtered_each(Q, k, nprobe, packed)
        assert_exact(gi, gd, ei, ed, "two queries, two masks")


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
    cen, off, lids = M.lists(O, base, NLIST, O.COSINE)
    _, _, uprobes = O.ivf_search(base, cen, off, lids, Q, 1, NPROBE, metric=O.COSINE, mode=O.MODE_DEV)
    bits_list = M.parity_bits(N, 5, off, lids, uprobes[0])
    which = M.deal(NQ_MAX, len(bits_list))
    rows = np.ascontiguousarray(engine.pack_masks(bits_list, N)[which])
    idx = engine.Index(base, "cosine", 0)
    idx.set_ivf(cen, off, lids)
    Qd = torch.from_numpy(Q).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    yield idx, base, Q, Qd, cen, off, lids, bits_list, which, rows
    idx.close()


def test_bits_do_not_depend_on_the_batch_or_the_rejection_mode(ivf):
    from hnsw_clj_amd import engine

    idx, base, Q, Qd, cen, off, lids, bits_list, which, rows = ivf
    gi, gd = idx.ivf_search_filtered_each(Q, K, NPROBE, rows)
    for q in range(NQ_MAX):
        si, sd = idx.ivf_search_filtered_each(Q[q:q + 1], K, NPROBE, rows[q:q + 1])
        _bits_equal(si[0], sd[0], gi[q], gd[q], "query %d alone" % q)
    with engine.Index(base, "cosine", 0) as h:
        h.set_rejection_test(0)
        h.set_ivf(cen, off, lids)
        for nq in NQS:
            hi, hd = h.ivf_search_filtered_each(Q[:nq], K, NPROBE, rows[:nq])
            _bits_equal(hi, hd, gi[:nq], gd[:nq], "rejection test off, nq %d" % nq)


@pytest.mark.parametrize("metric", METRICS)
def test_ties_keep_the_list_order_per_query_mask(native_lib, oracle, metric):
    from hnsw_clj_amd import datagen, engine

    O = oracle
    o_metric = M.om(O, metric)
    base = datagen.generate_dataset(N, DIM).copy()
    cen, off, lids = M.lists(O, base, NLIST, o_metric)
    l = int(np.argmax(np.diff(off)))
    a, b, c = (int(r) for r in lids[off[l]:off[l + 1]][[5, 1, 3]])   # three rows of one list; in list order: b, c, a
    base[b] = base[a]
    base[c] = base[a]
    Q = np.concatenate([base[a:a + 1]] * 3 + [datagen.generate_dataset(9, DIM, seed=43)])
    all3 = np.ones(N, np.bool_)
    all3[::7] = False
    all3[[a, b, c]] = True
    no_b, no_c = all3.copy(), all3.copy()
    no_b[b] = False
    no_c[c] = False
    bits_list, orders = [all3, no_b, no_c], [[b, c, a], [c, a], [b, a]]
    which = M.deal(len(Q), 3)
    ei, ed = M.expect_each(O, base, cen, off, lids, Q, bits_list, which, NLIST, o_metric, K)
    with engine.Index(base, metric, 0) as idx:
        idx.set_ivf(cen, off, lids)                                  # the caller's lists and centroids, as given
        gi, gd = idx.ivf_search_filtered_each(Q, K, NLIST, engine.pack_masks(bits_list, N)[which])
    assert_exact(gi, gd, ei, ed, metric + " ties")
    for q in range(len(Q)):                                          # wherever the equal rows appear, they appear in list order
        want = orders[which[q]]
        got = [int(r) for r in gi[q] if r in (a, b, c)]
        assert got == want[:len(got)], (metric, q, got)
    if metric != "dot":
        for q in range(3):                                           # the query is the row itself
            assert list(gi[q, :len(orders[q])]) == orders[q]


def test_life_cycle(ivf):
    import ctypes as C

    from hnsw_clj_amd import _native, datagen, engine

    idx, base, Q, Qd, cen, off, lids, bits_list, which, rows = ivf
    # a handle without lists: -3; no queries: 0
    with engine.Index(datagen.generate_dataset(50, DIM), "cosine", 0) as bare:
        with pytest.raises(_native.HnswGpuError) as e:
            bare.ivf_search_filtered_each(Q[:2], K, NPROBE, engine.pack_masks(np.ones((2, 50), np.bool_), 50))
        assert e.value.code == -3
    one = C.c_void_p(8)
    assert _native.lib().hnswgpu_ivf_search_filtered_each(idx._h, one, 0, K, NPROBE, one, one, one, None) == 0
    assert _native.lib().hnswgpu_ivf_search_filtered_each_dev(idx._h, one, 0, K, NPROBE, one, one, one, None) == 0
    # rows that change W join the lists: a call with the longer masks equals a fresh handle over all rows
    more = (Q[:30] * np.float32(1.5)).astype(np.float32)              # row N + q: query q's direction, its nearest row wherever allowed
    n2 = N + len(more)
    assert (n2 + 31) // 32 == (N + 31) // 32 + 1
    rng = np.random.default_rng(8)
    bits2 = [rng.random(n2) < 0.5, np.arange(n2) >= N - 40, rng.random(n2) < 0.05]
    which2 = M.deal(12, 3)
    rows2 = np.ascontiguousarray(M.garbage_past_n(engine.pack_masks(bits2, n2), n2, 3)[which2])
    with engine.Index(base, "cosine", 0) as grown:
        grown.set_ivf(cen, off, lids)
        grown.ivf_search_filtered_each(Q[:12], K, NPROBE, rows[:12])               # the scratch is sized for the old W first
        grown.ivf_add(more)
        cen2, off2, lids2 = grown.get_ivf()
        gi, gd = grown.ivf_search_filtered_each(Q[:12], K, NPROBE, rows2)
    with engine.Index(np.concatenate([base, more]), "cosine", 0) as fresh:
        fresh.set_ivf(cen2, off2, lids2)
        fi, fd = fresh.ivf_search_filtered_each(Q[:12], K, NPROBE, rows2)
    _bits_equal(gi, gd, fi, fd, "grown against fresh")
    assert [int(gi[q, 0]) for q in (1, 4, 7, 10)] == [N + 1, N + 4, N + 7, N + 10], "the added rows are not found"   # mask 1 allows them
    for q in range(12):
        assert bits2[which2[q]][gi[q][gi[q] >= 0]].all()


def test_each_call_between_unfiltered_calls_on_two_streams(ivf):
    """hg::Call orders the handle's scratch buffers across streams: an unfiltered search, an _each one, an unfiltered one again and
    a single-mask one, back to back on two streams without a synchronise, each return the bits of the call run alone."""
    import torch

    idx, base, Q, Qd, cen, off, lids, bits_list, which, rows = ivf
    nq = 64
    rows_d = _dev(torch, rows[:nq])
    one_d = _dev(torch, rows[2])
    dev = Qd.device

    def out(k=K):
        return torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev)

    calls = [
        lambda o: idx.ivf_search_dev(Qd[:nq], K, NPROBE, out=o),
        lambda o: idx.ivf_search_filtered_each_dev(Qd[:nq], K, NPROBE, rows_d, out=o),
        lambda o: idx.ivf_search_dev(Qd[:nq], K, 2 * NPROBE, out=o),
        lambda o: idx.ivf_search_filtered_dev(Qd[:nq], K, NPROBE, one_d, out=o),
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


# ---- the mirrors -------------------------------------------------------------------------------------------------------------
def test_mirrors_return_per_query_what_search_knn_filtered_returns(ivf):
    from hnsw_clj_amd import engine, ivf_flat, protocol
    from hnsw_clj_amd.ultra_fast import cosine_distance_ultra

    idx, base, Q, Qd, cen, off, lids, bits_list, which, rows = ivf
    h = engine.Index(base, "cosine", 0)
    h.set_ivf(cen, off, lids)
    index = ivf_flat.IVFFlatIndex(h, ["v%d" % i for i in range(N)], cosine_distance_ultra, NLIST)
    try:
        even = lambda s: int(s[1:]) % 2 == 0  # noqa: E731  (a predicate on the caller's String ids)
        fns = [even, bits_list[2], bits_list[4], even, bits_list[1], bits_list[3], bits_list[2].copy()]
        for mode in ("balanced", "accurate"):
            res = ivf_flat.search_batch_filtered_each(index, Q[:len(fns)], K, fns, mode=mode)
            assert len(res) == len(fns)
            for q, f in enumerate(fns):
                assert res[q] == ivf_flat.search_knn_filtered(index, Q[q], K, f, mode), (mode, q)
            assert all(even(r["id"]) for r in res[0]) and res[4] == [] and len(res[1]) == K
        res = protocol.GpuIvfFlatIndex(index).search_batch_filtered(Q[:len(fns)], K, fns)
        assert res == ivf_flat.search_batch_filtered_each(index, Q[:len(fns)], K, fns, mode="balanced")
        res = protocol.GpuFilterableIvfFlatIndex(index).search_batch_filtered(Q[:3], K, fns[:3], "accurate")
        assert res == [ivf_flat.search_knn_filtered(index, Q[q], K, fns[q], "accurate") for q in range(3)]
    finally:
        index.close()
