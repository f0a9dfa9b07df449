"""Range search at the shapes where its index arithmetic first matters: a second fill block and the later waves of one
(n = 32805), scan chunks of several tiles, slices of several groups, batches past one scan trip of range_lims_kernel and past one
slice's blockIdx.y (nq = 65600), stale hit words on a reused handle, the sort network's boundary lengths, and cap under
HNSWGPU_RANGE_BY_DISTANCE.  test_range_search_gpu.py and test_range_search_filtered_gpu.py cover distances, radii and masks at
549 rows x 35 queries; nothing there reaches these paths.

The reference is theirs: the expected SET comes from float64 numpy distances, with every radius in the middle of a float64 gap
that exceeds 100 x the largest |hnswgpu_batch_distances - float64| of its query vector (the EXISTING entry point's error, checked
for every query, none skipped; and checked against a float32 numpy restatement before anything runs on the GPU); the expected
distance BITS are those of hnswgpu_batch_distances.  Batches repeat 40 distinct vectors -- query q is vector q % 40 with its own
radius -- so equal queries of one group must still get their own words, counts and segments (range_shapes.py)."""
import functools

import numpy as np
import pytest
import range_shapes as S

pytestmark = pytest.mark.gpu

N = S.N_BIG
BIG = [("cosine", 20, 1100), ("l2", 20, 1100), ("dot", 20, 1100), ("cosine", 1100, 300)]   # dim 1100: 16 queries per group
EACH_NQ = {20: 522, 1100: 300}      # 17 groups of 32 (the last of 10 queries); 19 groups of 16 (the last of 12)


def _reference(metric, base, V, nq, targets, **kw):
    """Guarded radii and the expected id-order result of the batch whose query q is V[q % len(V)]."""
    from hnsw_clj_amd import engine

    dv = S.d64(metric, V, base)
    rad64, gap = S.radii(dv, nq, targets, **kw)
    cpu = S.guard(gap, np.abs(S.d32(metric, V, base).astype(np.float64) - dv).max(1), nq, rad64)
    with engine.Index(base, metric, 0) as idx:
        bd = np.stack([idx.batch_distances(v) for v in V])                # the existing entry point: the bits to match
    gpu = S.guard(gap, np.abs(bd.astype(np.float64) - dv).max(1), nq, rad64)
    print("%s n %d dim %d: smallest gap / error = %.0f (float32 numpy: %.0f)" % (metric, len(base), base.shape[1], gpu, cpu))
    within = np.empty((nq, len(base)), bool)
    for v in range(len(V)):                                               # (a NaN radius: nothing)
        within[v::len(V)] = dv[v][None, :] <= rad64[v::len(V), None]
    Q = np.ascontiguousarray(V[np.arange(nq) % len(V)])
    return dict(base=base, Q=Q, rad=rad64.astype(np.float32), within=within, bd=bd, want=S.csr(within, bd))


@functools.lru_cache(maxsize=None)
def _big(metric, dim, nq):
    base, V = S.big_data(dim)
    r = _reference(metric, base, V, nq, S.TARGETS, tied_row=S.TIED_BIG[0])
    r["want_d"] = S.by_distance(r["want"])
    lims, ids, _ = r["want"]
    cnt = np.diff(lims)
    some = np.flatnonzero(cnt)
    lo, hi = ids[lims[some]], ids[lims[some + 1] - 1]
    assert (lo >= 32768).any() and (hi < 32768).any()                     # hits in fill block 1 alone, in block 0 alone
    for wave in (1, 2, 3):                                                # ... and in the words of one later wave alone
        assert ((lo // 8192 == wave) & (hi // 8192 == wave)).any(), wave
    assert cnt[0] == 0 and cnt[S.NVEC] == len(S.TIED_BIG)                 # just below / just above the tied distance
    assert tuple(ids[lims[S.NVEC]:lims[S.NVEC + 1]]) == S.TIED_BIG
    assert {0, 1, N - 1, N} <= set(cnt) and ((cnt > 900) & (cnt < 1300)).any() and ((cnt > N // 2 - 600) & (cnt < N // 2 + 600)).any()
    assert np.isnan(r["rad"]).any() and lims[-1] < 8_000_000
    return r


@pytest.mark.parametrize("metric,dim,nq", BIG)
def test_unfiltered_two_fill_blocks_wide_chunks_and_grouped_slices(native_lib, tune, metric, dim, nq):
    """n = 32805: W = 1026 words, so range_fill_kernel runs two blocks per query (blk[q][1], the blockIdx.x term of row0) and all
    four waves of block 0 hold words.  At the default budget the batch is one slice whose scan chunks span several tiles; with
    FILTER_EACH_MB = 1 it is several slices of several groups each (lims + q0, the *run carry), bit-identical."""
    from hnsw_clj_amd import engine

    r = _big(metric, dim, nq)
    G, gps, chunk_rows = S.slicing(N, dim, nq)
    assert gps >= G and chunk_rows > 256                                  # one slice, chunks of more than one tile
    G1, gps1, _ = S.slicing(N, dim, nq, budget_mb=1)
    assert 1 < gps1 < G1                                                  # slices of several groups, several slices
    with engine.Index(r["base"], metric, 0) as idx:
        got = idx.range_search(r["Q"], r["rad"])
        S.same(got, r["want"], "id order")
        got_d = idx.range_search(r["Q"], r["rad"], by_distance=True)
        S.same(got_d, r["want_d"], "distance order")
        tune.set("FILTER_EACH_MB", 1)
        S.same(idx.range_search(r["Q"], r["rad"]), S.bits_of(got), "sliced, id order")
        S.same(idx.range_search(r["Q"], r["rad"], by_distance=True), S.bits_of(got_d), "sliced, distance order")


def _mask_big(kind):
    """ones | pct (about 1 %) | most (32785 rows pass: list positions reach the second fill block) | edge (32768 + 1 pass) |
    tail (the last, partial mask word + row 0).  The tied rows pass or fail together; the last row passes."""
    rng = np.random.default_rng(17)
    m = np.ones(N, bool)
    if kind == "pct":
        m = rng.random(N) < 0.01
        m[list(S.TIED_BIG)] = m[N - 1] = True
    elif kind in ("most", "edge"):
        free = np.setdiff1d(np.arange(N - 1), S.TIED_BIG)
        m[rng.choice(free, 20 if kind == "most" else N - 32769, replace=False)] = False
    elif kind == "tail":
        m[:] = False
        m[N // 32 * 32:] = m[0] = True
    return m


@pytest.mark.parametrize("kind", ["ones", "pct", "most", "edge", "tail"])
@pytest.mark.parametrize("metric,dim,nq", BIG)
def test_single_mask_at_two_fill_blocks(native_lib, tune, metric, dim, nq, kind):
    """The unfiltered result (pinned to the same arrays by the test above) with the failing rows dropped, ids and bits alike: in
    id order at the default budget, in distance order in slices of several groups."""
    from hnsw_clj_amd import engine

    r = _big(metric, dim, nq)
    m = _mask_big(kind)
    assert m.sum() == {"ones": N, "most": N - 20, "edge": 32769, "tail": N % 32 + 1}[kind] if kind != "pct" else 200 < m.sum() < 500
    want = S.csr(r["within"], r["bd"], m[None, :])
    if kind in ("most", "edge"):                                          # a hit at a list position in the second fill block
        assert (np.cumsum(m)[want[1]] - 1 >= 32768).any()
    if kind == "ones":
        assert all(np.array_equal(a, b) for a, b in zip(want, r["want"]))
    with engine.Index(r["base"], metric, 0) as idx:
        S.same(idx.range_search_filtered(r["Q"], r["rad"], engine.pack_mask(m, N)), want, "id order")
        tune.set("FILTER_EACH_MB", 1)
        S.same(idx.range_search_filtered(r["Q"], r["rad"], engine.pack_mask(m, N), by_distance=True), S.by_distance(want), "sliced, distance order")


def _masks_each(nq, n, seed=23):
    """One mask per query, densities from 0.05 % to 97 %; the first group holds an all-zero and an all-ones mask, two equal masks
    and two complementary ones; the last query's mask is all ones."""
    rng = np.random.default_rng(seed)
    M = rng.random((nq, n), dtype=np.float32) < rng.choice([0.0005, 0.01, 0.125, 0.5, 0.97], nq).astype(np.float32)[:, None]
    M[0], M[1], M[3], M[5], M[nq - 1] = False, True, M[2], ~M[4], True
    return M


@pytest.mark.parametrize("metric,dim,nq", BIG)
def test_each_mask_at_two_fill_blocks(native_lib, tune, metric, dim, nq):
    """Row q is the single-mask call of query q with mask q: against the reference set for every q, against an actual
    single-mask call for a sample spread over the groups.  Default budget (one slice) and FILTER_EACH_MB = 1 (slices of several
    groups, each with its own union lists) agree bit for bit."""
    from hnsw_clj_amd import engine

    r, ne = _big(metric, dim, nq), EACH_NQ[dim]
    Q, rad = r["Q"][:ne], r["rad"][:ne]
    M = _masks_each(ne, N)
    packed = S.pack_rows(M)
    assert np.array_equal(packed[:6], engine.pack_masks(M[:6], N))
    G, gps, chunk_rows = S.slicing(N, dim, ne, each=True)
    assert gps >= G and chunk_rows > 256
    G1, gps1, _ = S.slicing(N, dim, ne, budget_mb=1, each=True)
    assert 1 < gps1 < G1 and ne % S.tq_of(dim) != 0
    want = S.csr(r["within"][:ne], r["bd"], M)
    lims = want[0]
    with engine.Index(r["base"], metric, 0) as idx:
        got = idx.range_search_filtered_each(Q, rad, packed)
        S.same(got, want, "id order")
        got_d = idx.range_search_filtered_each(Q, rad, packed, by_distance=True)
        S.same(got_d, S.by_distance(want), "distance order")
        sample = sorted(set([0, 1, 2, 3, 4, 5]) | set(np.linspace(6, ne - 1, 12).astype(int)))
        assert (ne - 1) // S.tq_of(dim) == G - 1 and len({q // S.tq_of(dim) for q in sample}) >= min(G, 8)
        for q in sample:
            a, b = lims[q], lims[q + 1]
            one = idx.range_search_filtered(Q[q:q + 1], rad[q], packed[q])
            S.same(one, (np.array([0, b - a]), got[1][a:b], got[2][a:b].view(np.uint32)), "query %d alone" % q)
        tune.set("FILTER_EACH_MB", 1)
        S.same(idx.range_search_filtered_each(Q, rad, packed), S.bits_of(got), "sliced, id order")
        S.same(idx.range_search_filtered_each(Q, rad, packed, by_distance=True), S.bits_of(got_d), "sliced, distance order")


@pytest.mark.parametrize("later_nq", [96, 40])
def test_stale_hit_words_on_a_reused_handle(native_lib, later_nq):
    """The hit words are scratch of the handle.  A radius of +inf sets every bit of 96 queries' words; the gathered scans that
    follow must clear the words past their lists' ends (about 330 positions of 32805), or the count pass reads the old bits.
    Every call equals the same call on a fresh handle -- with as many queries as the first call, and with fewer."""
    from hnsw_clj_amd import engine

    r = _big("l2", 20, 1100)
    Q, rad, k = r["Q"], r["rad"], later_nq
    pct = engine.pack_mask(_mask_big("pct"), N)
    M = np.random.default_rng(29).random((k, N), dtype=np.float32) < np.float32(0.001)   # unions of a group: about 1000 rows
    packed = S.pack_rows(M)
    calls = [("single mask", lambda i: i.range_search_filtered(Q[:k], rad[:k], pct), S.csr(r["within"][:k], r["bd"], _mask_big("pct")[None, :])),
             ("each", lambda i: i.range_search_filtered_each(Q[:k], rad[:k], packed), S.csr(r["within"][:k], r["bd"], M)),
             ("unfiltered", lambda i: i.range_search(Q[:k], rad[:k]), S.csr(r["within"][:k], r["bd"]))]
    with engine.Index(r["base"], "l2", 0) as idx:
        assert np.array_equal(idx.range_search(Q[:96], np.inf)[0], np.arange(97) * N)
        for what, call, want in calls:
            with engine.Index(r["base"], "l2", 0) as fresh:
                ref = call(fresh)
            S.same(ref, want, what + ", fresh handle")
            S.same(call(idx), S.bits_of(ref), what + ", reused handle")
        assert np.array_equal(idx.range_search(Q[:96], np.inf)[0], np.arange(97) * N)


# ---- batches past 1024 queries and past one slice's blockIdx.y --------------------------------------------------------------
SMALL_N, SMALL_NQ = 70, 65600
ZERO_AT = (63, 64, 1023, 1024, 1088, SMALL_NQ - 1)


@functools.lru_cache(maxsize=None)
def _small(metric):
    base, V = S.small_data(SMALL_N, 20)
    r = _reference(metric, base, V, SMALL_NQ, tuple(range(SMALL_N + 1)), zero_at=ZERO_AT)
    cnt = np.diff(r["want"][0])
    assert not cnt[list(ZERO_AT)].any() and cnt[[62, 65, 1022, 1025, 1087, SMALL_NQ - 2]].all() and cnt.max() == SMALL_N
    rng = np.random.default_rng(31)
    r["mask"] = rng.random(SMALL_N) < 0.5
    r["masks"] = rng.random((SMALL_NQ, SMALL_N), dtype=np.float32) < rng.choice([0.0, 0.1, 0.5, 1.0], SMALL_NQ).astype(np.float32)[:, None]
    return r


@pytest.mark.parametrize("form", ["unfiltered", "single", "each"])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_batch_of_two_slices_by_the_grid_bound(native_lib, metric, form):
    """65600 queries on 70 rows: the 65535 / tq bound cuts the batch into a slice of 65504 queries and one of 96 at the default
    budget, and range_lims_kernel scans 64 trips of 1024 totals.  lims and the whole CSR against the float64 reference."""
    from hnsw_clj_amd import engine

    r = _small(metric)
    G, gps, _ = S.slicing(SMALL_N, 20, SMALL_NQ, each=form == "each")
    assert gps * 32 == 65504 and G * 32 == SMALL_NQ and G - gps == 3
    mask = {"unfiltered": None, "single": r["mask"][None, :], "each": r["masks"]}[form]
    want = S.csr(r["within"], r["bd"], mask)
    with engine.Index(r["base"], metric, 0) as idx:
        call = {"unfiltered": lambda **kw: idx.range_search(r["Q"], r["rad"], **kw),
                "single": lambda **kw: idx.range_search_filtered(r["Q"], r["rad"], engine.pack_mask(r["mask"], SMALL_N), **kw),
                "each": lambda **kw: idx.range_search_filtered_each(r["Q"], r["rad"], S.pack_rows(r["masks"]), **kw)}[form]
        S.same(call(), want, "id order")
        S.same(call(by_distance=True), S.by_distance(want), "distance order")


@pytest.mark.parametrize("nq", [1025, 1089])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_lims_scan_past_one_trip(native_lib, metric, nq):
    """range_lims_kernel alone: a second trip of its 1024-wide loop (one query; 65 queries = a wave and one), the carry between the
    trips, the cross-wave prefix inside a trip; queries without hits at 63, 64, 1023, 1024 and in the last slot."""
    from hnsw_clj_amd import engine

    r = _small(metric)
    want = S.csr(r["within"][:nq], r["bd"])
    assert want[0][nq] == want[0][nq - 1] and want[0][1024] == want[0][1023] > 0
    with engine.Index(r["base"], metric, 0) as idx:
        S.same(idx.range_search(r["Q"][:nq], r["rad"][:nq]), want)
        S.same(idx.range_search_filtered(r["Q"][:nq], r["rad"][:nq], engine.pack_mask(r["mask"], SMALL_N)),
               S.csr(r["within"][:nq], r["bd"], r["mask"][None, :]), "single mask")


# ---- sort lengths and keys ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tied(metric):
    from hnsw_clj_amd import engine

    base, q = S.tied_data(metric)
    n, nq = len(base), len(S.SORT_LENGTHS)
    dv = S.d64(metric, q[None, :], base)
    with engine.Index(base, metric, 0) as idx:
        bd = idx.batch_distances(q)[None, :]
    s = np.sort(bd[0].astype(np.float64))                                 # radii from the sorted batch_distances
    rad64 = np.array([0.5 * (s[L - 1] + s[L]) if L < n else s[-1] + 1.0 for L in S.SORT_LENGTHS])
    gap = np.array([s[L] - s[L - 1] if L < n else np.inf for L in S.SORT_LENGTHS])
    S.guard(gap, np.abs(S.d32(metric, q[None, :], base).astype(np.float64) - dv).max(1), nq, rad64)
    S.guard(gap, np.abs(bd.astype(np.float64) - dv).max(1), nq, rad64)
    within = dv <= rad64[:, None]
    assert tuple(within.sum(1)) == S.SORT_LENGTHS                         # 4096 +- 1 and 8192 +- 1 among them, exactly
    assert len(np.unique(bd)) == nq                                       # 17 distinct distances: everything else is a tie
    return dict(base=base, Q=np.ascontiguousarray(np.repeat(q[None, :], nq, 0)), rad=rad64.astype(np.float32), within=within, bd=bd)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_sort_lengths_at_the_network_boundaries(native_lib, metric, masked):
    """Segments of 2, 3, 4, 5, 1023 .. 1025, 4095 .. 4097 (one LDS tile), 8191 .. 8193 (two), 12288, 16384, 16385 and 16500
    entries of heavily tied, exact distances (dot: negative keys, and one row at distance -0, which comes back as +0 in
    distance order and as -0 in id order); under a mask the pass list moves every position and the ids still break the ties."""
    from hnsw_clj_amd import engine

    r = _tied(metric)
    n = len(r["base"])
    m = np.random.default_rng(37).random(n) < 0.6 if masked else None
    want = S.csr(r["within"], r["bd"], None if m is None else m[None, :])
    want_d = S.by_distance(want)
    minus0 = np.uint32(0x80000000)
    if metric == "dot":
        assert (want[2] == minus0).any() and not (want_d[2] == minus0).any()
        assert (r["bd"] < 0).any() and (r["bd"] > 0).any()
    with engine.Index(r["base"], metric, 0) as idx:
        if masked:
            call = lambda **kw: idx.range_search_filtered(r["Q"], r["rad"], engine.pack_mask(m, n), **kw)
        else:
            call = lambda **kw: idx.range_search(r["Q"], r["rad"], **kw)
        got = call()
        S.same(got, want, "id order")
        got_d = call(by_distance=True)
        S.same(got_d, want_d, "distance order")
    for q in range(len(S.SORT_LENGTHS)):                                  # the expected order, restated per segment
        a, b = got[0][q], got[0][q + 1]
        o = np.lexsort((got[1][a:b], got[2][a:b]))
        assert np.array_equal(got_d[1][a:b], got[1][a:b][o]), q


# ---- cap under HNSWGPU_RANGE_BY_DISTANCE on the _dev entries -----------------------------------------------------------------
@pytest.mark.parametrize("form", ["unfiltered", "single", "each"])
def test_dev_cap_in_distance_order(native_lib, form):
    """range_sort_kernel clips a segment to cap (s0 / s1): the segments wholly below cap come out in distance order, nothing at
    or past cap is written, lims is complete; the cut segment holds rows of its query's set, in no promised order."""
    import torch
    from test_range_search_filtered_gpu import NQ, N as N549, _mask, _masks_each as masks549, _ref

    from hnsw_clj_amd import engine

    base, Q, rad, within, _, _ = _ref("cosine", 260)
    dq, dr = torch.from_numpy(Q).cuda(), torch.from_numpy(rad).cuda()
    with engine.Index(base, "cosine", 0) as idx:
        if form == "unfiltered":
            allowed = within
            host = lambda: idx.range_search(Q, rad, by_distance=True)
            dev = lambda cap, out: idx.range_search_dev(dq, dr, cap, by_distance=True, out=out)
        elif form == "single":
            m = _mask("half")
            allowed = within & m[None, :]
            dm = torch.from_numpy(engine.pack_mask(m, N549).view(np.int32)).cuda()
            host = lambda: idx.range_search_filtered(Q, rad, engine.pack_mask(m, N549), by_distance=True)
            dev = lambda cap, out: idx.range_search_filtered_dev(dq, dr, dm, cap, by_distance=True, out=out)
        else:
            M = masks549()
            allowed = within & M
            dm = torch.from_numpy(engine.pack_masks(M, N549).view(np.int32)).cuda()
            host = lambda: idx.range_search_filtered_each(Q, rad, engine.pack_masks(M, N549), by_distance=True)
            dev = lambda cap, out: idx.range_search_filtered_each_dev(dq, dr, dm, cap, by_distance=True, out=out)
        lims, ids, d = host()
        total, cnt = int(lims[-1]), np.diff(lims)
        assert np.array_equal(cnt, allowed.sum(1))
        busy = np.flatnonzero(cnt >= 8)
        cut = int(busy[len(busy) // 2])                                   # a segment that is neither the first nor the last
        assert lims[cut] > 0 and lims[cut + 1] < total
        for cap in (int(lims[cut]) + int(cnt[cut]) // 2, int(lims[cut])):  # inside the segment; exactly on its boundary
            out = (torch.full((NQ + 1,), -1, dtype=torch.int64, device="cuda"), torch.full((total + 8,), -7, dtype=torch.int32, device="cuda"),
                   torch.full((total + 8,), -7.0, dtype=torch.float32, device="cuda"))
            dev(cap, out)
            torch.cuda.synchronize()
            gl, gi, gd = (t.cpu().numpy() for t in out)
            assert np.array_equal(gl, lims), cap                          # complete
            assert (gi[cap:] == -7).all() and (gd[cap:] == -7.0).all(), cap
            whole = int(lims[cut])                                        # the segments below `cut` lie wholly below cap
            assert np.array_equal(gi[:whole], ids[:whole]) and np.array_equal(gd[:whole].view(np.uint32), d[:whole].view(np.uint32)), cap
            part = gi[whole:cap]
            assert len(set(part)) == len(part) and allowed[cut, part].all(), cap
