"""Filtered search with one allow-mask per query on the device, against the unmodified oracle (ids identical, distance bits
identical).

Exact scan: per DISTINCT mask of a family, expected = O.exact_knn(base[pid], Q[qs], K_MAX, metric, MODE_DEV) with pid =
flatnonzero(bits) and qs the queries that bring this mask, ids mapped through pid.  One expectation per (shape, metric, family)
at 70 queries and k = 100; a smaller batch is a prefix of its rows and a smaller k a prefix of its columns (the search is exact
and every query independent).

HNSW: expected = O.hnsw_search(base, g, Q, kk, ef') once per ef; per query the ids >= 0 that pass ITS mask, the first k of them.

Slices (FILTER_EACH_MB): 1000 x 128, `overlap`, 70 queries at 1 MiB was planned as the case of "at least 2 slices".  The dense array of
that batch is 3 groups x 32 queries x <= 1000 positions x 4 bytes = 375 KiB, so a 1 MiB bound cannot cut it, whatever the
implementation; that case is run at 1 MiB for equal results, and the slice count is asserted where the bound bites: 40000 x 32,
where ONE group's dense array is 32 x 40000 x 4 bytes = 4.9 MiB, so every group of the 70 queries is a slice of its own (3)."""
import numpy as np
import pytest

from util import assert_exact

pytestmark = pytest.mark.gpu

SHAPES = [(33, 7), (1000, 128), (300, 768), (70, 1536), (70, 3072), (40000, 32)]
FAMILIES = ["same", "disjoint", "overlap", "tenants3", "mixed"]
NQS = [1, 33, 70]
KS = [1, 10, 100]
NQ_MAX, K_MAX = 70, 100
OM = {"cosine": "COSINE", "l2": "L2", "dot": "DOT"}


def _cases():
    for shape in SHAPES:
        for metric in ("cosine", "l2", "dot"):
            if shape[0] == 40000 and metric == "dot":
                continue
            yield pytest.param(shape, metric, id="%dx%d-%s" % (shape + (metric,)))


def _family(name, n, seed):
    """[70][n] bool: the masks of the 70 queries."""
    rng = np.random.default_rng(seed)
    b = np.zeros((NQ_MAX, n), np.bool_)
    if name == "same":
        b[:] = rng.random(n) < 0.5
    elif name == "disjoint":                                        # query q: rows q, q + 70, ...
        for q in range(NQ_MAX):
            b[q, q::NQ_MAX] = True
    elif name == "overlap":
        b = rng.random((NQ_MAX, n)) < 0.5
    elif name == "tenants3":
        t = rng.integers(0, 3, n)
        for q in range(NQ_MAX):
            b[q] = t == (q * 7 + q // 5) % 3
    elif name == "mixed":
        b = rng.random((NQ_MAX, n)) < 0.03
        b[0] = False
        b[1] = True
        b[NQ_MAX - 1] = False
        b[NQ_MAX - 1, n - 1] = True
        b[32:40] = False                                            # an empty whole group at 8 queries per group
    return b


def _garbage_past_n(masks, n, seed):
    """Random bits at the positions >= n of every row's last word: the library must ignore them."""
    m = masks.copy()
    if n & 31:
        g = np.random.default_rng(seed).integers(0, 1 << 32, len(m), dtype=np.uint64)
        m[:, -1] |= (((g >> np.uint64(n & 31)) << np.uint64(n & 31)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return m


def _expect_each(O, base, Q, bits, om, kmax=K_MAX):
    """Per distinct mask one oracle call over the rows it lets pass, for the queries that bring it."""
    nq = len(Q)
    ids = np.full((nq, kmax), -1, np.int32)
    d = np.full((nq, kmax), np.inf, np.float64)
    groups = {}
    for q in range(nq):
        groups.setdefault(bits[q].tobytes(), []).append(q)
    for qs in groups.values():
        pid = np.flatnonzero(bits[qs[0]])
        if len(pid):
            oi, od, _ = O.exact_knn(base[pid], Q[qs], kmax, metric=om, mode=O.MODE_DEV)
            ids[qs] = np.where(oi >= 0, pid[np.maximum(oi, 0)], -1)
            d[qs] = od
    return ids, d


def _dev(torch, masks):
    return torch.from_numpy(np.ascontiguousarray(masks).view(np.int32).copy()).to(torch.device("cuda", 0))


def _only_allowed(gi, bits, what):
    for q in range(len(gi)):
        got = gi[q][gi[q] >= 0]
        assert bits[q][got].all(), "%s: query %d was given a row its mask does not allow" % (what, q)


@pytest.mark.parametrize("shape,metric", _cases())
def test_exact_knn_filtered_each_matches_the_oracle_per_query(native_lib, oracle, shape, metric):
    import torch

    from hnsw_clj_amd import datagen, engine

    O = oracle
    om = getattr(O, OM[metric])
    n, dim = shape
    base = datagen.generate_dataset(n, dim)
    Q = datagen.generate_dataset(NQ_MAX, dim, seed=43)
    Qd = torch.from_numpy(Q).to(torch.device("cuda", 0))
    side = torch.cuda.Stream()
    tq = 32 if dim <= 1024 else (16 if dim <= 2048 else 8)
    with engine.Index(base, metric, 0) as idx:
        for fi, fam in enumerate(FAMILIES):
            bits = _family(fam, n, 200 + fi)
            ei, ed = _expect_each(O, base, Q, bits, om)
            masks = engine.pack_masks(bits, n)
            if fam == "mixed":
                masks = _garbage_past_n(masks, n, 11)
                assert (ei[0] == -1).all() and (ei[1] >= 0).sum() == min(n, K_MAX) and list(ei[NQ_MAX - 1][:2]) == [n - 1, -1]
                assert (ei[32:40] == -1).all()
            md = _dev(torch, masks)
            torch.cuda.synchronize()
            combos = [(nq, KS[(fi + j) % len(KS)]) for j, nq in enumerate(NQS)]
            if fam == "disjoint" and (NQ_MAX, K_MAX) not in combos:
                combos.append((NQ_MAX, K_MAX))
            for nq, k in combos:
                what = "%s %dx%d %s nq %d k %d" % (metric, n, dim, fam, nq, k)
                before = native_lib.debug_counter("filtered_each_groups")
                gi, gd = idx.exact_knn_filtered_each(Q[:nq], k, masks[:nq])
                served = native_lib.debug_counter("filtered_each_groups") - before
                assert_exact(gi, gd, ei[:nq, :k], ed[:nq, :k], what + " host")
                _only_allowed(gi, bits, what)
                p = bits[:nq].sum(axis=1)
                for q in np.flatnonzero(p < k):                     # the padding, stated: by the query's OWN count
                    assert (gi[q, p[q]:] == -1).all() and np.isinf(gd[q, p[q]:]).all() and (gi[q, :p[q]] >= 0).all(), what
                ngroups = -(-nq // tq)
                nonempty = sum(bool(bits[g * tq:min(nq, (g + 1) * tq)].any()) for g in range(ngroups))
                assert served == nonempty, what + ": groups served by the group scan"
                with torch.cuda.stream(side):
                    di, dd = idx.exact_knn_filtered_each_dev(Qd[:nq], k, md[:nq])
                side.synchronize()
                assert_exact(di.cpu().numpy(), dd.cpu().numpy(), ei[:nq, :k], ed[:nq, :k], what + " dev")
            if fam == "disjoint" and n <= 1000:                     # k = 100 exceeds every p_q; the union of a group holds more
                assert (bits.sum(axis=1) < K_MAX).all()
            if fam == "same":                                       # ... is the single-mask call on the whole batch
                si, sd = idx.exact_knn_filtered(Q, 10, masks[0])
                gi, gd = idx.exact_knn_filtered_each(Q, 10, masks)
                assert np.array_equal(gi, si) and np.array_equal(gd.view(np.uint32), sd.view(np.uint32))
            if n <= 1000:                                           # row q is the single-mask call for query q alone
                gi, gd = idx.exact_knn_filtered_each(Q, 10, masks)
                for q in (0, 1, 7, 31, 32, 33, 39, 40, 69):
                    si, sd = idx.exact_knn_filtered(Q[q:q + 1], 10, masks[q])
                    assert np.array_equal(gi[q], si[0]) and np.array_equal(gd[q].view(np.uint32), sd[0].view(np.uint32)), (fam, q)


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_each_ties_go_to_the_lower_allowed_row(native_lib, oracle, metric):
    from hnsw_clj_amd import datagen, engine

    O = oracle
    om = getattr(O, OM[metric])
    base = datagen.generate_dataset(1000, 128).copy()
    base[17] = base[5]
    base[40] = base[5]
    Q = np.repeat(base[5:6], 6, axis=0)
    bits = np.ones((6, 1000), np.bool_)
    bits[:, ::7] = False
    allowed = [(5, 17, 40), (17, 40), (40,), (5, 40), (), (5, 17)]
    for q, rows in enumerate(allowed):
        bits[q, [5, 17, 40]] = False
        bits[q, list(rows)] = True
    ei, ed = _expect_each(O, base, Q, bits, om, 10)
    with engine.Index(base, metric, 0) as idx:
        gi, gd = idx.exact_knn_filtered_each(Q, 10, engine.pack_masks(bits, 1000))
    assert_exact(gi, gd, ei, ed, metric + " ties")
    for q, rows in enumerate(allowed):
        got = [int(r) for r in gi[q] if r in (5, 17, 40)]
        assert got == list(rows)[:len(got)], (q, got)                # in row order, and only the allowed ones
        if metric != "dot":
            assert list(gi[q, :len(rows)]) == list(rows)             # the query is the row itself


def test_each_whole_batch_empty(native_lib):
    import torch

    from hnsw_clj_amd import datagen, engine

    base = datagen.generate_dataset(1000, 128)
    Q = datagen.generate_dataset(NQ_MAX, 128, seed=43)
    masks = engine.pack_masks(np.zeros((NQ_MAX, 1000), np.bool_), 1000)
    with engine.Index(base, "cosine", 0) as idx:
        before = native_lib.debug_counter("filtered_each_groups")
        gi, gd = idx.exact_knn_filtered_each(Q, 10, masks)
        assert (gi == -1).all() and np.isinf(gd).all() and (gd > 0).all()
        di, dd = idx.exact_knn_filtered_each_dev(torch.from_numpy(Q).cuda(), 10, _dev(torch, masks))
        torch.cuda.synchronize()
        assert (di.cpu().numpy() == -1).all() and np.isposinf(dd.cpu().numpy()).all()
        assert native_lib.debug_counter("filtered_each_groups") == before   # nothing launched the group scan


@pytest.mark.parametrize("shape,min_slices", [((1000, 128), 1), ((40000, 32), 3)], ids=["1000x128", "40000x32"])
def test_each_slices_by_filter_each_mb(native_lib, oracle, tune, shape, min_slices):
    from hnsw_clj_amd import datagen, engine

    n, dim = shape
    base = datagen.generate_dataset(n, dim)
    Q = datagen.generate_dataset(NQ_MAX, dim, seed=43)
    bits = _family("overlap", n, 202)
    masks = engine.pack_masks(bits, n)
    others = [c for c in native_lib.LAUNCH_COUNTERS if c != "filtered_each_groups"]
    with engine.Index(base, "cosine", 0) as idx:
        idx.set_profiling(True)
        idx.get_profile(engine.PROF_IVF_SCAN)
        wi, wd = idx.exact_knn_filtered_each(Q, 10, masks)
        _, one = idx.get_profile(engine.PROF_IVF_SCAN)
        assert one == 1                                             # the default bound: one slice
        tune.set("FILTER_EACH_MB", 1)
        before = native_lib.debug_counter("filtered_each_groups")
        rest = [native_lib.debug_counter(c) for c in others]
        gi, gd = idx.exact_knn_filtered_each(Q, 10, masks)
        _, slices = idx.get_profile(engine.PROF_IVF_SCAN)
        print("FILTER_EACH_MB 1 at %dx%d: %d slices" % (n, dim, slices))
        assert slices >= min_slices
        assert np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))
        assert native_lib.debug_counter("filtered_each_groups") - before == 3        # ceil(70 / 32), however they are sliced
        assert [native_lib.debug_counter(c) for c in others] == rest
    ei, ed = _expect_each(oracle, base, Q[:3], bits[:3], oracle.COSINE, 10)
    assert_exact(gi[:3], gd[:3], ei, ed, "sliced")


@pytest.mark.parametrize("shape", [(33, 7), (300, 768), (70, 3072)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_single_mask_call_equals_each_call_with_that_mask_for_every_query(native_lib, metric, shape):
    """Both forms of the mask run one chain, so they are pinned against each other directly: exact_knn_filtered(Q, k, m) and
    exact_knn_filtered_each(Q, k, [m] * 70) agree in ids and distance bits, host and device entries.  32 / 32 / 8 queries per
    group: 70 queries are 3 / 3 / 9 groups with a ragged last one.  Masks: p not a multiple of 4 (a dense stride that differs
    between the forms), none, only row n - 1, all.  The single call moves no launch counter and times one scan (none at p = 0);
    the each call counts its groups -- every one, since every group's union is m, and none at p = 0 -- and nothing else."""
    import torch

    from hnsw_clj_amd import datagen, engine

    n, dim = shape
    base = datagen.generate_dataset(n, dim)
    Q = datagen.generate_dataset(NQ_MAX, dim, seed=43)
    Qd = torch.from_numpy(Q).to(torch.device("cuda", 0))
    tq = 32 if dim <= 1024 else (16 if dim <= 2048 else 8)
    odd = np.random.default_rng(77).random(n) < 0.5
    while odd.sum() % 4 == 0 or not odd.any():
        odd[np.flatnonzero(~odd)[0]] = True
    last = np.zeros(n, np.bool_)
    last[n - 1] = True
    counters = lambda: [native_lib.debug_counter(c) for c in native_lib.LAUNCH_COUNTERS]  # noqa: E731
    at = native_lib.LAUNCH_COUNTERS.index("filtered_each_groups")
    with engine.Index(base, metric, 0) as idx:
        idx.set_profiling(True)
        for name, bits in (("odd", odd), ("none", np.zeros(n, np.bool_)), ("last", last), ("all", np.ones(n, np.bool_))):
            p = int(bits.sum())
            assert name != "odd" or p % 4
            m = _garbage_past_n(engine.pack_mask(bits, n)[None, :], n, 3)[0]
            rows = np.repeat(m[None, :], NQ_MAX, axis=0)
            md, rd = _dev(torch, m), _dev(torch, rows)
            torch.cuda.synchronize()
            for k in (1, 100):
                what = "%s %dx%d mask %s (p %d) k %d" % (metric, n, dim, name, p, k)
                idx.get_profile(engine.PROF_IVF_SCAN)
                c0 = counters()
                si, sd = idx.exact_knn_filtered(Q, k, m)
                assert counters() == c0, what + ": the single-mask call moved a launch counter"
                assert idx.get_profile(engine.PROF_IVF_SCAN)[1] == (1 if p else 0), what + ": scans of the single-mask call"
                ei, ed = idx.exact_knn_filtered_each(Q, k, rows)
                c1 = counters()
                want = list(c0)
                want[at] += -(-NQ_MAX // tq) if p else 0
                assert c1 == want, what + ": launch counters of the each call"
                assert np.array_equal(si, ei) and np.array_equal(sd.view(np.uint32), ed.view(np.uint32)), what + " host"
                filled = min(p, k)
                assert (si[:, :filled] >= 0).all() and (si[:, filled:] == -1).all() and np.isposinf(sd[:, filled:]).all(), what
                if name == "last":
                    assert (si[:, 0] == n - 1).all(), what
                idx.get_profile(engine.PROF_IVF_SCAN)
                di, dd = idx.exact_knn_filtered_dev(Qd, k, md)
                torch.cuda.synchronize()
                assert counters() == c1, what + ": the single-mask device call moved a launch counter"
                assert idx.get_profile(engine.PROF_IVF_SCAN)[1] == (1 if p else 0), what + ": scans of the single-mask device call"
                gi, gd = idx.exact_knn_filtered_each_dev(Qd, k, rd)
                torch.cuda.synchronize()
                want[at] += -(-NQ_MAX // tq) if p else 0
                assert counters() == want, what + ": launch counters of the each device call"
                assert torch.equal(di, gi) and torch.equal(dd.view(torch.int32), gd.view(torch.int32)), what + " dev"
                assert np.array_equal(di.cpu().numpy(), si) and np.array_equal(dd.cpu().numpy().view(np.uint32), sd.view(np.uint32)), what


# ---- the traversal path -----------------------------------------------------------------------------------------------------
N, DIM, K, NQ_H = 1000, 128, 10, 70
EFS = [50, 200]


@pytest.fixture(scope="module")
def hnsw(native_lib, oracle):
    import torch

    from hnsw_clj_amd import datagen, engine

    O = oracle
    assert engine.device_count() >= 1, "no GPU visible"
    base = datagen.generate_dataset(N, DIM)
    Q = datagen.generate_dataset(NQ_H, DIM, seed=43)
    g = O.hnsw_build(base, metric=O.COSINE, M=16, ef_construction=40, mode=O.MODE_DEV)
    idx = engine.Index(base, "cosine", 0)
    idx.set_graph(g)
    want = {}
    for ef in EFS:
        oi, od, ost, _ = O.hnsw_search(base, g, Q, min(ef, 1024), ef=ef, metric=O.COSINE, mode=O.MODE_DEV)
        want[ef] = (oi, od, ost)
    Qd = torch.from_numpy(Q).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    yield idx, base, Q, Qd, g, want
    idx.close()


def _take_each(oi, od, bits, k):
    ids = np.full((len(oi), k), -1, np.int32)
    d = np.full((len(oi), k), np.inf, np.float64)
    for q in range(len(oi)):
        keep = [j for j in range(oi.shape[1]) if oi[q, j] >= 0 and bits[q, oi[q, j]]][:k]
        ids[q, :len(keep)] = oi[q, keep]
        d[q, :len(keep)] = od[q, keep]
    return ids, d


@pytest.mark.parametrize("fam", FAMILIES + ["ones"])
@pytest.mark.parametrize("ef", EFS)
def test_hnsw_search_filtered_each_takes_by_the_querys_own_mask(hnsw, ef, fam):
    import torch

    from hnsw_clj_amd import engine

    idx, base, Q, Qd, g, want = hnsw
    oi, od, ost = want[ef]
    bits = np.ones((NQ_H, N), np.bool_) if fam == "ones" else _family(fam, N, 300)
    masks = _garbage_past_n(engine.pack_masks(bits, N), N, 5)
    md = _dev(torch, masks)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for nq in NQS:
        what = "%s ef %d nq %d" % (fam, ef, nq)
        ei, ed = _take_each(oi[:nq], od[:nq], bits, K)
        gi, gd, gs = idx.hnsw_search_filtered_each(Q[:nq], K, masks[:nq], ef, want_stats=True)
        assert_exact(gi, gd, ei, ed, what + " host")
        assert np.array_equal(gs, ost[:nq]), what + " host: stats"
        _only_allowed(gi, bits, what)
        stats = torch.zeros((nq, 2), dtype=torch.int64, device=Qd.device)
        with torch.cuda.stream(side):
            di, dd = idx.hnsw_search_filtered_each_dev(Qd[:nq], K, md[:nq], ef, stats=stats)
        side.synchronize()
        assert_exact(di.cpu().numpy(), dd.cpu().numpy(), ei, ed, what + " dev")
        assert np.array_equal(stats.cpu().numpy(), ost[:nq]), what + " dev: stats"
    for q in (0, 1, 33, 69):                                        # the single-mask call for query q alone, stats included
        si, sd, ss = idx.hnsw_search_filtered(Q[q:q + 1], K, masks[q], ef, want_stats=True)
        assert np.array_equal(gi[q], si[0]) and np.array_equal(gd[q].view(np.uint32), sd[0].view(np.uint32)) and np.array_equal(gs[q], ss[0])
    if fam == "ones":                                               # hnsw_search itself, bit for bit
        ui, ud, us = idx.hnsw_search(Q, K, ef, want_stats=True)
        assert np.array_equal(gi, ui) and np.array_equal(gd.view(np.uint32), ud.view(np.uint32)) and np.array_equal(gs, us)


def _code(eng, fn):
    try:
        fn()
    except eng._native.HnswGpuError as e:
        return e.code
    return 0


def test_each_refusals_leave_the_handle_unchanged(hnsw, native_lib):
    import ctypes

    import torch

    from hnsw_clj_amd import datagen, engine as eng

    idx, base, Q, Qd, g, want = hnsw
    masks = eng.pack_masks(np.ones((4, N), np.bool_), N)
    md = _dev(torch, masks)
    wi, wd = idx.hnsw_search_filtered_each(Q[:4], K, masks, 50)
    L = native_lib.lib()
    ids, d = np.empty((4, K), np.int32), np.empty((4, K), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert L.hnswgpu_exact_knn_filtered_each(idx._h, p(Q), 4, K, None, p(ids), p(d)) == -1
    assert b"allow is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_hnsw_search_filtered_each(idx._h, p(Q), 4, K, 50, None, p(ids), p(d), None) == -1
    assert L.hnswgpu_exact_knn_filtered_each_dev(idx._h, Qd.data_ptr(), 4, K, None, p(ids), p(d), None) == -1
    assert L.hnswgpu_hnsw_search_filtered_each_dev(idx._h, Qd.data_ptr(), 4, K, 50, None, p(ids), p(d), None, None) == -1
    assert L.hnswgpu_exact_knn_filtered_each(idx._h, p(Q), 0, K, None, p(ids), p(d)) == -1       # null mask before nq == 0, as the single-mask call
    assert L.hnswgpu_exact_knn_filtered_each(idx._h, p(Q), 0, K, p(masks), p(ids), p(d)) == 0
    assert L.hnswgpu_hnsw_search_filtered_each(idx._h, p(Q), 0, K, 50, p(masks), p(ids), p(d), None) == 0
    assert _code(eng, lambda: idx.exact_knn_filtered_each(Q[:4], 1025, masks)) == -5
    assert _code(eng, lambda: idx.hnsw_search_filtered_each(Q[:4], K, masks, 4097)) == -5      # hnsw_search's limit
    with eng.Index(base, "cosine", 0) as bare:                      # no graph
        assert _code(eng, lambda: bare.hnsw_search_filtered_each(Q[:4], K, masks, 50)) == -3
        assert _code(eng, lambda: bare.hnsw_search_filtered_each_dev(Qd[:4], K, md, 50)) == -3
        gi, gd = bare.exact_knn_filtered_each(Q[:4], K, masks)      # ... the exact scan needs none
        ei, ed = bare.exact_knn(Q[:4], K)
        assert np.array_equal(gi, ei)
    with eng.Index(base, "cosine", 0) as forest:
        forest.hnsw_build_parts(np.array([0, 400, N], np.int64), 8, 40, 42)
        for fn in (lambda: forest.hnsw_search_filtered_each(Q[:4], K, masks, 50),
                   lambda: forest.hnsw_search_filtered_each_dev(Qd[:4], K, md, 50)):
            with pytest.raises(eng._native.HnswGpuError, match="parts|forest") as e:
                fn()
            assert e.value.code == -3
        torch.cuda.synchronize()
        assert forest.n == N
    gi, gd = idx.hnsw_search_filtered_each(Q[:4], K, masks, 50)     # the handle is unchanged
    assert np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))
    with eng.Index(np.zeros((0, DIM), np.float32), "cosine", 0) as empty:   # n == 0: the host entries fill the padding
        z = np.zeros((2, 0), np.uint32)
        gi, gd = empty.exact_knn_filtered_each(Q[:2], 3, z)
        assert (gi == -1).all() and np.isposinf(gd).all()
    assert datagen is not None


def test_mirror_search_batch_filtered_each_is_search_knn_filtered_per_query(hnsw):
    from hnsw_clj_amd import ultra_fast

    idx, base, Q, Qd, g, want = hnsw

    class G:
        pass

    graph = G()
    graph.index, graph.ids, graph.M, graph.ef_construction = idx, ["row-%d" % i for i in range(N)], 16, 40
    rng = np.random.default_rng(9)
    sparse, half, third = rng.random(N) < 0.03, rng.random(N) < 0.5, rng.random(N) < 0.3
    fns = [sparse, half, (lambda s: int(s[4:]) % 3 == 0), third, np.zeros(N, bool), half, sparse, np.ones(N, bool), half.copy()]
    plans = {ultra_fast.filtered_plan(N, int(np.sum(ultra_fast._allow_bits(graph, f))), K)[0] for f in fns}
    assert plans == {"scan", "graph"}                               # queries on both sides of filtered_plan
    out = ultra_fast.search_batch_filtered_each(graph, Q[:len(fns)], K, fns)
    for q, f in enumerate(fns):
        assert out[q] == ultra_fast.search_knn_filtered(graph, Q[q], K, f), q
    same = ultra_fast.search_batch_filtered_each(graph, Q[:3], K, [half, half, half.copy()])
    assert same == ultra_fast.search_batch_filtered(graph, Q[:3], K, half)


def test_each_calls_on_two_streams_with_a_plain_search_between(hnsw):
    """hg::Call orders the handle's scratch across streams: two _each calls on two streams with a plain search between them and
    no synchronise return the bits of the calls run alone (tests/test_call_ordering.py)."""
    import torch

    from hnsw_clj_amd import engine

    idx, base, Q, Qd, g, want = hnsw
    nq, ef = 64, 64
    dev = Qd.device
    m1 = _dev(torch, engine.pack_masks(_family("overlap", N, 1)[:nq], N))
    m2 = _dev(torch, engine.pack_masks(_family("tenants3", N, 2)[:nq], N))

    def out():
        return torch.empty((nq, K), dtype=torch.int32, device=dev), torch.empty((nq, K), dtype=torch.float32, device=dev)

    calls = [
        lambda o: idx.exact_knn_filtered_each_dev(Qd[:nq], K, m1, out=o),
        lambda o: idx.hnsw_search_dev(Qd[:nq], K, ef, out=o),
        lambda o: idx.hnsw_search_filtered_each_dev(Qd[:nq], K, m2, ef, out=o),
        lambda o: idx.exact_knn_dev(Qd[:nq], K, out=o),
        lambda o: idx.exact_knn_filtered_each_dev(Qd[:nq], K, m2, out=o),
    ]
    alone = []
    for c in calls:
        o = out()
        c(o)
        torch.cuda.synchronize()
        alone.append(o)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for rep in range(4):
        outs = [out() for _ in calls]
        for i, c in enumerate(calls):
            with torch.cuda.stream(streams[(i + rep) % 2]):
                c(outs[i])
        torch.cuda.synchronize()
        for i, (o, w) in enumerate(zip(outs, alone)):
            assert torch.equal(o[0], w[0]) and torch.equal(o[1].view(torch.int32), w[1].view(torch.int32)), (rep, i)
