"""Filtered search on the device against the unmodified oracle (ids identical, distance bits identical).

Exact scan: expected = O.exact_knn(base[pid], Q, k, metric, MODE_DEV) with pid = flatnonzero(allow), ids mapped through pid --
which equals "full exact list, drop the failing rows, take k".  One expectation per (shape, metric, mask) at the largest nq and
k; a smaller nq is a prefix of its rows and a smaller k a prefix of its columns (the search is exact and every query is
independent), so each (nq, k) case is compared with that slice.

HNSW: expected = O.hnsw_search(base, g, Q, kk, ef=ef', MODE_DEV) with ef' the effective ef and kk = min(ef', 1024); per query
the ids >= 0 that pass, the first k of them, padded; stats are the oracle's, unchanged."""
import numpy as np
import pytest

from util import assert_exact

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "l2", "dot"]
SHAPES = [(1, 4), (33, 7), (1000, 128), (5000, 96), (300, 768), (70, 1536), (70, 3072)]
MASKS = ["ones", "zeros", "last", "every32", "half", "sparse"]
NQS = [1, 12, 33, 70]     # one group; a group and a remainder at 8 / 16 queries per group; two groups and a remainder at 32
KS = [1, 10, 64, 100]
NQ_MAX, K_MAX = 70, 100


def _bits(name, n, seed):
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
    return b


def _garbage_past_n(mask, n, seed):
    """Random bits at the positions >= n of the last word: the library must ignore them."""
    m = mask.copy()
    if n & 31:
        g = np.random.default_rng(seed).integers(0, 1 << 32, dtype=np.uint64)
        m[-1] |= np.uint32((int(g) >> (n & 31)) << (n & 31) & 0xFFFFFFFF)
    return m


def _expect_exact(O, base, Q, bits, metric):
    nq = len(Q)
    pid = np.flatnonzero(bits)
    ids = np.full((nq, K_MAX), -1, np.int32)
    d = np.full((nq, K_MAX), np.inf, np.float64)
    if len(pid):
        oi, od, _ = O.exact_knn(base[pid], Q, K_MAX, metric=metric, mode=O.MODE_DEV)
        ids = np.where(oi >= 0, pid[np.maximum(oi, 0)], -1).astype(np.int32)
        d = od
    return ids, d


def _dev_mask(torch, mask):
    return torch.from_numpy(mask.view(np.int32).copy()).to(torch.device("cuda", 0))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("metric", METRICS)
def test_exact_knn_filtered_matches_the_oracle_on_the_passing_rows(native_lib, oracle, metric, shape):
    import torch

    from hnsw_clj_amd import datagen, engine

    O = oracle
    om = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    n, dim = shape
    base = datagen.generate_dataset(n, dim)
    Q = datagen.generate_dataset(NQ_MAX, dim, seed=43)
    Qd = torch.from_numpy(Q).to(torch.device("cuda", 0))
    side = torch.cuda.Stream()
    with engine.Index(base, metric, 0) as idx:
        for mi, name in enumerate(MASKS):
            bits = _bits(name, n, 100 + mi)
            p = int(bits.sum())
            mask = engine.pack_mask(bits, n)
            if shape in ((33, 7), (1000, 128)):
                mask = _garbage_past_n(mask, n, 7 + mi)
            ei, ed = _expect_exact(O, base, Q, bits, om)
            if name == "ones":
                oi, od, _ = O.exact_knn(base, Q, K_MAX, metric=om, mode=O.MODE_DEV)
                assert np.array_equal(oi, ei) and np.array_equal(od, ed, equal_nan=True)
            if name == "zeros":
                assert p == 0 and (ei == -1).all() and np.isinf(ed).all()
            md = _dev_mask(torch, mask)
            torch.cuda.synchronize()
            for j, k in enumerate(KS):
                nq = NQS[(mi + j) % len(NQS)]
                what = "%s %dx%d mask %s (p %d) nq %d k %d" % (metric, n, dim, name, p, nq, k)
                gi, gd = idx.exact_knn_filtered(Q[:nq], k, mask)
                assert_exact(gi, gd, ei[:nq, :k], ed[:nq, :k], what + " host")
                if k > p:                                           # the padding, stated
                    assert (gi[:, p:] == -1).all() and np.isinf(gd[:, p:]).all() and (gi[:, :p] >= 0).all(), what
                assert bits[gi[gi >= 0]].all(), what + ": a failing row was returned"
                with torch.cuda.stream(side):
                    di, dd = idx.exact_knn_filtered_dev(Qd[:nq], k, md)
                side.synchronize()
                assert_exact(di.cpu().numpy(), dd.cpu().numpy(), ei[:nq, :k], ed[:nq, :k], what + " dev")


@pytest.mark.parametrize("metric", METRICS)
def test_exact_knn_filtered_ties_go_to_the_lower_row(native_lib, oracle, metric):
    from hnsw_clj_amd import datagen, engine

    O = oracle
    om = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    base = datagen.generate_dataset(1000, 128).copy()
    base[17] = base[5]
    base[40] = base[5]
    Q = np.concatenate([base[5:6], datagen.generate_dataset(11, 128, seed=43)])
    bits = np.ones(1000, np.bool_)
    bits[::7] = False
    bits[[5, 17, 40]] = True
    ei, ed = _expect_exact(O, base, Q, bits, om)
    with engine.Index(base, metric, 0) as idx:
        gi, gd = idx.exact_knn_filtered(Q, 10, engine.pack_mask(bits, 1000))
    assert_exact(gi, gd, ei[:, :10], ed[:, :10], metric + " ties")
    for q in range(len(Q)):                                        # wherever the three equal rows appear, they appear in row order
        pos = [list(gi[q]).index(r) for r in (5, 17, 40) if r in gi[q]]
        assert pos == sorted(pos)
        got = [r for r in gi[q] if r in (5, 17, 40)]
        assert got == [5, 17, 40][:len(got)]
    if metric != "dot":
        assert list(gi[0, :3]) == [5, 17, 40]                      # the query is the row itself


# ---- HNSW ------------------------------------------------------------------------------------------------------------------
N, DIM, K, NQ_H = 1000, 128, 10, 300
EFS = [None, 50, 200, 1500]
DENSITIES = [1.0, 0.5, 0.1, 0.0]


@pytest.fixture(scope="module")
def hnsw(native_lib, oracle):
    import torch

    from hnsw_clj_amd import datagen, engine

    O = oracle
    assert engine.device_count() >= 1, "no GPU visible"
    base = datagen.generate_dataset(N, DIM)
    Q = datagen.generate_dataset(NQ_H, DIM, seed=43)
    g = O.hnsw_build(base, metric=O.COSINE, M=8, ef_construction=40, mode=O.MODE_DEV)
    idx = engine.Index(base, "cosine", 0)
    idx.set_graph(g)
    want = {}
    for ef in EFS:                                                  # the unfiltered lists, once per ef, shared by every case
        ef2 = max(K, 50) if ef is None else max(ef, K)
        kk = min(ef2, 1024)
        oi, od, ost, _ = O.hnsw_search(base, g, Q, kk, ef=ef2, metric=O.COSINE, mode=O.MODE_DEV)
        want[ef] = (oi, od, ost)
    Qd = torch.from_numpy(Q).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    yield idx, base, Q, Qd, g, want
    idx.close()


def _density_bits(density):
    if density >= 1.0:
        return np.ones(N, np.bool_)
    if density <= 0.0:
        return np.zeros(N, np.bool_)
    return np.random.default_rng(int(density * 100)).random(N) < density


def _take(oi, od, bits, k):
    """Per query: the listed ids >= 0 that pass, the first k of them, -1 / +inf padded."""
    ids = np.full((len(oi), k), -1, np.int32)
    d = np.full((len(oi), k), np.inf, np.float64)
    passing = []
    for q in range(len(oi)):
        keep = [j for j in range(oi.shape[1]) if oi[q, j] >= 0 and bits[oi[q, j]]]
        passing.append(len(keep))
        keep = keep[:k]
        ids[q, :len(keep)] = oi[q, keep]
        d[q, :len(keep)] = od[q, keep]
    return ids, d, passing


def _check_hnsw(torch, idx, Q, Qd, want, ef, density, nq, what):
    from hnsw_clj_amd import engine

    oi, od, ost = want[ef]
    bits = _density_bits(density)
    ei, ed, passing = _take(oi[:nq], od[:nq], bits, K)
    mask = _garbage_past_n(engine.pack_mask(bits, N), N, 3)
    gi, gd, gs = idx.hnsw_search_filtered(Q[:nq], K, mask, ef, want_stats=True)
    assert_exact(gi, gd, ei, ed, what + " host")
    assert np.array_equal(gs, ost[:nq]), what + " host: stats"
    md = _dev_mask(torch, mask)
    stats = torch.zeros((nq, 2), dtype=torch.int64, device=Qd.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        di, dd = idx.hnsw_search_filtered_dev(Qd[:nq], K, md, ef, stats=stats)
    side.synchronize()
    assert_exact(di.cpu().numpy(), dd.cpu().numpy(), ei, ed, what + " dev")
    assert np.array_equal(stats.cpu().numpy(), ost[:nq]), what + " dev: stats"
    if density >= 1.0:                                              # all ones: hnsw_search itself, bit for bit
        ui, ud, us = idx.hnsw_search(Q[:nq], K, ef or 0, want_stats=True)
        assert_exact(gi, gd, ui, ud, what + " against hnsw_search")
        assert np.array_equal(gs, us)
    if density <= 0.0:
        assert (gi == -1).all() and np.isinf(gd).all()
    return passing


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("ef", EFS)
@pytest.mark.parametrize("nq", [1, 12, 300])
def test_hnsw_search_filtered_takes_the_first_passing_entries_of_the_list(hnsw, nq, ef, density):
    import torch

    idx, base, Q, Qd, g, want = hnsw
    passing = _check_hnsw(torch, idx, Q, Qd, want, ef, density, nq, "nq %d ef %s density %g" % (nq, ef, density))
    if ef == 50 and nq == 300:
        if density == 0.1:
            assert min(passing) < K, "the padded case is not exercised"
        if density == 0.5:
            assert min(passing) >= K, "the full rows are not exercised"
    if ef == 1500 and density == 1.0:
        assert (want[ef][0] >= 0).sum(axis=1).max() <= N             # the take sees at most the n valid entries of 1024


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("ef", EFS)
@pytest.mark.parametrize("nq", [1, 12])
def test_hnsw_search_filtered_on_the_helper_kernel(hnsw, tune, nq, ef, density):
    import torch

    idx, base, Q, Qd, g, want = hnsw
    tune.set("SOLO", 0)                                             # small launches: the round-2 helpers instead of several CUs
    _check_hnsw(torch, idx, Q, Qd, want, ef, density, nq, "SOLO 0, nq %d ef %s density %g" % (nq, ef, density))


def test_filtered_call_between_unfiltered_calls_on_two_streams(hnsw):
    """hg::Call orders the handle's scratch buffers across streams: an unfiltered search, a filtered one and an unfiltered one
    again, back to back on two streams without a synchronise, each return the bits of the call run alone."""
    import torch

    from hnsw_clj_amd import engine

    idx, base, Q, Qd, g, want = hnsw
    nq, ef = 64, 64
    bits = _density_bits(0.5)
    md = _dev_mask(torch, engine.pack_mask(bits, N))
    dev = Qd.device

    def out(k=K):
        return torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev)

    calls = [
        lambda o: idx.hnsw_search_dev(Qd[:nq], K, ef, out=o),
        lambda o: idx.hnsw_search_filtered_dev(Qd[:nq], K, md, ef, out=o),
        lambda o: idx.hnsw_search_dev(Qd[:nq], K, 2 * ef, out=o),
        lambda o: idx.exact_knn_filtered_dev(Qd[:nq], K, md, out=o),
        lambda o: idx.hnsw_search_dev(Qd[:nq], K, ef, out=o),
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
def ultra(hnsw):
    from hnsw_clj_amd import ultra_fast

    idx, base, Q, Qd, g, want = hnsw
    graph = ultra_fast.build_index([["v%d" % i, base[i]] for i in range(N)], M=8, ef_construction=40, show_progress=False, graph=g)
    yield graph
    graph.close()


def test_search_batch_filtered_walks_the_graph_when_many_rows_pass(hnsw, ultra):
    from hnsw_clj_amd import engine, ultra_fast

    idx, base, Q, Qd, g, want = hnsw
    pred = lambda s: int(s[1:]) % 2 == 0  # noqa: E731  (a predicate on the caller's String ids)
    bits = np.arange(N) % 2 == 0
    assert ultra_fast.filtered_plan(N, int(bits.sum()), K) == ("graph", 60)
    res = ultra_fast.search_batch_filtered(ultra, Q[:12], K, pred)
    gi, gd = ultra.index.hnsw_search_filtered(Q[:12], K, engine.pack_mask(bits, N), 60)
    assert len(res) == 12
    for q in range(12):
        assert [r["id"] for r in res[q]] == ["v%d" % i for i in gi[q] if i >= 0]
        assert [np.float32(r["distance"]) for r in res[q]] == [d for i, d in zip(gi[q], gd[q]) if i >= 0]
        assert all(pred(r["id"]) for r in res[q])
    assert ultra_fast.search_batch_filtered(ultra, Q[:12], K, bits) == res      # a bool array instead of the predicate


def test_search_batch_filtered_scans_the_passing_rows_when_few_pass(hnsw, ultra):
    from hnsw_clj_amd import engine, ultra_fast

    idx, base, Q, Qd, g, want = hnsw
    pred = lambda s: int(s[1:]) % 50 == 0  # noqa: E731
    bits = np.arange(N) % 50 == 0
    p = int(bits.sum())
    assert p == 20 and ultra_fast.filtered_plan(N, p, K)[0] == "scan"
    for k in (K, 30):
        res = ultra_fast.search_batch_filtered(ultra, Q[:12], k, pred)
        gi, gd = ultra.index.exact_knn_filtered(Q[:12], k, engine.pack_mask(bits, N))
        for q in range(12):
            assert len(res[q]) == min(k, p) and all(pred(r["id"]) for r in res[q])
            assert [r["id"] for r in res[q]] == ["v%d" % i for i in gi[q] if i >= 0]
            assert [np.float32(r["distance"]) for r in res[q]] == [d for i, d in zip(gi[q], gd[q]) if i >= 0]
    assert ultra_fast.search_batch_filtered(ultra, Q[:3], K, lambda s: False) == [[], [], []]


def test_protocol_search_knn_filtered_star(hnsw, ultra):
    from hnsw_clj_amd import protocol

    idx, base, Q, Qd, g, want = hnsw
    index = protocol.GpuHnswIndex(ultra)
    assert protocol.supports_filtering(index)
    pred = lambda s: int(s[1:]) % 3 == 0  # noqa: E731
    res = index.search_knn_filtered_star(Q[0], K, pred)
    assert len(res) == K and all(set(r) == {"id", "distance"} and pred(r["id"]) for r in res)
    ds = [r["distance"] for r in res]
    assert ds == sorted(ds)
