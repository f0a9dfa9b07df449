"""The top-k selection and merge kernels on crafted distance streams (tests/topk_streams.py): rows v[i] * e0 make any
float32 stream the exact distance stream of a search, so every leg compares ids and float32 values with a plain stable
argsort of the stream -- no tolerance anywhere -- and, wherever it forces a schedule through hnswgpu_set_tuning, with the
result at the default as well ("keys are a total order: the result does not depend on W").

  leg A  hnswgpu_exact_knn_filtered, all-pass mask   filtered_group_kernel -> select_topk_kernel (stride p), SELECT_W
  leg B  hnswgpu_exact_knn, 1 .. 15 queries          scan_kernel's per-wave lists, merge_topk_kernel, MERGE_W, SCAN_BLOCKS
  leg C  hnswgpu_exact_knn, 16 and 33 queries        tile scan + select_topk_kernel (stride n); k = 1: tile_argmin_all;
         hnswgpu_kmeans_assign                       the fused argmin over a centroid table with duplicates
  leg D  hnswgpu_rerank                              gather_dist_kernel's keys + merge_topk_kernel, MERGE_W
  leg E  hnswgpu_merge_lists_dev / _topk_dev / _keyed_dev   merge_shards_kernel, merge_keyed_kernel
  leg F  hnswgpu_ivf_search(..., want_probes)        routing selection (topk_small_wg: histograms, bisection; above 64
                                                     probes select_topk_wg) and the finish merge
"""
import numpy as np
import pytest

import topk_streams as ts

pytestmark = pytest.mark.gpu

DIM = 4
N_EDGES = [1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2049, 4099, 8192]
K_EDGES = [1, 2, 10, 63, 64, 65, 128, 129, 256, 257, 1000, 1024]
SCALES = (1.0, 2.0, -1.0, 0.5)


@pytest.fixture(scope="module")
def eng(native_lib):
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    return engine


def _searches(fam, v, k, nq, dim=DIM):
    """The searches one stream gives: (metric, rows, queries, per-query distance streams)."""
    sc = [SCALES[i % len(SCALES)] for i in range(nq)]
    v1 = ts.fit_scale(v, 2.0)
    out = [("dot", ts.rows_of(v1, dim), np.stack([ts.unit_query(-s, dim) for s in sc]), [ts.dot_stream(v1, s) for s in sc])]
    if fam == "grid":                                    # squares exact: zero query, distance |v[i]|
        out.append(("l2", ts.rows_of(v, dim), np.zeros((nq, dim), np.float32), [np.abs(v)] * nq))
    if fam in ts.MODERATE:                               # query c * e0: 0 / 1 / 2 (c < 0: 2 / 1 / 0)
        r, cs = ts.cosine_rows(v, k)
        out.append(("cosine", ts.rows_of(r, dim), np.stack([ts.unit_query(s, dim) for s in sc]),
                    [cs if s > 0 else (2.0 - cs).astype(np.float32) for s in sc]))
    return out


class _Expect:
    """expected() of the streams of one search, computed once and shared by every schedule."""

    def __init__(self, streams, k):
        self.want = [ts.expected(s, k) for s in streams]

    def check(self, res, what):
        ids, d = res                                     # (a batch may be a prefix of the queries)
        assert 0 < len(ids) <= len(self.want)
        for qi, (wi, wd) in enumerate(self.want[:len(ids)]):
            ts.assert_same(ids[qi], d[qi], wi, wd, "%s query %d" % (what, qi))


def _same(res, ref, what):
    np.testing.assert_array_equal(res[0], ref[0], err_msg=what + ": ids differ from the default schedule's")
    assert (np.asarray(res[1]) == np.asarray(ref[1])).all(), what + ": distances differ from the default schedule's"


# ---- leg A ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ts.FAMILIES)
def test_leg_a_select_through_the_filtered_scan(eng, tune, fam):
    for name, n, k, v in ts.sample(N_EDGES, K_EDGES, 11, names=(fam,)):
        allow = eng.pack_mask(np.ones(n, np.bool_), n)
        for metric, rows, Q, streams in _searches(fam, v, k, 5):
            ex = _Expect(streams, k)
            with eng.Index(rows, metric) as idx:
                for nq in (1, 5):
                    what = "leg A %s %s n=%d k=%d nq=%d" % (name, metric, n, k, nq)
                    tune.unset("SELECT_W")
                    ref = idx.exact_knn_filtered(Q[:nq], k, allow)
                    ex.check(ref, what)
                    for w in (1, 2, 4, 16):              # W = 1: four queries share a workgroup, 5 leaves one partly filled
                        tune.set("SELECT_W", w)
                        res = idx.exact_knn_filtered(Q[:nq], k, allow)
                        ex.check(res, what + " SELECT_W=%d" % w)
                        _same(res, ref, what + " SELECT_W=%d" % w)
                    tune.unset("SELECT_W")


# ---- leg B ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ts.FAMILIES)
def test_leg_b_scan_lists_and_merge(eng, tune, fam):
    NQ = (1, 3, 15)
    grid = [(mw, sb) for mw in (None, 1, 4, 16) for sb in (None, 1, 64)]
    for name, n, k, v in ts.sample(N_EDGES, K_EDGES, 12, names=(fam,)):
        for metric, rows, Q, streams in _searches(fam, v, k, 15):
            ex = _Expect(streams, k)
            with eng.Index(rows, metric) as idx:
                refs = {}
                for nq in NQ:
                    what = "leg B %s %s n=%d k=%d nq=%d" % (name, metric, n, k, nq)
                    refs[nq] = idx.exact_knn(Q[:nq], k)
                    ex.check(refs[nq], what)
                for mw, sb in grid[1:]:                  # every (MERGE_W, SCAN_BLOCKS) schedule at every batch size
                    tune.set("MERGE_W", mw) if mw else tune.unset("MERGE_W")
                    tune.set("SCAN_BLOCKS", sb) if sb else tune.unset("SCAN_BLOCKS")
                    for nq in NQ:
                        what = "leg B %s %s n=%d k=%d nq=%d MERGE_W=%s SCAN_BLOCKS=%s" % (name, metric, n, k, nq, mw, sb)
                        res = idx.exact_knn(Q[:nq], k)
                        ex.check(res, what)
                        _same(res, refs[nq], what)
                tune.unset("MERGE_W")
                tune.unset("SCAN_BLOCKS")


# ---- leg C ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ts.FAMILIES)
def test_leg_c_tile_scan_select_and_argmin(eng, fam):
    for name, n, k, v in ts.sample(N_EDGES, K_EDGES, 13, names=(fam,)):
        for metric, rows, Q, streams in _searches(fam, v, k, 33):
            ex = _Expect(streams, k)
            with eng.Index(rows, metric) as idx:
                for nq in (16, 33):                      # k = 1: the fused argmin, the lowest of the tied rows wins
                    what = "leg C %s %s n=%d k=%d nq=%d" % (name, metric, n, k, nq)
                    ex.check(idx.exact_knn(Q[:nq], k), what)


@pytest.mark.parametrize("fam", ts.FAMILIES)
def test_leg_c_assignment_to_the_lowest_nearest_centroid(eng, fam):
    """hnswgpu_kmeans_assign with the stream as the centroid table (rows of the index are the queries): duplicated
    centroids tie, every row goes to the lowest-numbered nearest one."""
    rs = np.random.RandomState(5)
    for name, n, k, v in ts.sample(N_EDGES, K_EDGES, 14, names=(fam,)):
        v = v.copy()
        if n > 2:                                        # duplicated centroids in every family, the minimum among them
            dup = rs.randint(0, n, max(1, n // 8))
            v[dup] = v[rs.randint(0, n, len(dup))]
            v[rs.randint(0, n, 2)] = v.min()
        for metric, cen, rowsq, streams in _searches(fam, v, k, 37):
            with eng.Index(rowsq, metric) as idx:        # (the index holds the 37 "queries")
                a, d = idx.kmeans_assign(cen)
            what = "leg C assign %s %s centroids=%d" % (name, metric, n)
            want = [ts.expected(s, 1) for s in streams]
            ts.assert_same(a, d, np.array([w[0][0] for w in want]), np.array([w[1][0] for w in want]), what)


# ---- leg D ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ts.FAMILIES)
def test_leg_d_rerank(eng, tune, fam):
    M = (1, 64, 65, 2047, 2048, 2049, 5000)
    rs = np.random.RandomState(6)
    cases = [(c, M[(2 * ci + j) % len(M)]) for ci, c in enumerate(ts.sample(N_EDGES, K_EDGES, 15, names=(fam,))) for j in (0, 1)]
    for (name, n, k, v), m in cases:
        nq = 3
        cand = rs.randint(-1, n + 3, (nq, m)).astype(np.int32)      # repeats, -1, ids >= n
        cand[0, : min(m, n)] = rs.permutation(n)[: min(m, n)]      # (one query names many distinct rows)
        for metric, rows, Q, streams in _searches(fam, v, k, nq):
            what = "leg D %s %s n=%d k=%d m=%d" % (name, metric, n, k, m)
            want = [ts.expected_mapped(streams[qi], cand[qi], k) for qi in range(nq)]
            wi, wd = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
            with eng.Index(rows, metric) as idx:
                tune.unset("MERGE_W")
                ref = idx.rerank(Q, cand, k)
                ts.assert_same(ref[0], ref[1], wi, wd, what)
                for mw in (1, 4, 16):
                    tune.set("MERGE_W", mw)
                    res = idx.rerank(Q, cand, k)
                    ts.assert_same(res[0], res[1], wi, wd, what + " MERGE_W=%d" % mw)
                    _same(res, ref, what + " MERGE_W=%d" % mw)
                tune.unset("MERGE_W")


# ---- leg E ------------------------------------------------------------------------------------------------------------
def _variant_cycle():
    names = [nm for base in ts.FAMILIES for nm in ts.variants(base)]
    i = 0
    while True:
        yield names[i % len(names)]
        i += 1


def _k_outs(k_in, nvalid_max):
    """1, k_in, below k_in, above k_in (up to 1024), above the number of valid entries."""
    ks = {1, k_in, max(1, k_in // 2), min(1024, k_in + 7), min(1024, 2 * k_in + 1), 1024, min(1024, nvalid_max + 5)}
    return sorted(ks)


@pytest.mark.parametrize("nshard", [1, 2, 7, 64])
def test_leg_e_merge_entry_points(eng, nshard):
    import torch

    rs = np.random.RandomState(70 + nshard)
    names = _variant_cycle()
    for _ in range(nshard % 5):
        next(names)
    for k_in in (1, 10, 64, 65, 300, 1024):
        for nq in (1, 37):
            name = next(names)
            v = None
            while v is None:                             # (a variant that does not fit this size: the next one)
                v = ts.make(name, 2048, max(1, min(1024, nshard * k_in // 2)), rs)
                name = name if v is not None else next(names)
            what = "leg E %s nshard=%d k_in=%d nq=%d" % (name, nshard, k_in, nq)
            ids = np.empty((nshard, nq, k_in), np.int32)
            dist = np.empty((nshard, nq, k_in), np.float32)
            order = np.empty((nshard, nq, k_in), np.uint32)
            for q in range(nq):
                qi, qd = ts.merge_case(v, nshard, k_in, rs)
                ids[:, q], dist[:, q] = qi, qd
                tot = nshard * k_in                                      # unique words over the 32-bit range, neither 0 nor 0xfffffffe
                o = ((rs.permutation(2 * tot)[:tot].astype(np.uint64) + 1) * (0xfffffffd // (2 * tot + 1))).astype(np.uint32)
                o[rs.randint(0, len(o))] = 0                             # the smallest and the largest order word
                o[rs.randint(1, len(o)) if len(o) > 1 else 0] = 0xfffffffe if len(o) > 1 else 0
                order[:, q] = o.reshape(nshard, k_in)
            if nq == 37:
                ids[:, 5] = -1                                           # a query with nothing at all
            t_ids, t_dist = torch.from_numpy(ids).cuda(), torch.from_numpy(dist).cuda()
            t_order = torch.from_numpy(order.view(np.int32)).cuda()
            nvalid = int((ids >= 0).sum(axis=(0, 2)).max())
            full = [ts.expected_merge(ids[:, q], dist[:, q], 1024) for q in range(nq)]
            fi, fd = np.stack([f[0] for f in full]), np.stack([f[1] for f in full])
            for k_out in _k_outs(k_in, nvalid):
                oi, od = eng.merge_lists_dev(t_ids, t_dist, k_out)
                ts.assert_same(oi.cpu().numpy(), od.cpu().numpy(), fi[:, :k_out], fd[:, :k_out], what + " lists k_out=%d" % k_out)
            oi, od = eng.merge_topk_dev(t_ids, t_dist)
            ts.assert_same(oi.cpu().numpy(), od.cpu().numpy(), fi[:, :k_in], fd[:, :k_in], what + " topk")
            keyed = [ts.expected_merge(ids[:, q], dist[:, q], k_in, order=order[:, q]) for q in range(nq)]
            oi, od = eng.merge_keyed_dev(t_ids, t_dist, t_order)
            ts.assert_same(oi.cpu().numpy(), od.cpu().numpy(), np.stack([f[0] for f in keyed]), np.stack([f[1] for f in keyed]),
                           what + " keyed")


# ---- leg F ------------------------------------------------------------------------------------------------------------
NLIST = [2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1500]
NPROBE = [1, 2, 32, 63, 64, 65, 200]
IVF_FAMILIES = tuple(f for f in ts.FAMILIES if f != "straddle")
IVF_NQ = (1, 12, 13, 40)
IVF_SCALES = (0.5, 1.0, 2.0)
# (name, value) or None = the default, each compared with the default
IVF_TUNINGS = [("QUERY_WAVES", 1), ("STREAM_ROUTE", 1), ("STREAM_ROUTE", 64), ("FINISH_BISECT", 1), ("FINISH_BISECT", 1000),
               ("FINISH_DIRECT", 0)]
# the handles: (dim, IVF_CODES): dim 128 on the survivor stream and its finish kernel, the same on the scan kernel and its
# fused tail, dim 8 without int8 rows
IVF_HANDLES = [(128, None), (128, 0), (8, None)]


def _ivf_pairs(fi):
    pairs = []
    for i, nl in enumerate(NLIST):
        fit = [p for p in NPROBE if p <= nl]
        pairs.append((nl, fit[(fi + i) % len(fit)]))
    for i, p in enumerate(NPROBE):
        fit = [nl for nl in NLIST if nl >= p]
        pairs.append((fit[(fi + 2 * i + 1) % len(fit)], p))
    return pairs


def _ivf_cases(fam):
    rs = np.random.RandomState(16)
    fi = ts.FAMILIES.index(fam)
    var = ts.variants(fam)
    for j, (nl, p) in enumerate(_ivf_pairs(fi)):
        got = 0
        for m in range(len(var)):
            name = var[(2 * j + m) % len(var)]
            v = ts.make(name, nl, p, rs)
            if v is not None:
                yield name, nl, p, v
                got += 1
                if got == min(2, len(var)):
                    break
    if fam == "plateau":                                 # the larger groups must straddle the nprobe boundary: each size, each placement
        spots = [(1024, 32), (1025, 64), (1500, 65), (1023, 200), (257, 2), (1024, 63)]
        for ti, t in enumerate((33, 256, 257, 400)):
            for wi, w in enumerate(("first", "inside", "last")):
                nl, p = spots[(ti * 3 + wi) % len(spots)]
                v = ts.make("plateau_%d_%s" % (t, w), nl, p, rs)
                if v is not None:
                    yield "plateau_%d_%s" % (t, w), nl, p, v


def _ivf_queries(nq, dim):
    sc = [IVF_SCALES[i % 3] for i in range(nq)]
    sc[nq // 2] = -1.0                                   # one +e0: the reversed stream
    return sc, np.stack([ts.unit_query(-s, dim) for s in sc])


@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("fam", IVF_FAMILIES)
def test_leg_f_ivf_routing_and_finish(eng, tune, fam, metric):
    """Centroid i = row i = v[i] * e0, list i = {row i}: the reported probes are the selection over the stream, and with
    k = nprobe the result is the same list in the same order (the stream position of a candidate is its probe's rank, so
    the routing and the finish break ties alike)."""
    for name, nlist, nprobe, v in _ivf_cases(fam):
        off, lids = np.arange(nlist + 1, dtype=np.int64), np.arange(nlist, dtype=np.int32)
        if metric == "cosine":
            r, cs = ts.cosine_rows(v, nprobe)
        for dim, codes in IVF_HANDLES:
            tune.set("IVF_CODES", codes) if codes is not None else tune.unset("IVF_CODES")
            sc, Q = _ivf_queries(max(IVF_NQ), dim)
            if metric == "cosine":                       # the rows negated: the queries -s * e0 (s > 0) see the stream cs
                rows = ts.rows_of(-r, dim)
                streams = [cs if s > 0 else (2.0 - cs).astype(np.float32) for s in sc]
            else:
                rows = ts.rows_of(v, dim)
                streams = [ts.dot_stream(v, s) for s in sc]
            want = [ts.expected(s, nprobe) for s in streams]
            wi, wd = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])

            def check(res, nq, what):
                ids, d, pr = res
                np.testing.assert_array_equal(pr[:, :nprobe], wi[:nq], err_msg=what + ": probes")
                ts.assert_same(ids, d, wi[:nq], wd[:nq], what)

            with eng.Index(rows, metric) as idx:
                idx.set_rejection_test(2)
                idx.set_ivf(rows, off, lids)
                refs = {}
                for nq in IVF_NQ:                        # 12 / 13: the one-launch routing and the routing tail
                    what = "leg F %s %s nlist=%d nprobe=%d dim=%d codes=%s nq=%d" % (name, metric, nlist, nprobe, dim, codes, nq)
                    refs[nq] = idx.ivf_search(Q[:nq], nprobe, nprobe, want_probes=True)
                    check(refs[nq], nq, what)
                for key, val in IVF_TUNINGS:
                    tune.set(key, val)
                    for nq in IVF_NQ:
                        what = "leg F %s %s nlist=%d nprobe=%d dim=%d codes=%s nq=%d %s=%d" % (
                            name, metric, nlist, nprobe, dim, codes, nq, key, val)
                        res = idx.ivf_search(Q[:nq], nprobe, nprobe, want_probes=True)
                        check(res, nq, what)
                        _same(res[:2], refs[nq][:2], what)
                        np.testing.assert_array_equal(res[2], refs[nq][2], err_msg=what + ": probes differ from the default's")
                    tune.unset(key)
        tune.unset("IVF_CODES")
