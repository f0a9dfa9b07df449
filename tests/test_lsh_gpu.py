"""Hybrid LSH on the device (hnswgpu_lsh_*) against yardsticks that do not run the code under test: the codes against the CPU
oracle's device-order dot, the buckets against a stable counting sort, the search against the numpy model of hybrid_lsh.clj
(lsh_model.py) fed with the oracle's dense device-order distances -- ids and distance bits equal -- and the distances within the
project's tolerance of the f64 order."""
import numpy as np
import pytest

import lsh_model as M
from util import assert_exact, close, metric_scale

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "l2", "dot"]
K = 10
# (num_probes, probe_radius, take_main, take_flip): the five modes (hybrid_lsh.clj:350-364: 2 k of the own bucket, k of a
# neighbour) and search-hybrid's default form (:195-259: radius 0, 3 k)
CONFIGS = [(p, r, 2 * K, K) for p, r in M.MODES.values()] + [(2, 0, 3 * K, K)]


def _om(O, metric):
    return {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]


def _dense(O, base, Q, metric, mode):
    """Every query's distance to every row, [nq][n], from one exact_knn over the whole base (-0 canonicalised as the keys do)"""
    ids, d, _ = O.exact_knn(base, Q, len(base), metric=_om(O, metric), mode=mode)
    D = np.empty((len(Q), len(base)), np.float64)
    np.put_along_axis(D, ids.astype(np.int64), d, axis=1)
    return D + 0.0


def _oracle_codes(O, X, planes):
    """bit i of table t = O.distance_dev(DOT, plane, row) <= 0: the negated GEMV-order dot with the plane in the query's role
    (orc_dist_dev directly: the two norms distance_dev computes per call play no part in a DOT distance)"""
    T, B, dim = planes.shape
    X, planes = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(planes, np.float32)
    fn, pp = O.lib().orc_dist_dev, [[O._p(planes[t, i]) for i in range(B)] for t in range(T)]
    dist = np.array([[[fn(O.DOT, pp[t][i], xp, dim, 1.0, 1.0) for i in range(B)] for t in range(T)] for xp in map(O._p, X)])
    assert dist[0, 0, 0] == O.distance_dev(O.DOT, planes[0, 0], X[0])
    return M.codes_from_dots(-dist)


def _model(D, qcodes, off, ids, bits, k, cfg):
    return M.search_batch(D, qcodes, off, ids, bits, k, *cfg)


def _check_search(idx, O, base, Q, metric, D, cfg, k=K, what=""):
    """One search against the model: ids and bits; returns (ids, distances)"""
    _, _, off, ids = idx.lsh_get()
    bits = idx.lsh_sizes()[1]
    gi, gd = idx.lsh_search(Q, k, *cfg)
    ei, ed = _model(D, idx.lsh_hash(Q), off, ids, bits, k, cfg)
    assert_exact(gi, gd, ei, ed, "%s %s %s" % (what, metric, cfg))
    return gi, gd


@pytest.mark.parametrize("dim", [7, 20, 128, 772, 1536])
def test_codes_bit_for_bit(native_lib, oracle, dim):
    from hnsw_clj_amd import engine

    O = oracle
    rng = np.random.default_rng(dim)
    n, T, B = 300, 3, 5
    base = rng.standard_normal((n, dim)).astype(np.float32)
    planes = rng.standard_normal((T, B, dim)).astype(np.float32)
    for (t, i), axis in {(0, 0): 0, (1, 2): dim - 1, (2, 4): dim // 2}.items():   # axis-aligned among the random ones
        planes[t, i] = 0
        planes[t, i, axis] = 1
    base[5, 0] = 0.0          # dot with plane (0, 0) exactly +0
    base[6, 0] = -0.0         # a -0.0 component under the same plane
    base[7, dim - 1] = -0.0
    base[8] = 0.0             # a zero row: every dot +0
    Q = rng.standard_normal((37, dim)).astype(np.float32)
    with engine.Index(base, "dot", 0) as idx:
        idx.set_lsh(planes)
        gp, codes, off, ids = idx.lsh_get()
        assert np.array_equal(gp, planes)
        want = _oracle_codes(O, base, planes)
        assert np.array_equal(codes, want)
        assert (codes[8] == (1 << B) - 1).all() and (codes[5, 0] & 1) == 1 and (codes[6, 0] & 1) == 1
        assert np.array_equal(idx.lsh_hash(base), codes)             # the same kernel: a base row lands in its own buckets
        assert np.array_equal(idx.lsh_hash(Q), _oracle_codes(O, Q, planes))
        assert np.array_equal(idx.lsh_hash(base[3]), codes[3:4])
        # buckets: the stable counting sort of the codes
        eo, ei = M.buckets(codes, B)
        assert np.array_equal(off, eo) and np.array_equal(ids, ei)
        for t in range(T):
            assert np.array_equal(np.sort(ids[t]), np.arange(n))
            for b in range(1 << B):
                seg = ids[t, off[t, b]:off[t, b + 1]]
                assert (np.diff(seg) > 0).all() and (codes[seg, t] == b).all()


@pytest.fixture(scope="module")
def data2000():
    rng = np.random.default_rng(2000)
    base = rng.standard_normal((2000, 128)).astype(np.float32)
    Q = rng.standard_normal((33, 128)).astype(np.float32)
    Q[::2] = base[rng.integers(0, 2000, 17)] + 0.05 * rng.standard_normal((17, 128)).astype(np.float32)   # near a base row
    return base, Q


@pytest.fixture(scope="module")
def codes2000(oracle, data2000):
    """The reference's hyperplanes -- Random(42), 8 tables x 64 rows x dim Gaussians, the first 12 rows of a table kept -- drawn by
    the oracle's generator, and the 12-bit codes of the rows and queries under them.  (A build with fewer bits keeps fewer rows
    of the same draws: its codes are the low bits.)"""
    O = oracle
    base, Q = data2000
    r = O.JavaRandom(42)
    planes = np.array([r.next_gaussian() for _ in range(8 * 64 * 128)]).reshape(8, 64, 128)[:, :12].astype(np.float32)
    return planes, _oracle_codes(O, base, planes), _oracle_codes(O, Q, planes)


@pytest.mark.parametrize("bits", [4, 12])
@pytest.mark.parametrize("metric", METRICS)
def test_search_matches_the_model(native_lib, oracle, data2000, codes2000, metric, bits):
    """8 x 4 bits: buckets of about 125 rows, every probe truncates.  8 x 12 bits: most buckets empty, the results padded."""
    from hnsw_clj_amd import engine

    O = oracle
    base, Q = data2000
    D = _dense(O, base, Q, metric, O.MODE_DEV)
    D64 = _dense(O, base, Q, metric, O.MODE_F64)
    scale = metric_scale(metric, Q, base)
    with engine.Index(base, metric, 0) as idx:
        idx.lsh_build(8, bits, 64, 42)
        planes, codes, off, ids = idx.lsh_get()
        want_planes, want_codes, want_qcodes = codes2000
        assert np.array_equal(planes, want_planes[:, :bits])
        mask = (1 << bits) - 1
        assert np.array_equal(codes, want_codes & mask) and np.array_equal(idx.lsh_hash(Q), want_qcodes & mask)
        eo, ei = M.buckets(codes, bits)
        assert np.array_equal(off, eo) and np.array_equal(ids, ei)
        padded = truncated = 0
        for cfg in CONFIGS:
            for nq in (1, 7, 33):
                gi, gd = _check_search(idx, O, base, Q[:nq], metric, D[:nq], cfg, what="nq %d" % nq)
                for q in range(nq):
                    c = int((gi[q] >= 0).sum())
                    assert (gi[q, c:] == -1).all() and np.isinf(gd[q, c:]).all() and len(set(gi[q, :c].tolist())) == c
                    assert close(gd[q, :c], D64[q, gi[q, :c]], scale).all()
                    padded += c < K
            sizes = np.diff(off, axis=1)
            truncated += int((sizes > cfg[2]).any())
        assert (padded > 0) == (bits == 12) and (truncated > 0) == (bits == 4)


def test_crafted_ties_duplicates_and_truncation(native_lib, oracle):
    """The hand-worked examples of lsh_model.py on the device: identical rows at two ids, rows found through two tables, the case
    where truncate-then-dedup and dedup-then-truncate differ."""
    from hnsw_clj_amd import engine

    O = oracle
    Q = M.HAND_QUERY[None, :]
    D = _dense(O, M.HAND_ROWS, Q, "l2", O.MODE_DEV)
    with engine.Index(M.HAND_ROWS, "l2", 0) as idx:
        idx.set_lsh(M.HAND_PLANES)
        _, codes, _, _ = idx.lsh_get()
        assert np.array_equal(codes, M.HAND_CODES) and np.array_equal(idx.lsh_hash(Q), [[3, 3]])
        for (k, probes, radius, take_main, take_flip), want in M.HAND_CASES:
            gi, gd = _check_search(idx, O, M.HAND_ROWS, Q, "l2", D, (probes, radius, take_main, take_flip), k=k, what="hand")
            assert gi[0, :len(want)].tolist() == want and (gi[0, len(want):] == -1).all()
        # the batch form: every query of a batch is the single query
        gi, _ = idx.lsh_search(np.repeat(Q, 5, axis=0), 4, 1, 2, 2, 1)
        assert (gi == [0, 1, 4, 5]).all()


def test_zero_rows_under_cosine(native_lib, oracle):
    from hnsw_clj_amd import engine

    O = oracle
    rng = np.random.default_rng(5)
    base = np.abs(rng.standard_normal((40, 4))).astype(np.float32)    # all in bucket 3 of both tables
    base[[3, 17, 18]] = 0.0                                          # zero rows hash to all-ones too: distance 1
    Q = np.stack([M.HAND_QUERY, np.zeros(4, np.float32), base[7]])
    D = _dense(O, base, Q, "cosine", O.MODE_DEV)
    assert (D[:, [3, 17, 18]] == 1.0).all() and (D[1] == 1.0).all()
    with engine.Index(base, "cosine", 0) as idx:
        idx.set_lsh(M.HAND_PLANES)
        for k, cfg in ((10, (2, 1, 20, 10)), (40, (2, 0, 45, 1)), (40, (1, 2, 38, 38))):
            _check_search(idx, O, base, Q, "cosine", D, cfg, k=k, what="zero rows")


@pytest.mark.parametrize("dim,RB", [(128, 8), (1536, 4), (3072, 2)])
def test_bucket_walk_edges(native_lib, oracle, dim, RB):
    """One table of 4 axis-aligned bits: bucket b holds SIZES[b] rows.  Sizes around the rows a wave walks per step (RB) and around
    both key stores' takes: 64 keys in registers, 66 in LDS."""
    from hnsw_clj_amd import engine

    O = oracle
    sizes = sorted({0, 1, RB - 1, RB, RB + 1, 63, 64, 65, 66, 67})
    assert len(sizes) <= 16
    rng = np.random.default_rng(dim)
    sign = lambda b: np.array([1.0 if (b >> i) & 1 else -1.0 for i in range(4)], np.float32)
    rows, Q = [], []
    for b, s in enumerate(sizes):
        x = rng.standard_normal((s + 1, dim)).astype(np.float32)
        x[:, :4] = np.abs(x[:, :4]) * sign(b)
        rows.append(x[:s])
        Q.append(x[s])
    base = np.concatenate(rows)
    base = base[rng.permutation(len(base))]
    Q = np.stack(Q)
    planes = np.zeros((1, 4, dim), np.float32)
    planes[0, np.arange(4), np.arange(4)] = 1
    for metric in ("cosine", "l2"):
        D = _dense(O, base, Q, metric, O.MODE_DEV)
        with engine.Index(base, metric, 0) as idx:
            idx.set_lsh(planes)
            _, codes, off, _ = idx.lsh_get()
            assert np.diff(off[0])[:len(sizes)].tolist() == sizes and np.array_equal(idx.lsh_hash(Q)[:, 0], np.arange(len(sizes)))
            for take in (64, 66, 1, RB):
                gi, _ = _check_search(idx, O, base, Q, metric, D, (1, 0, take, take), k=70, what="walk take %d" % take)
                assert [(g >= 0).sum() for g in gi] == [min(s, take) for s in sizes]
            _check_search(idx, O, base, Q, metric, D, (1, 4, 66, 64), k=256, what="walk flips")   # both stores in one launch


def test_all_rows_in_one_bucket(native_lib, oracle):
    from hnsw_clj_amd import engine

    O = oracle
    rng = np.random.default_rng(11)
    base = np.abs(rng.standard_normal((300, 64))).astype(np.float32)
    Q = np.abs(rng.standard_normal((5, 64))).astype(np.float32)
    planes = np.ones((2, 1, 64), np.float32)
    D = _dense(O, base, Q, "dot", O.MODE_DEV)
    with engine.Index(base, "dot", 0) as idx:
        idx.set_lsh(planes)
        _, _, off, _ = idx.lsh_get()
        assert off.tolist() == [[0, 0, 300]] * 2
        for cfg in ((2, 1, 64, 64), (2, 1, 66, 3), (1, 0, 256, 1), (2, 5, 20, 10)):
            _check_search(idx, O, base, Q, "dot", D, cfg, k=K, what="one bucket")
        _check_search(idx, O, base, Q, "dot", D, (2, 0, 256, 1), k=256, what="one bucket, k 256")


def test_every_base_row_finds_itself(native_lib, oracle, data2000):
    from hnsw_clj_amd import engine

    O = oracle
    base, _ = data2000
    with engine.Index(base, "cosine", 0) as idx:
        idx.lsh_build()
        gi, gd = idx.lsh_search(base, K, *M.MODES["turbo"])
        assert np.array_equal(gi[:, 0], np.arange(len(base)))
        self_d = np.array([O.distance_dev(O.COSINE, r, r) for r in base], np.float32)
        assert np.array_equal(gd[:, 0].view(np.uint32), (self_d + np.float32(0)).view(np.uint32))


def test_entry_points_and_state(native_lib, oracle, data2000):
    import torch

    from hnsw_clj_amd import engine
    from hnsw_clj_amd._native import HnswGpuError

    base, Q = data2000
    base = base[:600]
    dev = torch.device("cuda", 0)

    def code_of(fn):
        with pytest.raises(HnswGpuError) as e:
            fn()
        return e.value.code

    def bits_equal(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))

    with engine.Index(base, "cosine", 0) as idx:
        # a handle without tables
        assert idx.lsh_sizes() == (0, 0)
        assert code_of(lambda: idx.lsh_search(Q, K)) == -3 and code_of(lambda: idx.lsh_hash(Q)) == -3
        assert code_of(idx.lsh_get) == -3
        idx.hnsw_build(8, 40, 42)
        before = idx.hnsw_search(Q, K, 32)
        idx.lsh_build(8, 6, 64, 42)
        first = idx.lsh_get()
        idx.lsh_build(8, 6, 64, 42)            # replaces the tables: one seed, the same planes and codes
        assert all(np.array_equal(a, b) for a, b in zip(first, idx.lsh_get()))
        assert bits_equal(before, idx.hnsw_search(Q, K, 32))
        host = idx.lsh_search(Q, K, 6, 2)
        # the device entry on a stream of the caller's
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            di, dd = idx.lsh_search(torch.from_numpy(Q).to(dev), K, 6, 2)
        s.synchronize()
        assert bits_equal(host, (di.cpu().numpy(), dd.cpu().numpy()))
        # the tables would miss added rows
        assert code_of(lambda: idx.hnsw_add(Q[:2])) == -3 and idx.n == len(base)
        # arguments and limits
        assert code_of(lambda: idx.lsh_search(Q, 0)) == -1 and code_of(lambda: idx.lsh_search(Q, K, 6, 2, 0, 1)) == -1
        assert code_of(lambda: idx.lsh_search(Q, K, 0, 2)) == -1 and code_of(lambda: idx.lsh_search(Q, K, 6, -1)) == -1
        assert code_of(lambda: idx.lsh_search(Q, 257)) == -5 and code_of(lambda: idx.lsh_search(Q, K, 6, 2, 257, 1)) == -5
        assert code_of(lambda: idx.lsh_search(Q, K, 6, 2, 1, 257)) == -5
        assert code_of(lambda: idx.lsh_build(17, 6)) == -5 and code_of(lambda: idx.lsh_build(8, 17)) == -5
        assert code_of(lambda: idx.lsh_build(8, 0)) == -5 and code_of(lambda: idx.lsh_build(0, 6)) == -1
        assert bits_equal(host, idx.lsh_search(Q, K, 6, 2))          # a refused build left the tables alone
        assert bits_equal(idx.lsh_search(Q, K, 8, 2), idx.lsh_search(Q, K, 60, 2))   # probes clamped to the tables ...
        assert bits_equal(idx.lsh_search(Q, K, 6, 6), idx.lsh_search(Q, K, 6, 99))   # ... the radius to the bits
        gi, gd = idx.lsh_search(Q[:0], K)
        assert gi.shape == (0, K)
        # the exported planes on a fresh handle: the same buckets, the same search bits
        with engine.Index(base, "cosine", 0) as other:
            other.ivf_build(8, 3, 42)
            before = other.ivf_search(Q, K, 3)
            other.set_lsh(first[0])
            assert bits_equal(before, other.ivf_search(Q, K, 3))
            assert code_of(lambda: other.ivf_add(Q[:2])) == -3 and other.n == len(base)
            assert all(np.array_equal(a, b) for a, b in zip(first, other.lsh_get()))
            assert bits_equal(host, other.lsh_search(Q, K, 6, 2))
    with engine.Index(np.zeros((0, 16), np.float32), "l2", 0) as empty:
        empty.lsh_build()
        assert empty.lsh_sizes() == (8, 12)
        gi, gd = empty.lsh_search(np.ones((3, 16), np.float32), 4)
        assert (gi == -1).all() and np.isinf(gd).all()


def test_mirror(native_lib, data2000):
    from hnsw_clj_amd import hybrid_lsh as H
    from hnsw_clj_amd import protocol

    base, Q = data2000
    base = base[:500]
    index = H.build_index([["v%d" % i, v] for i, v in enumerate(base)], show_progress=False)
    try:
        for mode, (probes, radius) in H.MODE_CONFIGS.items():
            ids, d = index.index.lsh_search(Q[:4], K, probes, radius, 2 * K, K)
            got = H.search_knn(index, Q[:4], K, mode)
            assert [[r["id"] for r in rs] for rs in got] == [["v%d" % i for i in row if i >= 0] for row in ids]
            assert H.search_knn(index, Q[0], K, mode) == got[0]
        assert H.search_knn(index, Q[0], K) == H.search_knn(index, Q[0], K, "balanced") == H.search_batch(index, Q[:1], K, None)[0]
        ids, _ = index.index.lsh_search(Q[:2], K, 2, 0, 3 * K, K)
        assert [[r["id"] for r in rs] for rs in H.search_hybrid(index, Q[:2], K)] == [["v%d" % i for i in row if i >= 0] for row in ids]
        self_hit = H.search_knn(index, base[7], 1, "turbo")
        assert self_hit[0]["id"] == "v7"
        info = H.index_info(index)
        _, _, off, _ = index.index.lsh_get()
        assert info["vectors"] == 500 and info["hash-tables"] == 8 and info["buckets-per-table"] == 4096
        assert info["total-buckets"] == int((np.diff(off, axis=1) > 0).sum()) and info["avg-bucket-size"] == 500 / info["total-buckets"]
        p = protocol.GpuHybridLshIndex(index)
        assert p.search_knn_star(Q[0], K, "fast") == H.search_knn(index, Q[0], K, "fast")
        assert p.search_batch_star(Q[:3], K, "fast") == H.search_knn(index, Q[:3], K, "fast") and p.index_info_star() == info
    finally:
        index.close()
    empty = H.build_index([], show_progress=False)
    try:
        assert H.search_knn(empty, [1.0], 5) == [] and H.search_batch(empty, [[1.0], [2.0]], 5, "fast") == [[], []]
    finally:
        empty.close()
