"""GPU parity tests: the HIP path (through the C ABI of libhnswgpu.so) against the CPU oracle.

Two bars, both from BASELINE.json's north_star:
  * vs the oracle's f64 reference-order mode: identical top-k id sets (modulo ties inside the
    tolerance at the k-th boundary), distances within 1e-4 relative (+1e-6 absolute)  -> util.assert_topk_parity
  * vs the oracle's device-order f32 mode (a bit-mimic of the kernels' summation order): ids
    IDENTICAL, distances BIT-identical, traversal counters (distance evaluations, expansions) equal
    -> util.assert_exact.  This is the bit-exact bar for the index/integer side of the path.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import index_file  # noqa: E402
from util import assert_exact, assert_topk_parity, close, metric_scale  # noqa: E402

pytestmark = pytest.mark.gpu

METRIC_NAMES = {0: "cos", 1: "l2", 2: "dot"}


@pytest.fixture(scope="module")
def eng(native_lib):
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    return engine


def _ivf_mode(O, metric, dim, nq, nprobe, nlist):
    """Which arithmetic serves an IVF search (ivf.hip: ivf_search_enqueue, kTilePairs): the MFMA tile path once the batch
    has more than 12 (query, list) pairs per list (cosine / dot), else the GEMV order (one GEMV per pair, the register-row
    group kernel or the int8 bounds pass + f32 refine: the same bits)."""
    tiled = metric != O.L2 and dim <= 3072 and nq * min(nprobe, nlist) > 12 * nlist
    return O.MODE_MFMA if tiled else O.MODE_DEV


def _data(oracle, n, dim, dist="gaussian", seed=42, **kw):
    return oracle.generate_dataset(n, dim, dist, seed=seed, **kw).astype(np.float32)


# ---- the :distance-fn seam, on the reference's own known answers ------------------------------------
def test_pair_distance_reference_kats(eng):
    # test/hnsw/core_test.clj:9-31, test/simple_test.clj:33-41, test/hnsw/graph_test.clj:11-22
    assert eng.pair_distance("l2", [1, 2, 3], [1, 2, 3]) == 0.0
    assert eng.pair_distance("l2", [0, 0], [3, 4]) == 5.0
    assert abs(eng.pair_distance("l2", [1, 2, 3], [4, 5, 6]) - 5.196152422706632) < 1e-5
    assert 1.73 < eng.pair_distance("l2", [1, 2, 3], [2, 3, 4]) < 1.74
    assert eng.pair_distance("cosine", [1, 2, 3], [1, 2, 3]) < 1e-3
    assert abs(eng.pair_distance("cosine", [1, 0], [-1, 0]) - 2.0) < 1e-3
    assert abs(eng.pair_distance("cosine", [1, 0], [0, 1]) - 1.0) < 1e-3
    assert abs(eng.pair_distance("cosine", [1, 2, 3], [4, 5, 6]) - 0.025368153802923787) < 1e-6
    assert eng.pair_distance("cosine", [0, 0, 0], [1, 2, 3]) == 1.0      # zero-norm guard, ultra_fast.clj:92-95
    assert eng.pair_distance("dot", [1, 2, 3], [4, 5, 6]) == -32.0


@pytest.mark.parametrize("dim", [1, 2, 3, 5, 64, 100, 128, 257, 768, 1000, 1536, 3072])
def test_batch_distances_and_norms(eng, oracle, dim):
    O = oracle
    n = 70
    base = _data(O, n, dim)
    q = _data(O, 1, dim, seed=43)[0]
    for metric in (O.COSINE, O.L2, O.DOT):
        with eng.Index(base, metric) as idx:
            d = idx.batch_distances(q)
            want_dev = np.array([O.distance_dev(metric, q, base[i]) for i in range(n)], np.float32)
            np.testing.assert_array_equal(d.view(np.uint32), want_dev.view(np.uint32))
            want64 = np.array([O.distance(metric, q, base[i]) for i in range(n)])
            assert close(d, want64, metric_scale(metric, q, base)).all()
            ids = np.array([5, 0, 69, 5, 33], np.int32)                 # gather, with a repeat
            np.testing.assert_array_equal(idx.batch_distances(q, ids), d[ids])
            bad = idx.batch_distances(q, np.array([3, n, -1], np.int32))  # out-of-range ids -> NaN, no fault
            assert bad[0] == d[3] and np.isnan(bad[1]) and np.isnan(bad[2])
            if metric == O.COSINE:
                np.testing.assert_array_equal(idx.norms().view(np.uint32), O.norms(base, O.MODE_DEV).view(np.uint32))
                assert np.allclose(idx.norms(), np.linalg.norm(base.astype(np.float64), axis=1), rtol=1e-6)


@pytest.mark.parametrize("dim", [5, 100, 768, 1536, 3072])
def test_device_f32_inside_the_spread_of_the_reference_f32_forms(eng, oracle, dim):
    """the reference's own float32 kernels (simd.clj:18-115, chunked with SPECIES_PREFERRED = 4 / 8 / 16 lanes;
    wip/vector.clj:21-86, lane accumulators) differ among themselves in the last bits.  The device's f32 result must lie
    within north_star's 1e-4 of EVERY one of them (and they of the f64 form): the device is one more f32 summation order."""
    O = oracle
    rng = np.random.default_rng(dim)
    base = rng.standard_normal((12, dim)).astype(np.float32)
    base[3] = 0.75 * base[0] + 0.01 * base[3]                          # near-duplicate direction: small cosine distance
    q = (base[0] + 0.05 * rng.standard_normal(dim)).astype(np.float32)
    for metric in (O.COSINE, O.L2, O.DOT):
        with eng.Index(base, metric) as idx:
            d = idx.batch_distances(q)
        scale = metric_scale(metric, q, base)
        for r in range(len(base)):
            forms = [f(metric, q, base[r], L, s) for f in (O.f32_vector, O.f32_lane_accumulate) for L in (4, 8, 16) for s in (0, 1)]
            if metric == O.DOT:
                forms = [-v for v in forms]                              # the engine's DOT is the ordering key -dot
            f64 = O.distance(metric, q, base[r])
            assert close(forms, f64, scale).all()
            assert close(np.full(len(forms), d[r]), forms, scale).all(), (metric, r, d[r], forms)
            spread = max(forms) - min(forms)
            assert min(forms) - 4 * spread - 1e-6 * scale <= d[r] <= max(forms) + 4 * spread + 1e-6 * scale


def test_dim_limit_and_bad_args(eng):
    with pytest.raises(Exception, match="3072"):
        eng.Index(np.zeros((2, 3073), np.float32))
    with eng.Index(np.ones((4, 8), np.float32)) as idx:
        with pytest.raises(ValueError):
            idx.batch_distances(np.ones(7, np.float32))
        with pytest.raises(Exception, match="no graph"):
            idx.hnsw_search(np.ones(8, np.float32), 2)
        with pytest.raises(Exception, match="no IVF"):
            idx.ivf_search(np.ones(8, np.float32), 2, 1)
        with pytest.raises(Exception, match="k must be"):
            idx.exact_knn(np.ones(8, np.float32), 0)


# ---- exact kNN (bench.clj:72-84) ------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,k", [(1, 4, 3), (33, 7, 5), (1000, 128, 10), (5000, 96, 64), (300, 768, 100)])
def test_exact_knn(eng, oracle, n, dim, k):
    O = oracle
    base = _data(O, n, dim)
    Q = np.vstack([_data(O, 9, dim, seed=43), base[:3]])
    for metric in (O.COSINE, O.L2, O.DOT):
        with eng.Index(base, metric) as idx:
            ids, d = idx.exact_knn(Q, k)
        oi, od, _ = O.exact_knn(base, Q, k, metric=metric, mode=O.MODE_DEV)
        assert_exact(ids, d, oi, od, "exact dev n=%d" % n)
        fi, fd, _ = O.exact_knn(base, Q, k, metric=metric)
        assert_topk_parity(ids, d, fi, fd, "exact f64 n=%d" % n, metric_scale(metric, Q, base))
        if k > n:
            assert (ids[:, n:] == -1).all() and np.isinf(d[:, n:]).all()


@pytest.mark.parametrize("n,dim,nq,k", [(1000, 128, 70, 10), (300, 768, 33, 100), (2500, 100, 64, 5), (129, 8, 16, 3),
                                       (260, 1536, 21, 5), (140, 3072, 17, 3), (200, 900, 40, 4)])
def test_tiled_mfma_path_exact(eng, oracle, n, dim, nq, k):
    """Many queries against the same rows run on the MFMA tile kernel (v_mfma_f32_32x32x2_f32); its k-order is
    mimicked by the oracle's MFMA mode: ids identical, distances bit-identical.  L2 stays on the GEMV kernel."""
    O = oracle
    base = _data(O, n, dim)
    Q = np.vstack([_data(O, nq - 2, dim, seed=43), base[:2]])
    for metric in (O.COSINE, O.DOT, O.L2):
        with eng.Index(base, metric) as idx:
            ids, d = idx.exact_knn(Q, k)
            mode = O.MODE_DEV if metric == O.L2 else O.MODE_MFMA
            oi, od, _ = O.exact_knn(base, Q, k, metric=metric, mode=mode)
            assert_exact(ids, d, oi, od, "tile exact n=%d metric=%d" % (n, metric))
            fi, fd, _ = O.exact_knn(base, Q, k, metric=metric)
            assert_topk_parity(ids, d, fi, fd, "tile f64", metric_scale(metric, Q, base))
            if metric != O.L2:  # k-means assignment = every base row against the centroid table, k = 1
                cen = _data(O, 37, dim, seed=5)
                a, ad = idx.kmeans_assign(cen)
                oa, oad = O.kmeans_assign_f32(base, cen, metric, O.MODE_MFMA)
                np.testing.assert_array_equal(a, oa)
                np.testing.assert_array_equal(ad.view(np.uint32), oad.view(np.uint32))


# ---- HNSW search on FIXED graphs (the committed golden adjacency) -----------------------------------------
@pytest.mark.parametrize("name", ["g256x64", "c1000x128"])
def test_hnsw_search_golden(eng, oracle, name):
    import make_golden

    O = oracle
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    base, Q = make_golden.inputs(name)
    for metric, m in METRIC_NAMES.items():
        g = O.Graph(gold[m + "_levels"], gold[m + "_l0"].astype(np.int32), gold[m + "_up_off"],
                    gold[m + "_up"].astype(np.int32), 8, int(gold[m + "_entry"]), int(gold[m + "_maxl"]))
        with eng.Index(base, metric) as idx:
            idx.set_graph(g)
            ids, d, st = idx.hnsw_search(Q, 10, 50, want_stats=True)
            # golden = f64 reference-order results
            assert_topk_parity(ids, d, gold[m + "_hnsw_ids"], gold[m + "_hnsw_d"], name + " " + m,
                               metric_scale(metric, Q, base))
            # device-order oracle: everything identical, including the traversal itself
            oi, od, ost, _ = O.hnsw_search(base, g, Q, 10, ef=50, metric=metric, mode=O.MODE_DEV)
            assert_exact(ids, d, oi, od, name + " " + m)
            np.testing.assert_array_equal(st, ost, err_msg="distance evaluations / expansions differ")
            # export == import
            g2 = idx.get_graph()
            assert np.array_equal(g2.l0_adj, g.l0_adj) and np.array_equal(g2.up_adj, g.up_adj) and g2.entry == g.entry


@pytest.mark.parametrize("ef,k", [(1, 1), (10, 10), (50, 10), (200, 10), (333, 100), (1024, 10)])
def test_hnsw_search_ef_sweep(eng, oracle, ef, k):
    O = oracle
    base = _data(O, 3000, 64, "clustered", num_clusters=20, noise_level=0.5)
    Q = _data(O, 12, 64, "clustered", num_clusters=20, noise_level=0.5, seed=43)
    g = O.hnsw_build(base, O.COSINE, M=16, ef_construction=100, mode=O.MODE_FAST)
    with eng.Index(base, "cosine") as idx:
        idx.set_graph(g)
        ids, d, st = idx.hnsw_search(Q, k, ef, want_stats=True)
    oi, od, ost, _ = O.hnsw_search(base, g, Q, k, ef=ef, mode=O.MODE_DEV)
    assert_exact(ids, d, oi, od, "ef=%d" % ef)
    np.testing.assert_array_equal(st, ost)
    fi, fd, _, _ = O.hnsw_search(base, g, Q, k, ef=ef)
    assert_topk_parity(ids, d, fi, fd, "ef=%d f64" % ef)


def test_hnsw_collisions_and_zero_vectors(eng, oracle):
    """Duplicate rows give exact distance ties (the evicted-but-tied 'ghost' rule of the traversal),
    zero rows hit the cosine guard."""
    O = oracle
    rs = np.random.RandomState(7)
    uniq = rs.randn(40, 16).astype(np.float32)
    base = uniq[rs.randint(0, 40, 600)]            # every row has ~15 exact duplicates
    base[::50] = 0.0
    Q = np.vstack([uniq[:6], np.zeros((1, 16), np.float32), rs.randn(5, 16).astype(np.float32)])
    for metric in (O.COSINE, O.L2):
        g = O.hnsw_build(base, metric, M=6, ef_construction=40, mode=O.MODE_DEV)
        with eng.Index(base, metric) as idx:
            idx.set_graph(g)
            for ef in (1, 5, 20, 64):
                ids, d, st = idx.hnsw_search(Q, 5, ef, want_stats=True)
                oi, od, ost, _ = O.hnsw_search(base, g, Q, 5, ef=ef, metric=metric, mode=O.MODE_DEV)
                assert_exact(ids, d, oi, od, "dups ef=%d metric=%d" % (ef, metric))
                np.testing.assert_array_equal(st, ost)


def test_hnsw_edge_cases(eng, oracle):
    O = oracle
    # empty index -> [] (ultra_fast.clj:349-351, core_test.clj:63-68)
    with eng.Index(np.zeros((0, 3), np.float32)) as idx:
        idx.hnsw_build()
        ids, d = idx.hnsw_search([1, 2, 3], 5)
        assert (ids == -1).all() and np.isinf(d).all()
    # single vector (core_test.clj:70-78)
    one = np.array([[1.0, 2.0, 3.0, 4.0]], np.float32)
    with eng.Index(one) as idx:
        idx.hnsw_build()
        ids, d = idx.hnsw_search(one[0], 1)
        assert ids[0, 0] == 0 and d[0, 0] < 1e-3
    # k > n (core_test.clj:90-96)
    five = _data(O, 5, 64)
    with eng.Index(five) as idx:
        idx.hnsw_build()
        ids, d = idx.hnsw_search(five[0], 10)
        assert (ids[0] >= 0).sum() == 5 and sorted(ids[0][:5].tolist()) == [0, 1, 2, 3, 4]
    # malformed graphs are rejected, not run
    with eng.Index(five) as idx:
        g = O.hnsw_build(five)
        bad = O.Graph(g.levels, g.l0_adj.copy(), g.up_off, g.up_adj, g.M, g.entry, g.max_level)
        bad.l0_adj[0, 0] = 99
        with pytest.raises(Exception, match="out of range"):
            idx.set_graph(bad)


def test_hnsw_build_on_device(eng, oracle):
    """hnswgpu_hnsw_build: a valid graph (re-importable), reference level distribution, and recall
    comparable to the oracle's sequential reference-structure build."""
    O = oracle
    base = _data(O, 4000, 64)
    Q = _data(O, 64, 64, seed=43)
    ex, _, _ = O.exact_knn(base, Q, 10, mode=O.MODE_FAST)
    with eng.Index(base) as idx:
        idx.hnsw_build(16, 200, 42)
        g = idx.get_graph()
        # levels follow floor(-ln U / ln 2) of java.util.Random(42) (ultra_fast.clj:133,143-147)
        r = O.JavaRandom(42)
        want = [min(int((1.0 / np.log(2.0)) * -np.log(r.next_double())), 30) for _ in range(4000)]
        assert g.levels.tolist() == want
        assert g.levels[g.entry] == g.max_level == max(want)
        deg = (g.l0_adj >= 0).sum(1)
        assert deg.min() >= 1 and deg.max() <= 32
        idx.set_graph(g)  # passes the validator
        ids, d = idx.hnsw_search(Q, 10, 100)
        rec_gpu_graph = O.recall(ids, ex)
        # same graph searched by the oracle gives the same answer
        oi, od, _, _ = O.hnsw_search(base, g, Q, 10, ef=100, mode=O.MODE_DEV)
        assert_exact(ids, d, oi, od, "gpu-built graph")
    g_ref = O.hnsw_build(base, O.COSINE, 16, 200, 42, mode=O.MODE_FAST)
    ri, _, _, _ = O.hnsw_search(base, g_ref, Q, 10, ef=100, mode=O.MODE_FAST)
    rec_ref = O.recall(ri, ex)
    assert rec_gpu_graph >= 0.9 and rec_gpu_graph >= rec_ref - 0.03, (rec_gpu_graph, rec_ref)


def _same_graph(g, og, what):
    """Edge for edge: levels, entry point, every adjacency row in its order."""
    np.testing.assert_array_equal(g.levels, og.levels, err_msg=what + ": levels")
    assert (g.entry, g.max_level, g.M, g.M0) == (og.entry, og.max_level, og.M, og.M0), what
    np.testing.assert_array_equal(g.up_off, og.up_off, err_msg=what + ": up_off")
    bad = np.nonzero((g.l0_adj.reshape(og.l0_adj.shape) != og.l0_adj).any(axis=1))[0]
    assert bad.size == 0, "%s: layer-0 rows differ at nodes %s: device %s oracle %s" % (
        what, bad[:5], g.l0_adj.reshape(og.l0_adj.shape)[bad[0]], og.l0_adj[bad[0]])
    np.testing.assert_array_equal(g.up_adj.ravel(), og.up_adj.ravel(), err_msg=what + ": upper layers")


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_hnsw_build_equals_oracle_graph(eng, oracle, metric):
    """HNSWGPU_BUILD_SEQUENTIAL is insert-single itself (ultra_fast.clj:216-275): one row at a time, the walk starting at
    min(level, entry-level) with the entry point (:247-248), ef 1 above layer 0 (:250-251), links to the m closest, an
    over-full neighbour list pruned at > m by a stable sort on the distance (:264-266, 279-299).  The exported adjacency
    must equal the CPU restatement's (oracle.c: orc_hnsw_build_ex, device-order arithmetic) EDGE FOR EDGE -- with
    duplicated rows (exact ties in every list they meet), a zero row, and clustered rows."""
    O = oracle
    code = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    base = _data(O, 3000, 48, "clustered", num_clusters=12, noise_level=0.4, seed=7)
    base[100:140] = base[60:100]          # 40 duplicated rows: exact distance ties
    base[500] = base[499]
    base[777] = 0.0
    with eng.Index(base, metric) as idx:
        idx.hnsw_build(8, 40, 42, sequential=True)
        g = idx.get_graph()
        og = O.hnsw_build_ex(base, code, 8, 40, 42, 0, mode=O.MODE_DEV)
        _same_graph(g, og, "sequential closest-m build, %s" % metric)
        Q = _data(O, 16, 48, seed=43)
        ids, d, st = idx.hnsw_search(Q, 10, 60, want_stats=True)
        oi, od, ost, _ = O.hnsw_search(base, og, Q, 10, ef=60, metric=code, mode=O.MODE_DEV)
        assert_exact(ids, d, oi, od, "search on the sequentially built graph")
        np.testing.assert_array_equal(st, ost)


@pytest.mark.parametrize("flags", ["heuristic", "heuristic+symmetric", "heuristic+extend"])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_hnsw_heuristic_build_equals_oracle_graph(eng, oracle, metric, flags):
    """The neighbour selection of src/hnsw/graph.clj on the device: get-neighbors-heuristic (:162-198) for the new node's
    links and for an over-full list (prune-connections :208-232), a dropped edge removed from both lists with SYMMETRIC
    (:226-231), extend-candidates? with EXTEND (:191-195).  In the sequential order the graph must equal the oracle's
    restatement edge for edge; the pair distances come from heuristic_select_kernel."""
    O = oracle
    code = {"cosine": O.COSINE, "l2": O.L2}[metric]
    sym, ext = "symmetric" in flags, "extend" in flags
    base = _data(O, 2500, 40, "clustered", num_clusters=10, noise_level=0.4, seed=17)
    base[200:220] = base[100:120]         # duplicated rows: ties inside the (distance, id) order of the heuristic
    with eng.Index(base, metric) as idx:
        idx.hnsw_build(6, 48, 42, sequential=True, heuristic=True, symmetric=sym, extend=ext)
        g = idx.get_graph()
        of = O.BUILD_HEURISTIC | (O.BUILD_SYMMETRIC if sym else 0) | (O.BUILD_EXTEND if ext else 0)
        og, cnt = O.hnsw_build_ex(base, code, 6, 48, 42, of, mode=O.MODE_DEV, want_counters=True)
        assert cnt[3] > 100, "the data set must overflow lists: %s" % cnt
        _same_graph(g, og, "sequential %s build, %s" % (flags, metric))


def test_hnsw_heuristic_build_connects_clusters(eng, oracle):
    """What the heuristic is for (missing 1): on well-separated clusters closest-m pruning
    (ultra_fast.clj:279-299) leaves the clusters disconnected -- recall@10 stays near 0 at any ef --, the diversity
    heuristic keeps links between them.  Batched device build, 20k x 96 clustered-normalised rows, held-out queries of
    other clusters' directions (the survey's seed-43 recipe); search parity against the oracle on the exported graph."""
    O = oracle
    base = _data(O, 20000, 96, "clustered", num_clusters=160, noise_level=0.3, seed=42)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    Q = _data(O, 200, 96, "clustered", num_clusters=160, noise_level=0.3, seed=43)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    with eng.Index(base) as idx:
        ex, _ = idx.exact_knn(Q, 10)
        rec = {}
        for name, kw in (("closest", {}), ("heuristic", dict(heuristic=True)), ("heuristic+symmetric", dict(heuristic=True, symmetric=True))):
            idx.hnsw_build(16, 200, 42, **kw)
            g = idx.get_graph()
            deg = (g.l0_adj.reshape(len(base), -1) >= 0).sum(1)
            assert deg.min() >= 1 and deg.max() <= 32
            idx.set_graph(g)                # passes the validator
            ids, d, st = idx.hnsw_search(Q, 10, 400, want_stats=True)
            rec[name] = O.recall(ids, ex)
            oi, od, ost, _ = O.hnsw_search(base, g, Q[:32], 10, ef=400, mode=O.MODE_DEV)
            assert_exact(ids[:32], d[:32], oi, od, "search on the %s graph" % name)
            np.testing.assert_array_equal(st[:32], ost)
        assert rec["closest"] < 0.3 and rec["heuristic"] > 0.9 and rec["heuristic+symmetric"] > 0.9, rec


@pytest.mark.parametrize("dim", [384, 768, 1536, 3072])
def test_hnsw_embedding_dims(eng, oracle, dim):
    """The dimensions the reference's integration test walks (test/hnsw/integration_test.clj:91-118): four row-length
    instantiations (2, 3, 6 and 12 float4 chunks per lane) of the kernel a small launch takes in this suite, the several-CU one
    (every traversal kernel at every width: test_hnsw_search_widths_gpu.py), build on the device + search, against the
    oracle on the same graph; results ascending (:134-136), recall against exact kNN >= 0.8 (:138-157)."""
    O = oracle
    # rows on a 12-dimensional manifold (like sentence embeddings; on well-separated clusters the reference's
    # closest-m pruning leaves the graph disconnected and recall says nothing about the kernel: DESIGN.md section 6)
    rs = np.random.RandomState(4)
    w = rs.randn(12, dim)
    base = (rs.randn(1200, 12) @ w / np.sqrt(12) + 0.1 * rs.randn(1200, dim)).astype(np.float32)
    Q = (rs.randn(20, 12) @ w / np.sqrt(12) + 0.1 * rs.randn(20, dim)).astype(np.float32)
    for metric in (O.COSINE, O.L2):
        with eng.Index(base, metric) as idx:
            idx.hnsw_build(8, 60, 42)
            g = idx.get_graph()
            ids, d, st = idx.hnsw_search(Q, 10, 80, want_stats=True)
            oi, od, ost, _ = O.hnsw_search(base, g, Q, 10, ef=80, metric=metric, mode=O.MODE_DEV)
            assert_exact(ids, d, oi, od, "dim=%d metric=%d" % (dim, metric))
            np.testing.assert_array_equal(st, ost)
            assert (np.diff(d, axis=1) >= 0).all()
            ex, _ = idx.exact_knn(Q, 10)
            assert O.recall(ids, ex) >= 0.8


def test_hnsw_build_small_and_degenerate(eng, oracle):
    """Device build on tiny and degenerate inputs (1 .. 3 rows, all rows equal, M = 1 and M = 32, every metric; more
    shapes with HNSWGPU_SOAK): the graph passes the import validator, and searching it on the device equals the
    oracle's search of the same graph -- ids, distances, counters."""
    O = oracle
    rs = np.random.RandomState(31)
    cases = [(1, 8, 4, O.COSINE), (2, 8, 1, O.L2), (3, 5, 2, O.DOT), (40, 16, 32, O.COSINE), (300, 24, 1, O.L2)]
    for _ in range(int(os.environ.get("HNSWGPU_SOAK", "0"))):
        cases.append((int(rs.choice([5, 33, 400, 2500])), int(rs.choice([1, 7, 64, 300])), int(rs.choice([1, 2, 8, 16, 32])),
                      int(rs.choice([O.COSINE, O.L2, O.DOT]))))
    for ci, (n, dim, M, metric) in enumerate(cases):
        base = _data(O, n, dim, "clustered", num_clusters=3, noise_level=0.4, seed=200 + ci)
        if ci % 2 == 1:
            base[: max(1, n // 3)] = base[0]                    # a third of the rows identical
        Q = np.vstack([base[:1], _data(O, 4, dim, seed=43)]).astype(np.float32)
        tag = "case %d n=%d dim=%d M=%d metric=%d" % (ci, n, dim, M, metric)
        with eng.Index(base, metric) as idx:
            idx.hnsw_build(M, 30, 5)
            g = idx.get_graph()
            assert g.levels[g.entry] == g.max_level, tag
            assert ((g.l0_adj >= -1) & (g.l0_adj < n)).all(), tag
            idx.set_graph(g)                                    # the validator accepts what the build produced
            for ef, k in [(1, 1), (20, 5)]:
                ids, d, st = idx.hnsw_search(Q, k, ef, want_stats=True)
                oi, od, ost, _ = O.hnsw_search(base, g, Q, k, ef=max(ef, k), metric=metric, mode=O.MODE_DEV)
                assert_exact(ids, d, oi, od, tag + " ef=%d" % ef)
                np.testing.assert_array_equal(st, ost, err_msg=tag)


def test_hnsw_build_linker_threads_do_not_change_the_graph(eng, oracle, tune):
    """The host linker applies a batch's edges with several threads (own lists by node range, reverse edges by
    target node mod T): every adjacency list must see the sequential loop's update sequence, so the graph is
    identical for 1, 3 and 16 threads -- levels, both adjacency arrays, entry point."""
    O = oracle
    base = _data(O, 9000, 24, "clustered", num_clusters=32, noise_level=0.6)
    base[100:140] = base[100]                                # equal edge distances: pruning ties
    graphs = []
    with eng.Index(base) as idx:
        for nt in ("1", "3", "16"):
            tune.set("BUILD_THREADS", nt)
            idx.hnsw_build(8, 64, 7)
            graphs.append(idx.get_graph())
    for g in graphs[1:]:
        for f in ("levels", "l0_adj", "up_off", "up_adj"):
            np.testing.assert_array_equal(getattr(g, f), getattr(graphs[0], f), err_msg=f)
        assert (g.entry, g.max_level, g.M) == (graphs[0].entry, graphs[0].max_level, graphs[0].M)
    assert ((graphs[0].l0_adj >= 0).sum(1) >= 1).all()


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_hnsw_hundreds_of_tied_candidates(eng, oracle, metric):
    """500 copies of one row: far more unexpanded candidates tie with the ef-th distance than the traversal
    kernel's 32 ghost slots hold.  The reference still expands every one of them (ultra_fast.clj:175-178 uses <=), so
    search repeats such queries on the device (a second pass of the kernel over the flagged queries) with the largest
    list the LDS holds: ids, distances AND the traversal counters (distance evaluations, expansions) equal the oracle's,
    through the synchronous and the asynchronous entry point."""
    O = oracle
    m = {"cosine": O.COSINE, "dot": O.DOT, "l2": O.L2}[metric]
    rs = np.random.RandomState(9)
    base = _data(O, 3000, 48, "clustered", num_clusters=6, noise_level=0.4)
    dup = rs.choice(3000, 500, replace=False)
    base[dup] = base[dup[0]]
    Q = np.vstack([base[dup[:2]], _data(O, 6, 48, seed=43)]).astype(np.float32)
    g = O.hnsw_build(base, m, M=5, ef_construction=40, seed=3, mode=O.MODE_DEV)
    with eng.Index(base, metric) as idx:
        idx.set_graph(g)
        for ef, k in [(50, 10), (7, 3), (300, 70)]:
            ids, d, st = idx.hnsw_search(Q, k, ef, want_stats=True)
            oi, od, ost, _ = O.hnsw_search(base, g, Q, k, ef=max(ef, k), metric=m, mode=O.MODE_DEV)
            assert_exact(ids, d, oi, od, "ties %s ef=%d" % (metric, ef))
            np.testing.assert_array_equal(st, ost, err_msg="ties %s ef=%d" % (metric, ef))
        import torch                                         # the asynchronous entry point repeats them as well
        Qt = torch.from_numpy(Q).cuda()
        stt = torch.zeros((len(Q), 2), dtype=torch.int64, device="cuda")
        ti, td = idx.hnsw_search_dev(Qt, 10, 50, stats=stt)
        torch.cuda.synchronize()
        oi, od, ost, _ = O.hnsw_search(base, g, Q, 10, ef=50, metric=m, mode=O.MODE_DEV)
        assert_exact(ti.cpu().numpy(), td.cpu().numpy(), oi, od, "ties dev %s" % metric)
        np.testing.assert_array_equal(stt.cpu().numpy(), ost)


def test_randomised_differential(eng, oracle):
    """40 random configurations (size, dim, metric, M, ef, k, nlist, nprobe, batch): every search entry point of
    the C ABI against the oracle's matching device-order mode, bit for bit."""
    O = oracle
    # HNSWGPU_SOAK=<n>: n more seeds with larger batches / dims (a soak run before a release, not part of the suite)
    soak = int(os.environ.get("HNSWGPU_SOAK", "1"))   # (one soak seed is part of the default run)
    for seed in [2026] + [3000 + i for i in range(soak)]:
        _differential_cases(eng, O, seed, big=seed != 2026)
        if soak:
            print("differential seed %d ok" % seed, file=sys.stderr, flush=True)   # a long soak must not look hung


def _differential_cases(eng, O, seed, big):
    rs = np.random.RandomState(seed)
    for case in range(40):
        n = int(rs.choice([3, 17, 64, 200, 777, 1500] + ([4000] if big else [])))
        dim = int(rs.choice([1, 2, 7, 16, 33, 96, 130, 260, 400] + ([768, 1000, 1300] if big else [])))
        metric = int(rs.choice([O.COSINE, O.L2, O.DOT]))
        dist = str(rs.choice(["gaussian", "uniform", "clustered"]))
        base = _data(O, n, dim, dist, seed=100 + case, num_clusters=4, noise_level=0.3)
        if rs.rand() < 0.3:
            base[rs.randint(0, n, max(1, n // 10))] = base[0]            # duplicates -> exact ties
        nq = int(rs.choice([1, 2, 5, 19, 40] + ([33, 70, 150] if big else [])))
        Q = np.vstack([_data(O, nq, dim, dist, seed=500 + case, num_clusters=4, noise_level=0.3)])
        Q[0] = base[min(1, n - 1)]
        k = int(rs.choice([1, 3, 10, 70]))
        tag = "seed %d case %d n=%d dim=%d metric=%d nq=%d k=%d" % (seed, case, n, dim, metric, nq, k)
        with eng.Index(base, metric) as idx:
            # HNSW on an oracle-built graph
            M = int(rs.choice([2, 5, 16]))
            g = O.hnsw_build(base, metric, M=M, ef_construction=int(rs.choice([8, 40])), seed=case, mode=O.MODE_DEV)
            idx.set_graph(g)
            ef = int(rs.choice([1, 7, 50, 300]))
            ids, d, st = idx.hnsw_search(Q, k, ef, want_stats=True)
            oi, od, ost, _ = O.hnsw_search(base, g, Q, k, ef=max(ef, k), metric=metric, mode=O.MODE_DEV)
            assert_exact(ids, d, oi, od, tag + " hnsw ef=%d M=%d" % (ef, M))
            np.testing.assert_array_equal(st, ost, err_msg=tag)
            # exact kNN (tile path from 16 queries on, cosine / dot)
            ids, d = idx.exact_knn(Q, k)
            mode = O.MODE_MFMA if (metric != O.L2 and nq >= 16) else O.MODE_DEV
            oi, od, _ = O.exact_knn(base, Q, k, metric=metric, mode=mode)
            assert_exact(ids, d, oi, od, tag + " exact")
            # IVF on random lists
            nlist = int(rs.choice([1, 3, 8, 20]))
            assign = rs.randint(0, nlist, n)
            off, lids = O.lists_from_assign(assign, nlist)
            cen = _data(O, nlist, dim, seed=900 + case)
            idx.set_ivf(cen, off, lids)
            nprobe = int(rs.choice([1, 2, nlist, nlist + 3]))
            ids, d, pr = idx.ivf_search(Q, k, nprobe, want_probes=True)
            oi, od, opr = O.ivf_search(base, cen, off, lids, Q, k, nprobe, metric=metric,
                                       mode=_ivf_mode(O, metric, dim, nq, nprobe, nlist))
            np.testing.assert_array_equal(pr[:, :min(nprobe, nlist)], opr, err_msg=tag + " probes")
            assert_exact(ids, d, oi, od, tag + " ivf nlist=%d nprobe=%d" % (nlist, nprobe))


def test_documented_limits(eng, oracle):
    """The maxima include/hnswgpu.h documents work (ef 4096, k 1024, M0 64, dim 3072) and one past them is an
    error code, not a fault."""
    O = oracle
    base = _data(O, 6000, 24)
    Q = _data(O, 3, 24, seed=43)
    g = O.hnsw_build(base, O.COSINE, M=32, ef_construction=80, mode=O.MODE_FAST)      # M0 = 64
    with eng.Index(base) as idx:
        idx.set_graph(g)
        ids, d, st = idx.hnsw_search(Q, 1024, 4096, want_stats=True)
        oi, od, ost, _ = O.hnsw_search(base, g, Q, 1024, ef=4096, mode=O.MODE_DEV)
        assert_exact(ids, d, oi, od, "ef=4096 k=1024")
        np.testing.assert_array_equal(st, ost)
        with pytest.raises(Exception, match="4096"):
            idx.hnsw_search(Q, 10, 4097)
        ei, ed = idx.exact_knn(Q, 1024)
        oi, od, _ = O.exact_knn(base, Q, 1024, mode=O.MODE_DEV)
        assert_exact(ei, ed, oi, od, "exact k=1024")
        with pytest.raises(Exception, match="1024"):
            idx.exact_knn(Q, 1025)
        idx.ivf_build(4, 2, 42)
        cen, off, lids = idx.get_ivf()
        ii, dd = idx.ivf_search(Q, 1024, 4)
        oi, od, _ = O.ivf_search(base, cen, off, lids, Q, 1024, 4, mode=_ivf_mode(O, O.COSINE, 24, 3, 4, 4))
        assert_exact(ii, dd, oi, od, "ivf k=1024")
        with pytest.raises(Exception, match="M"):
            bad = O.Graph(g.levels, np.full((6000, 65), -1, np.int32), g.up_off, g.up_adj, g.M, g.entry, g.max_level)
            idx.set_graph(bad)


def test_hnsw_large_index_hbm_visited(eng, oracle):
    """n > 262,144 rows: the visited set moves from the LDS bitset to generation stamps in HBM and the
    grid becomes persistent.  Same traversal, checked bit for bit against the oracle on the same graph."""
    O = oracle
    rs = np.random.RandomState(11)
    z = rs.randn(300_000, 6).astype(np.float32)
    base = (z @ rs.randn(6, 24).astype(np.float32) + 0.05 * rs.randn(300_000, 24).astype(np.float32))
    Q = base[rs.randint(0, 300_000, 24)] + 0.01 * rs.randn(24, 24).astype(np.float32)
    with eng.Index(base, "l2") as idx:
        idx.hnsw_build(8, 48, 42)
        g = idx.get_graph()
        for ef in (1, 40, 200):
            ids, d, st = idx.hnsw_search(Q, 10, ef, want_stats=True)
            oi, od, ost, _ = O.hnsw_search(base, g, Q, 10, ef=ef, metric=O.L2, mode=O.MODE_DEV)
            assert_exact(ids, d, oi, od, "large n ef=%d" % ef)
            np.testing.assert_array_equal(st, ost)
        big = np.tile(Q, (200, 1))                       # 4800 queries > resident slabs: persistent loop + reuse
        ids2, d2 = idx.hnsw_search(big, 10, 40)
        ids1, d1 = idx.hnsw_search(Q, 10, 40)
        assert np.array_equal(ids2, np.tile(ids1, (200, 1))) and np.array_equal(d2, np.tile(d1, (200, 1)))
        ex, _ = idx.exact_knn(Q, 10)
        assert O.recall(idx.hnsw_search(Q, 10, 200)[0], ex) >= 0.9


# ---- IVF-FLAT -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g256x64", "c1000x128"])
def test_ivf_build_golden(eng, oracle, name):
    import make_golden

    O = oracle
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    base, Q = make_golden.inputs(name)
    with eng.Index(base) as idx:
        np.testing.assert_array_equal(idx.kmeanspp(16), gold["ivf_kpp"])      # same D^2 samples as the f64 path
        a, d = idx.kmeans_assign(gold["ivf_cent"])
        oa, od = O.kmeans_assign(base, gold["ivf_cent"].astype(np.float64))
        flips = np.flatnonzero(a != oa)
        for i in flips:  # an assignment may only differ where the two best centroids tie within tolerance
            dd = np.sort([O.distance(O.COSINE, base[i], c) for c in gold["ivf_cent"]])
            assert dd[1] - dd[0] <= 1e-4 * abs(dd[0]) + 1e-6
        assert close(d, od).all()
        idx.ivf_build(16, 10, 42)
        cen, off, lids = idx.get_ivf()
        assign = np.empty(len(base), np.int64)
        for l in range(16):
            assign[lids[off[l]:off[l + 1]]] = l
            assert np.all(np.diff(lids[off[l]:off[l + 1]]) > 0)               # index order inside a list
        assert (assign != gold["ivf_assign"]).mean() <= 0.01
        if np.array_equal(assign, gold["ivf_assign"]):
            assert np.allclose(cen, gold["ivf_cent"], rtol=1e-5, atol=1e-6)
        # search: bit-exact vs the device-order oracle on the engine's own lists / centroids
        for nprobe, k in [(1, 10), (4, 10), (16, 10), (4, 40)]:
            ids, dist, pr = idx.ivf_search(Q, k, nprobe, want_probes=True)
            oi, odist, opr = O.ivf_search(base, cen, off, lids, Q, k, nprobe,
                                          mode=_ivf_mode(O, O.COSINE, base.shape[1], len(Q), nprobe, 16))
            np.testing.assert_array_equal(pr, opr)
            assert_exact(ids, dist, oi, odist, "ivf nprobe=%d" % nprobe)
            fi, fd, _ = O.ivf_search(base, cen, off, lids, Q, k, nprobe)
            assert_topk_parity(ids, dist, fi, fd, "ivf f64 nprobe=%d" % nprobe)
        # caller-chosen lists (the :turbo path)
        probes = np.tile(np.array([[3, -1, 7]], np.int32), (len(Q), 1))
        ids, dist = idx.ivf_search_lists(Q, 5, probes)
        members = set(lids[off[3]:off[4]].tolist()) | set(lids[off[7]:off[8]].tolist())
        assert all(i in members for i in ids.ravel() if i >= 0)


@pytest.mark.parametrize("solo", [2, 0, 1])
@pytest.mark.parametrize("metric,dim,M", [("cosine", 136, 16), ("l2", 72, 16), ("dot", 300, 32)])
def test_helpers_evaluate_small_launches(eng, oracle, tune, metric, dim, M, solo):
    """Launches of a handful of queries: helper workgroups on idle CUs evaluate the neighbours of the candidates the
    traversal will expand next and publish the distances; the traversal gathers only what has not arrived.  solo = 2: one
    query over several CUs at every ef (solo_kernels.hpp: an owner workgroup keeps the reference's order -- its sequencer
    wave holds the list as main list + admission buffer, hnsw_list.hpp --, its fetcher waves copy published distances into an LDS cache,
    the helpers evaluate and chase); 0: the round-2 helper kernel (kernels.hpp: pf_res); 1: the default rule (from ef 200).
    Timing decides WHICH distances arrive, never what they are: ids, distance bits and both counters equal the oracle's for
    1 / 3 / 20 / 64 queries, several times over, and the device counters show that published distances were used (the int8
    test is switched off here, so every neighbour not gathered locally was published)."""
    O = oracle
    tune.set("SOLO", solo)
    code = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    base = _data(O, 20000, dim, "clustered", seed=51)
    base[9000:9100] = base[17]                                  # ties among the candidates
    Q = np.concatenate([_data(O, 63, dim, "clustered", seed=52), base[17:18]]).astype(np.float32)
    with eng.Index(base, metric) as idx:
        idx.hnsw_build(M, 80, 42)                               # M = 32: 64 neighbour slots, 16 per helper
        g = idx.get_graph()
        idx.set_rejection_test(0)
        idx.set_profiling(True)
        used = 0
        for ef in (96, 640):                                    # (640: the headline's operating point -- a long list, many merges)
            oi, od, ost, _ = O.hnsw_search(base, g, Q, 10, ef=ef, metric=code, mode=O.MODE_DEV)
            for rep in range(3 if ef == 96 else 1):
                for lo, hi in [(0, 1), (1, 4), (4, 24), (0, 64), (63, 64)]:
                    idx.rejection_stats(reset=True)
                    ids, d, st = idx.hnsw_search(Q[lo:hi], 10, ef, want_stats=True)
                    gathered, neighbours = idx.rejection_stats(reset=True)
                    assert_exact(ids, d, oi[lo:hi], od[lo:hi], "helpers ef %d rep %d queries %d..%d" % (ef, rep, lo, hi))
                    np.testing.assert_array_equal(st, ost[lo:hi])
                    assert neighbours == int(ost[lo:hi, 0].sum()) and gathered <= neighbours
                    used += neighbours - gathered
        idx.set_profiling(False)
        assert used > 0, "no published distance was ever used"


@pytest.mark.parametrize("vis_global", [0, 1])
@pytest.mark.parametrize("metric,dim,M", [("cosine", 136, 16), ("l2", 72, 16), ("dot", 300, 32), ("cosine", 768, 8)])
def test_wave_kernel_against_oracle(eng, oracle, tune, metric, dim, M, vis_global):
    """Large launches run one wave per query on a main list + a register-resident admission buffer (wave_kernels.hpp: the
    list of hnsw_list.hpp, solo_kernels.hpp's sequencer keeps the same) instead of the single-workgroup kernel's positional merge; search-layer-ultra,
    ultra_fast.clj:151-212.  Forced here for batches of 130 and 600 queries (HNSW_WAVE = 2; by default launches that fill the
    chip take it: test_timed_launch_configurations_against_oracle, test_full_size_31k_properties), with the int8 rejection
    test on and off, the visited set in LDS and in HBM stamps, duplicated rows (hundreds of exact ties at the list's worst:
    ghosts, and lists that overflow into the repeat pass), ef from 1 to 900: ids, distance bits and both counters equal the
    oracle's, and the launch counter says the kernel ran."""
    O = oracle
    code = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    base = _data(O, 12000, dim, "clustered", seed=61)
    base[7000:7300] = base[23]                                  # 300 copies of one row
    base[100:140] = base[5]
    Q = np.concatenate([_data(O, 598, dim, "clustered", seed=62), base[23:24], base[5:6]]).astype(np.float32)
    tune.set("HNSW_WAVE", 2)
    tune.set("VIS_GLOBAL", vis_global)
    with eng.Index(base, metric) as idx:
        idx.hnsw_build(M, 80, 42)
        g = idx.get_graph()
        for ef, k in ((1, 1), (10, 10), (96, 10), (333, 100), (900, 10)):
            oi, od, ost, _ = O.hnsw_search(base, g, Q, k, ef=ef, metric=code, mode=O.MODE_DEV)
            for mode in (2, 0):
                idx.set_rejection_test(mode)
                for nq in (130, 600):
                    n0 = eng.debug_counter("hnsw_wave")
                    ids, d, st = idx.hnsw_search(Q[-nq:], k, ef, want_stats=True)
                    assert eng.debug_counter("hnsw_wave") > n0, "the wave kernel did not run"
                    assert_exact(ids, d, oi[-nq:], od[-nq:], "wave kernel %s ef %d mode %d nq %d" % (metric, ef, mode, nq))
                    np.testing.assert_array_equal(st, ost[-nq:])


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_rejection_test_modes_agree(eng, oracle, metric):
    """hnswgpu_set_rejection_test: off, large batches only, every launch -- ids, distance bits and the evals / hops
    counters of a batch large enough for mode 1 to switch the test on (>= 2 queries per CU) are identical, and equal to
    the oracle's on a subsample.  Clustered data with duplicates: ties at the list's worst are where a bound that was
    merely "almost" a lower bound would show."""
    O = oracle
    base = _data(O, 20000, 136, "clustered", seed=21)  # mode 1 needs dim >= 128
    base[5000:5200] = base[100]                      # 200 copies of one row
    Q = np.concatenate([_data(O, 1400, 136, "clustered", seed=22), base[100:101], base[5:45]]).astype(np.float32)
    code = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    with eng.Index(base, metric) as idx:
        idx.hnsw_build(12, 60, 42)
        res, rows = {}, {}
        idx.set_profiling(True)
        for mode in (0, 1, 2):
            idx.set_rejection_test(mode)
            idx.rejection_stats(reset=True)
            res[mode] = idx.hnsw_search(Q, 10, 64, want_stats=True)
            rows[mode] = idx.rejection_stats(reset=True)
        idx.set_profiling(False)
        # the counters: without the test every neighbour costs an f32 row, with it a minority does (and mode 1 did
        # switch it on for this batch); `neighbours` is the evals counter of the stats
        assert rows[0][1] == rows[2][1] == int(res[0][2][:, 0].sum())
        assert rows[0][0] > 0.8 * rows[0][1] and rows[2][0] < 0.85 * rows[0][0] and rows[1] == rows[2], rows
        for mode in (1, 2):
            np.testing.assert_array_equal(res[mode][0], res[0][0])
            np.testing.assert_array_equal(res[mode][1].view(np.uint32), res[0][1].view(np.uint32))
            np.testing.assert_array_equal(res[mode][2], res[0][2])
        small = idx.hnsw_search(Q[:3], 10, 64, want_stats=True)   # mode 2, a latency-sized launch
        np.testing.assert_array_equal(small[0], res[0][0][:3])
        np.testing.assert_array_equal(small[2], res[0][2][:3])
        g = idx.get_graph()
        sub = np.r_[0:24, len(Q) - 41:len(Q)]
        oi, od, ost, _ = O.hnsw_search(base, g, Q[sub], 10, ef=64, metric=code, mode=O.MODE_DEV)
        assert_exact(res[2][0][sub], res[2][1][sub], oi, od, "rejection test vs oracle, %s" % metric)
        np.testing.assert_array_equal(res[2][2][sub], ost)


@pytest.mark.parametrize("kind", ["gaussian", "clustered"])
def test_traversal_int8_test_is_calibrated_per_graph(eng, oracle, kind):
    """Rejection mode 1 measures on a graph's first large launch what the traversal's int8 test decides there
    (hnswgpu_hnsw_rejection_state: state 0 -> 1 -> 2) and switches it off for that graph when it leaves more than 65 % of the
    neighbours' f32 rows to fetch; afterwards a launch fetches what a launch without the test fetches (off) or fewer rows (on).  Ids,
    distance bits and counters never depend on the verdict: equal to mode 0's and to the oracle's on a subsample."""
    O = oracle
    if kind == "gaussian":
        base = _data(O, 9000, 256, "gaussian", seed=71)       # i.i.d.: every neighbour lies within the bounds' width of the worst
        Q = _data(O, 1300, 256, "gaussian", seed=72)
    else:
        base = _data(O, 9000, 256, "clustered", seed=71)
        Q = _data(O, 1300, 256, "clustered", seed=72)
    with eng.Index(base, "cosine") as idx:
        idx.hnsw_build(12, 60, 42)
        idx.set_rejection_test(0)
        idx.set_profiling(True)
        idx.rejection_stats(reset=True)
        want = idx.hnsw_search(Q, 10, 48, want_stats=True)
        rows_untested, _ = idx.rejection_stats(reset=True)     # f32 rows a launch fetches without the test
        idx.set_profiling(False)
        idx.set_rejection_test(1)                              # (mode 0 launches measure nothing: the graph is still unmeasured)
        assert idx.hnsw_rejection_state()[0] == 0
        got = [idx.hnsw_search(Q, 10, 48, want_stats=True) for _ in range(3)]
        state, off, frac = idx.hnsw_rejection_state()
        assert state == 2 and 0.0 < frac <= 1.0 and off == (frac > 0.65), (state, off, frac)
        idx.set_profiling(True)
        idx.rejection_stats(reset=True)
        got.append(idx.hnsw_search(Q, 10, 48, want_stats=True))
        f32_rows, neighbours = idx.rejection_stats(reset=True)
        idx.set_profiling(False)
        assert neighbours == int(want[2][:, 0].sum())
        assert (f32_rows == rows_untested) if off else (f32_rows < rows_untested), (off, f32_rows, rows_untested, neighbours)
        for g in got:
            np.testing.assert_array_equal(g[0], want[0])
            np.testing.assert_array_equal(g[1].view(np.uint32), want[1].view(np.uint32))
            np.testing.assert_array_equal(g[2], want[2])
        gr = idx.get_graph()
        oi, od, ost, _ = O.hnsw_search(base, gr, Q[:32], 10, ef=48, metric=O.COSINE, mode=O.MODE_DEV)
        assert_exact(want[0][:32], want[1][:32], oi, od, "calibrated traversal vs oracle, %s" % kind)
        np.testing.assert_array_equal(want[2][:32], ost)


def test_ivf_euclidean_large_batch_all_gemv_order(eng, oracle):
    """A Euclidean batch of more than 1024 queries: routing through the register-row group kernel, bounds on the matrix
    cores (dozens of queries per probed list), refine in the GEMV order -- every stage keeps the one arithmetic the
    Euclidean metric has at any batch size: probes, ids and distance bits equal the oracle's."""
    O = oracle
    base = _data(O, 3000, 136, "clustered", num_clusters=12, noise_level=0.3, seed=61)
    Q = _data(O, 1100, 136, "clustered", num_clusters=12, noise_level=0.3, seed=62)
    with eng.Index(base, "l2") as idx:
        idx.ivf_build(16, 3, 42)
        cen, off, lids = idx.get_ivf()
        ids, d, pr = idx.ivf_search(Q, 10, 4, want_probes=True)
        oi, od, opr = O.ivf_search(base, cen, off, lids, Q, 10, 4, metric=O.L2, mode=O.MODE_DEV)
        np.testing.assert_array_equal(pr, opr)
        assert_exact(ids, d, oi, od, "euclidean batch 1100")


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_ivf_bounds_pass_agrees_and_rejects(eng, oracle, metric):
    """The IVF bounds pass (stream_kernels.hpp): a batch in the GEMV regime with the int8 bounds pass on (mode 2) and off
    (mode 0) returns the same ids and distance bits, equal to the oracle's; the device counters show that the pass ran
    and excluded most candidates; duplicated rows (ties at the k-th distance) and k beyond the candidate count included."""
    O = oracle
    code = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    base = _data(O, 6000, 136, "clustered", num_clusters=30, noise_level=0.2, seed=31)
    base[3000:3040] = base[7]                               # 40 copies of one row: ties around the k-th distance
    Q = np.concatenate([_data(O, 15, 136, "clustered", num_clusters=30, noise_level=0.2, seed=32), base[7:8]]).astype(np.float32)
    with eng.Index(base, metric) as idx:
        idx.ivf_build(40, 4, 42)
        cen, off, lids = idx.get_ivf()
        idx.set_profiling(True)
        for nq, nprobe, k in [(16, 4, 10), (9, 5, 30), (16, 4, 64), (12, 6, 100), (16, 3, 256), (16, 2, 1000)]:
            assert metric == "l2" or nq * nprobe <= 12 * 40
            got = {}
            for mode in (2, 0):
                idx.set_rejection_test(mode)
                idx.rejection_stats(reset=True)
                got[mode] = idx.ivf_search(Q[:nq], k, nprobe)
                surv, cand = idx.rejection_stats(reset=True)
                if mode == 2 and k <= 256:
                    # it ran, and it rejected (the running threshold of a 150-row list is looser than a global one)
                    assert cand > 0 and (k > 30 or surv < 0.8 * cand), (surv, cand)
                else:
                    assert cand == 0                             # the f32 scans only (mode 0, or k beyond the bounds pass)
            np.testing.assert_array_equal(got[2][0], got[0][0])
            np.testing.assert_array_equal(got[2][1].view(np.uint32), got[0][1].view(np.uint32))
            oi, od, _ = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, metric=code, mode=O.MODE_DEV)
            assert_exact(got[2][0], got[2][1], oi, od, "ivf bounds pass %s nq=%d nprobe=%d k=%d" % (metric, nq, nprobe, k))
        idx.set_profiling(False)


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_ivf_survivor_stream_regimes(eng, oracle, metric, tune):
    """The survivor stream of the IVF list scan (stream_kernels.hpp) in each of its regimes, all bit-equal to the oracle:
    a handful of queries (every pair its own work item, no plan launch), grouped batches, survivor lists too small for
    what the bounds let through (HNSWGPU_STREAM_CAP: the finish kernel falls back to the candidate stream itself, i.e. the
    plain f32 scan), per-list buckets too small for the pairs of a hot list (the queries that do not fit take the same
    fallback), and routing through the separate launches instead of the fused routing kernel."""
    O = oracle
    code = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    base = _data(O, 9000, 200, "clustered", num_clusters=40, noise_level=0.25, seed=71)
    base[4000:4030] = base[11]                               # exact ties
    Q = np.concatenate([_data(O, 40, 200, "clustered", num_clusters=40, noise_level=0.25, seed=72), base[11:12]]).astype(np.float32)
    with eng.Index(base, metric) as idx:
        idx.ivf_build(50, 4, 42)
        cen, off, lids = idx.get_ivf()
        idx.set_rejection_test(2)
        want = {}

        def check(nq, k, nprobe, what):
            key = (nq, k, nprobe)
            if key not in want:
                want[key] = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, metric=code, mode=O.MODE_DEV)
            ids, d = idx.ivf_search(Q[:nq], k, nprobe)
            assert_exact(ids, d, want[key][0], want[key][1], "%s %s nq=%d k=%d nprobe=%d" % (what, metric, nq, k, nprobe))

        tune.set("IVF_CODES", "1")         # the bounds pass from one query on
        for nq, k, nprobe in [(1, 10, 8), (3, 5, 12), (4, 70, 6), (5, 10, 8), (12, 10, 12), (41, 10, 5), (41, 33, 12)]:
            if metric != "l2" and nq * nprobe > 12 * 50:
                continue                                      # beyond 12 pairs per list cosine / dot take the MFMA order
            check(nq, k, nprobe, "stream")
        tune.set("STREAM_CAP", "7")        # nothing fits: every query through the fallback
        for nq, k, nprobe in [(1, 10, 8), (12, 10, 12), (41, 33, 12)]:
            if metric != "l2" and nq * nprobe > 12 * 50:
                continue
            check(nq, k, nprobe, "fallback")
        tune.set("STREAM_CAP", "300")      # some queries fit, some do not
        check(12, 10, 12, "mixed fallback")
        tune.unset("STREAM_CAP")
        tune.set("STREAM_BUCKET", "3")     # three pairs fit a list's bucket: most queries take the fallback
        check(12, 10, 12, "full buckets")
        check(41, 10, 5, "full buckets")
        tune.set("STREAM_ROUTE", "0")      # ... filed by the separate routing launches
        check(41, 33, 12 if metric == "l2" else 5, "full buckets, separate routing")
        tune.unset("STREAM_BUCKET")
        tune.set("STREAM_ROUTE", "0")      # routing by the separate launches
        check(12, 10, 12, "separate routing")
        tune.set("STREAM_GROUP", "1000")   # ungrouped work items for a mid-size batch as well
        check(12, 10, 12, "ungrouped")


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_ivf_production_boundary(eng, oracle, metric, tune):
    """The default boundary between the two summation orders of a cosine / dot IVF search: with int8 and half-precision
    list rows (and k <= 256) the survivor stream -- GEMV order -- serves EVERY batch size; without them (mode 0), or for
    a k the stream does not serve, the MFMA tile scan takes over beyond 12 (query, list) pairs per list.  (The suite
    otherwise pins the boundary at 12.)"""
    O = oracle
    code = {"cosine": O.COSINE, "dot": O.DOT}[metric]
    tune.unset("TILE_PAIRS")
    nlist, nprobe = 20, 10
    base = _data(O, 8000, 136, "clustered", num_clusters=20, noise_level=0.3, seed=81)
    Q = _data(O, 120, 136, "clustered", num_clusters=20, noise_level=0.3, seed=82)
    with eng.Index(base, metric) as idx:
        idx.ivf_build(nlist, 4, 42)
        cen, off, lids = idx.get_ivf()
        for nq, k, mode_rej, want in [(40, 10, 2, O.MODE_DEV),       # 20 pairs per list, int8 rows: the stream
                                      (96, 10, 2, O.MODE_DEV),       # 48: still the stream
                                      (120, 10, 2, O.MODE_DEV),      # 60: and still (the half-precision pass on top)
                                      (40, 300, 2, O.MODE_MFMA),     # a k the stream does not serve: boundary 12
                                      (40, 10, 0, O.MODE_MFMA),      # no int8 rows: boundary 12
                                      (20, 10, 0, O.MODE_DEV)]:      # 10 pairs per list without them: the f32 GEMV order
            idx.set_rejection_test(mode_rej)
            ids, d = idx.ivf_search(Q[:nq], k, nprobe)
            oi, od, _ = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, metric=code, mode=want)
            assert_exact(ids, d, oi, od, "production boundary %s nq=%d k=%d rejection mode %d" % (metric, nq, k, mode_rej))


@pytest.mark.parametrize("dim", [24, 300, 768, 1024, 1536, 2048, 2050, 3072])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_rejection_bounds_never_exceed_the_distance(eng, metric, dim):
    """The HNSW traversal skips the f32 row of a neighbour whose int8 lower bound is already >= the list's worst
    (kernels.hpp: quantize_rows_kernel).  That is only exact if the bound never exceeds the distance the exact path
    computes: checked for every row-loader width and metric on rows of very different scale, a zero row, a row with
    one huge component, duplicates of the query, a zero query and a non-finite row -- and the bound must be TIGHT
    (within 4 % of the distance scale), or the test would silently stop rejecting anything."""
    rs = np.random.RandomState(dim)
    n = 800
    base = rs.randn(n, dim).astype(np.float32) * np.exp(rs.uniform(-6, 6, (n, 1))).astype(np.float32)
    base[:200] = rs.randn(200, dim).astype(np.float32)          # a well-behaved block for the tightness check
    base[200] = 0.0
    base[201, 3] = 1.0e6
    base[202] = base[5]
    base[203, 1] = np.inf
    base[204, 2] = np.nan
    ids = np.arange(n, dtype=np.int32)
    queries = [rs.randn(dim).astype(np.float32), base[5].copy(), (base[7] * 1000).astype(np.float32),
               np.zeros(dim, np.float32), base[201].copy()]
    with eng.Index(base, metric) as idx:
        idx.set_rejection_test(2)          # int8 rows whatever the default mode and the dim
        for qi, q in enumerate(queries):
            lb, ub = idx.distance_bounds(q, ids)
            np.testing.assert_array_equal(lb.view(np.uint32), idx.rejection_bounds(q, ids).view(np.uint32))
            d = idx.batch_distances(q, ids)
            ok = ~np.isnan(lb)
            assert np.all(lb[ok] <= d[ok]), "metric %s dim %d query %d: bound above the distance at rows %s" % (
                metric, dim, qi, np.nonzero(ok & ~(lb <= d))[0][:8])
            # the UPPER bound sets the IVF bounds pass's threshold (k candidates with ub <= tau put D_k at or below tau):
            # it may never be below the distance the exact path computes
            oku = ~np.isnan(ub) & ~np.isnan(d)
            assert np.all(d[oku] <= ub[oku]), "metric %s dim %d query %d: upper bound below the distance at rows %s" % (
                metric, dim, qi, np.nonzero(oku & ~(d <= ub))[0][:8])
            assert np.isnan(lb[203]) and np.isnan(lb[204])            # non-finite rows abstain
            assert not (ub[203] < np.inf) and not (ub[204] < np.inf)  # ... on both sides (NaN or +inf: no threshold from them)
            if qi == 0:                                               # tightness on the well-behaved block
                qn, vn = np.linalg.norm(q), np.linalg.norm(base[:200], axis=1)
                scale = {"cosine": 1.0, "dot": qn * vn, "l2": qn + vn}[metric]
                gap = (d[:200] - lb[:200]) / scale
                assert ok[:200].all() and gap.max() < 0.04, gap.max()
                gap_u = (ub[:200] - d[:200]) / scale
                assert gap_u.max() < 0.04, gap_u.max()


@pytest.mark.parametrize("dim", [24, 300, 768, 3072])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_half_precision_bounds_hold_and_are_tight(eng, metric, dim):
    """Batches of 1.5 M candidates and more filter the int8 survivors of an IVF search with HALF-precision list rows
    (stream_kernels.hpp step 1b) before any f32 row is fetched: a candidate is dropped when its lower bound is above
    the k-th smallest upper bound.  Both sides must hold against the distance the exact path computes -- rows of very
    different scale (the per-row power-of-two scale), a zero row, a huge component (fp16 would overflow unscaled), tiny
    rows (fp16 would flush unscaled), duplicates of the query, a zero query; non-finite rows abstain -- and they must be
    TIGHT: within 1e-3 of the distance scale, forty times narrower than the int8 bounds, or the pass would filter
    nothing."""
    rs = np.random.RandomState(dim + 1)
    n = 600
    base = rs.randn(n, dim).astype(np.float32) * np.exp(rs.uniform(-6, 6, (n, 1))).astype(np.float32)
    base[:200] = rs.randn(200, dim).astype(np.float32)
    base[200] = 0.0
    base[201, 3] = 1.0e6
    base[202] = base[5]
    base[203, 1] = np.inf
    base[204, 2] = np.nan
    base[205] = (rs.randn(dim) * 1e-9).astype(np.float32)
    base[206] = (rs.randn(dim) * 1e9).astype(np.float32)
    # lists by hand (k-means on non-finite rows is not the subject): three lists, rows dealt round-robin
    lids = np.concatenate([np.arange(l, n, 3) for l in range(3)]).astype(np.int32)
    off = np.cumsum([0] + [len(np.arange(l, n, 3)) for l in range(3)]).astype(np.int64)
    pos = np.empty(n, np.int32)
    pos[lids] = np.arange(n, dtype=np.int32)                  # list position of base row i
    queries = [rs.randn(dim).astype(np.float32), base[5].copy(), (base[7] * 1000).astype(np.float32),
               np.zeros(dim, np.float32), base[201].copy(), base[205].copy()]
    with eng.Index(base, metric) as idx:
        idx.set_rejection_test(2)
        idx.set_ivf(base[:3].copy(), off, lids)
        rows = np.arange(n, dtype=np.int32)                   # every list position
        for qi, q in enumerate(queries):
            lb, ub = idx.ivf_half_bounds(q, rows)
            d = idx.batch_distances(q, lids)                  # the exact path, same order
            ok = ~np.isnan(lb) & ~np.isnan(d)
            assert np.all(lb[ok] <= d[ok]), "metric %s dim %d query %d: lower bound above the distance at list rows %s" % (
                metric, dim, qi, np.nonzero(ok & ~(lb <= d))[0][:8])
            oku = ~np.isnan(ub) & ~np.isnan(d)
            assert np.all(d[oku] <= ub[oku]), "metric %s dim %d query %d: upper bound below the distance at list rows %s" % (
                metric, dim, qi, np.nonzero(oku & ~(d <= ub))[0][:8])
            for bad in (203, 204):
                assert np.isnan(lb[pos[bad]]) and not (ub[pos[bad]] < np.inf)
            if qi == 0:
                blk = pos[:200]
                qn, vn = np.linalg.norm(q), np.linalg.norm(base[:200], axis=1)
                scale = {"cosine": 1.0, "dot": qn * vn, "l2": qn + vn}[metric]
                assert ok[blk].all()
                assert ((d[blk] - lb[blk]) / scale).max() < 1e-3 and ((ub[blk] - d[blk]) / scale).max() < 1e-3


@pytest.mark.parametrize("dim", [128, 384, 768, 1536, 3072])
@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_home_list_bounds_hold_and_are_tight(eng, metric, dim):
    """Large batches put the half-precision rows of a query's NEAREST list through the matrix cores once for all the
    queries it is nearest to (stream_kernels.hpp step 1a, ivf_home_kernel: v_mfma_f32_16x16x32_f16, the query in two fp16
    planes) and the bounds of every row of that list come from there.  Same obligations as the per-survivor pass: lb <= d
    <= ub against the exact path for rows of very different scale, a zero row, a huge component, tiny and huge rows,
    duplicates of the query, a zero query; non-finite rows and queries abstain; and tight -- within 1.5e-3 of the distance
    scale.  More queries than one group holds (17 / 9 / 5 by row length), a row count that ends inside a 16-row block."""
    rs = np.random.RandomState(dim + 7)
    n = 603
    base = rs.randn(n, dim).astype(np.float32) * np.exp(rs.uniform(-6, 6, (n, 1))).astype(np.float32)
    base[:200] = rs.randn(200, dim).astype(np.float32)
    base[200] = 0.0
    base[201, 3] = 1.0e6
    base[202] = base[5]
    base[203, 1] = np.inf
    base[204, 2] = np.nan
    base[205] = (rs.randn(dim) * 1e-9).astype(np.float32)
    base[206] = (rs.randn(dim) * 1e9).astype(np.float32)
    lids = np.concatenate([np.arange(l, n, 3) for l in range(3)]).astype(np.int32)
    off = np.cumsum([0] + [len(np.arange(l, n, 3)) for l in range(3)]).astype(np.int64)
    pos = np.empty(n, np.int32)
    pos[lids] = np.arange(n, dtype=np.int32)
    queries = [rs.randn(dim).astype(np.float32), base[5].copy(), (base[7] * 1000).astype(np.float32),
               np.zeros(dim, np.float32), base[201].copy(), base[205].copy(), base[206].copy()]
    queries += [rs.randn(dim).astype(np.float32) * np.float32(np.exp(rs.uniform(-8, 8))) for _ in range(12)]
    bad_q = rs.randn(dim).astype(np.float32)
    bad_q[1] = np.inf
    queries.append(bad_q)
    Q = np.stack(queries)
    with eng.Index(base, metric) as idx:
        idx.set_rejection_test(2)
        idx.set_ivf(base[:3].copy(), off, lids)
        for (r0, r1) in ((0, n), (int(off[1]), int(off[2])), (5, 5 + 37)):
            LB, UB = idx.ivf_home_bounds(Q, r0, r1)
            for qi, q in enumerate(queries):
                lb, ub = LB[qi], UB[qi]
                if qi == len(queries) - 1:                       # a non-finite query has no bounds at all
                    assert np.isnan(lb).all() and not (ub < np.inf).any()
                    continue
                d = idx.batch_distances(q, lids)[r0:r1]          # the exact path, list order
                ok = ~np.isnan(lb) & ~np.isnan(d)
                assert np.all(lb[ok] <= d[ok]), "metric %s dim %d query %d: lower bound above the distance at list rows %s" % (
                    metric, dim, qi, r0 + np.nonzero(ok & ~(lb <= d))[0][:8])
                oku = ~np.isnan(ub) & ~np.isnan(d)
                assert np.all(d[oku] <= ub[oku]), "metric %s dim %d query %d: upper bound below the distance at list rows %s" % (
                    metric, dim, qi, r0 + np.nonzero(oku & ~(d <= ub))[0][:8])
                for bad in (203, 204):
                    if r0 <= pos[bad] < r1:
                        assert np.isnan(lb[pos[bad] - r0]) and not (ub[pos[bad] - r0] < np.inf)
                if qi == 0 and r0 == 0:
                    blk = pos[:200]
                    qn, vn = np.linalg.norm(q), np.linalg.norm(base[:200], axis=1)
                    scale = {"cosine": 1.0, "dot": qn * vn, "l2": qn + vn}[metric]
                    assert ok[blk].all()
                    assert ((d[blk] - lb[blk]) / scale).max() < 1.5e-3 and ((ub[blk] - d[blk]) / scale).max() < 1.5e-3
                    if metric != "l2":
                        # ... and the bounds' centre against f64: within the half-precision copy's own error
                        c64 = (base[:200].astype(np.float64) @ q.astype(np.float64)) / (qn * vn.astype(np.float64))
                        mid = 0.5 * (lb[blk].astype(np.float64) + ub[blk].astype(np.float64)) / scale
                        ref = (1.0 - c64) if metric == "cosine" else -c64
                        assert np.abs(mid - ref).max() < 3e-4, np.abs(mid - ref).max()
                    if metric == "cosine":
                        # ... and the matrix cores' ACCUMULATION alone (the kernel allows 1.1e-4 |q||v| for it): the same fp16
                        # planes built here -- rows h = fp16(v / s), s = 2^(e - 14); the query as hi + 2^-12 lo -- and summed in f64
                        def pow2_scale(x):
                            return np.float32(2.0) ** (np.floor(np.log2(np.abs(x).max(axis=-1, keepdims=True))) - 14)
                        rows = base[:200]
                        sv = pow2_scale(rows)
                        h = (rows / sv).astype(np.float16).astype(np.float64)
                        sq_ = pow2_scale(q)
                        x = (q / sq_).astype(np.float32)
                        hi = x.astype(np.float16).astype(np.float32)
                        lo = ((x - hi) * np.float32(4096.0)).astype(np.float16).astype(np.float64)
                        exact = (h @ (hi.astype(np.float64) + lo / 4096.0)) * (sv[:, 0].astype(np.float64) * float(sq_[0])) / (qn * vn.astype(np.float64))
                        acc_err = np.abs((1.0 - exact) - mid).max()
                        print("matrix-core accumulation error, dim %d: %.2e of |q||v| (allowance 1.1e-4)" % (dim, acc_err))
                        assert acc_err < 2e-5, acc_err


@pytest.mark.parametrize("metric,dim", [("cosine", 128), ("dot", 128), ("l2", 128), ("cosine", 384), ("cosine", 768), ("l2", 768),
                                        ("cosine", 1536), ("dot", 3072)])   # (groups of 16 / 8 / 4 queries by row length)
def test_ivf_home_list_pass(eng, oracle, metric, dim, tune):
    """Large IVF batches with the home-list pass (production: from 1024 queries and half a query per list), bit-equal to
    the oracle: forced on for small batches through the tuning table (queries ordered by nearest list from one query on),
    lists that are home to more queries than one group holds, lists home to none, k of one / beyond a wave, exact ties,
    survivor lists that overflow next to it, heavy queries (whose slice 0 appends the home rows), and the counters show
    that f32 rows were fetched for little more than k candidates per query."""
    O = oracle
    code = {"cosine": O.COSINE, "dot": O.DOT, "l2": O.L2}[metric]
    n = 9000 if dim <= 768 else 4500
    base = _data(O, n, dim, "clustered", num_clusters=40, noise_level=0.25, seed=73)
    base[4000:4030] = base[11]                               # exact ties
    Q = np.concatenate([_data(O, 299, dim, "clustered", num_clusters=40, noise_level=0.25, seed=74), base[11:12]]).astype(np.float32)
    with eng.Index(base, metric) as idx:
        idx.ivf_build(50, 4, 42)
        cen, off, lids = idx.get_ivf()
        idx.set_rejection_test(2)
        idx.set_profiling(True)
        tune.set("TILE_PAIRS", str(1 << 40))   # the GEMV-order paths at every batch size (the production rule of such a handle)
        tune.set("IVF_CODES", "1")
        tune.set("STREAM_MID", "1")
        tune.set("FINISH_ORDER", "1")
        tune.set("STREAM_HOME", "1")

        def check(nq, k, nprobe, what, expect_few=True):
            idx.rejection_stats(reset=True)
            ids, d = idx.ivf_search(Q[-nq:], k, nprobe)
            surv, cand = idx.rejection_stats(reset=True)
            oi, od, _ = O.ivf_search(base, cen, off, lids, Q[-nq:], k, nprobe, metric=code, mode=O.MODE_DEV)
            assert_exact(ids, d, oi, od, "%s %s nq=%d k=%d nprobe=%d" % (what, metric, nq, k, nprobe))
            if expect_few:                                    # (+ 32: the strays the finish kernel takes as they are)
                assert cand > 0 and surv <= nq * (max(k + 40, 128) + 32), (what, surv, cand, nq, k)

        for nq, k, nprobe in [(1, 10, 8), (3, 1, 12), (41, 10, 5), (41, 70, 12), (300, 10, 12), (300, 100, 50), (170, 10, 1)]:
            check(nq, k, nprobe, "home forced")
        tune.set("HOME_STRAYS", "0")       # every appended candidate through the per-survivor half-precision pass
        check(300, 10, 12, "no strays")
        check(41, 70, 12, "no strays")
        tune.set("HOME_STRAYS", "100000")  # ... none of them
        check(300, 10, 12, "all strays", expect_few=False)
        tune.unset("HOME_STRAYS")
        tune.set("STREAM_HOME", "0")
        check(300, 10, 12, "home off")
        tune.set("STREAM_WIDE2", "1")      # the bounds pass with two 32-query column blocks per group (production: the largest batches)
        check(300, 10, 12, "home off, two column blocks")
        tune.set("STREAM_HOME", "1")
        check(300, 10, 12, "two column blocks")
        check(300, 100, 50, "two column blocks")
        check(170, 10, 1, "two column blocks")
        tune.set("STREAM_WIDE2", "4")      # ... with four (production from 96 pairs per list): groups of up to 128 members
        wide0 = eng.debug_counter("bounds_two_column_blocks")
        check(300, 10, 12, "four column blocks")
        assert (eng.debug_counter("bounds_two_column_blocks") > wide0) == (dim <= 1024)   # (rows of up to 1024 bytes of codes)
        check(300, 100, 50, "four column blocks")
        check(170, 10, 1, "four column blocks")
        tune.set("STREAM_HOME", "0")
        check(300, 10, 12, "home off, four column blocks")
        tune.set("STREAM_HOME", "1")
        tune.unset("STREAM_WIDE2")
        tune.set("QUERY_WAVES", "1")       # the per-query kernels with a wave per query (production from 2048 queries)
        tw0 = eng.debug_counter("route_tail_waves")
        check(300, 10, 12, "a wave per query")
        assert eng.debug_counter("route_tail_waves") > tw0
        check(41, 64, 12, "a wave per query")
        check(300, 100, 50, "a wave per query (k beyond a wave: the workgroup kernels)")
        check(3, 1, 12, "a wave per query")
        tune.set("QUERY_WAVES", "0")
        check(300, 10, 12, "a workgroup per query")
        tune.unset("QUERY_WAVES")
        tune.set("STREAM_CAP", "300")      # some lists overflow (and home rows that do not fit send a query through the fallback)
        check(300, 10, 12, "mixed fallback", expect_few=False)
        tune.set("STREAM_HEAVY_MEAN", "0")
        for thr in ("1", "8"):
            tune.set("STREAM_HEAVY_MIN", thr)
            check(41, 33, 5, "heavy + fallback, threshold " + thr, expect_few=False)
        tune.unset("STREAM_CAP")
        tune.set("STREAM_HEAVY_MIN", "1")
        check(300, 10, 12, "every query with foreign survivors heavy", expect_few=False)
        idx.set_profiling(False)


@pytest.mark.parametrize("metric,dim,nlist", [("cosine", 256, 50), ("dot", 256, 77), ("cosine", 512, 33), ("cosine", 768, 130), ("dot", 768, 64)])
def test_ivf_routing_on_the_matrix_cores(eng, oracle, metric, dim, nlist, tune):
    """The centroid distances of large batches come from the f32 matrix cores IN THE GEMV ORDER (ivf_route_mfma_kernel: one
    v_mfma_f32_32x32x2_f32 chain per lane partial, the 64 partial tiles added in the butterfly's tree): the probed lists, their
    order, and with them every id and distance bit must be what the VALU routing gives and what the oracle's device order
    gives -- rows of very different scale, a zero query, a zero centroid row's worth of duplicates, table sizes that end inside
    a 32-centroid tile, batches that end inside a 32-query group, every slicing of the table."""
    O = oracle
    code = {"cosine": O.COSINE, "dot": O.DOT}[metric]
    rs = np.random.RandomState(dim + nlist)
    base = _data(O, 6000, dim, "clustered", num_clusters=nlist, noise_level=0.3, seed=91)
    base *= np.exp(rs.uniform(-3, 3, (len(base), 1))).astype(np.float32)      # (row norms of very different size)
    base[100:140] = base[7]                                                    # duplicates: ties between candidates
    Q = _data(O, 170, dim, "clustered", num_clusters=nlist, noise_level=0.3, seed=92).astype(np.float32)
    if metric == "cosine":                                                     # (dot: -0 against the engine's canonical +0, whatever the routing)
        Q[5] = 0.0
    Q[6] = base[7]
    with eng.Index(base, metric) as idx:
        idx.ivf_build(nlist, 3, 42)
        cen, off, lids = idx.get_ivf()
        idx.set_rejection_test(2)
        tune.set("TILE_PAIRS", str(1 << 40))
        tune.set("IVF_CODES", "1")
        for nq, k, nprobe in [(170, 10, 8), (33, 5, nlist), (64, 10, 1)]:
            oi, od, _ = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, metric=code, mode=O.MODE_DEV)
            tune.set("ROUTE_MFMA", "0")
            ids0, d0, pr0 = idx.ivf_search(Q[:nq], k, nprobe, want_probes=True)
            assert_exact(ids0, d0, oi, od, "VALU routing %s dim %d nq=%d" % (metric, dim, nq))
            for sl in (1, 2, 3, 64):                                           # auto, and explicit slicings of the table
                tune.set("ROUTE_MFMA", str(sl))
                ids, d, pr = idx.ivf_search(Q[:nq], k, nprobe, want_probes=True)
                np.testing.assert_array_equal(pr, pr0, err_msg="probed lists %s dim %d nq=%d slices %d" % (metric, dim, nq, sl))
                assert_exact(ids, d, oi, od, "matrix-core routing %s dim %d nq=%d slices %d" % (metric, dim, nq, sl))


@pytest.mark.parametrize("dim", [128, 768, 3072])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_bounds_randomised_soak(eng, metric, dim):
    """Every bit-exact result of the int8 / half-precision paths hangs on lb <= d <= ub against the distance the exact path
    computes (kernels.hpp: code_bounds; stream_kernels.hpp: the half-precision bounds): a randomised check over (query,
    row) pairs built to stress the slack constants -- per-row scales e^+-12 (f32 rounding of sums of very different
    magnitude), rows that are near-duplicates of the query (distance ~ 0: cancellation in 1 - dot / (|q||v|) and in
    |q - v|), rows whose dot with the query cancels to ~0 by construction (sign-alternating copies), sparse rows with one
    dominant component, and queries of the same families.  1.2e5 pairs per (metric, dim) in the suite (one soak unit:
    HNSWGPU_SOAK defaults to 1); HNSWGPU_SOAK=<n> runs n units with fresh seeds."""
    reps = 1 + int(os.environ.get("HNSWGPU_SOAK", "1")) * 5       # (one soak unit is part of the default run)
    n = 2000
    for rep in range(reps):
        rs = np.random.RandomState(1000 * rep + dim + {"cosine": 0, "l2": 1, "dot": 2}[metric])
        scale = np.exp(rs.uniform(-12, 12, (n, 1)))
        base = (rs.randn(n, dim) * scale).astype(np.float32)
        qs = [rs.randn(dim).astype(np.float32) * np.float32(np.exp(rs.uniform(-12, 12))) for _ in range(6)]
        # near-duplicates of query 0 at relative distances 1e-7 .. 1e-2, and exact copies at other scales
        for j in range(200):
            base[j] = (qs[0] * (1.0 + 0.0 * j) + rs.randn(dim).astype(np.float32) * np.linalg.norm(qs[0]) / np.sqrt(dim) * 10.0 ** rs.uniform(-7, -2)).astype(np.float32)
        for j in range(200, 260):
            base[j] = (qs[0] * np.float32(np.exp(rs.uniform(-10, 10)))).astype(np.float32)
        # rows orthogonal to query 1 by construction: its elements with alternating signs and pairwise swapped
        q1 = qs[1]
        orth = np.empty(dim, np.float32)
        orth[0::2], orth[1::2] = q1[1::2], -q1[0::2]
        for j in range(260, 330):
            base[j] = (orth * np.float32(np.exp(rs.uniform(-6, 6))) + rs.randn(dim).astype(np.float32) * np.float32(np.linalg.norm(q1) / np.sqrt(dim) * 10.0 ** rs.uniform(-8, -3))).astype(np.float32)
        # sparse rows: one dominant component over a tiny tail
        for j in range(330, 400):
            base[j] = (rs.randn(dim) * 1e-6).astype(np.float32)
            base[j, rs.randint(dim)] = np.float32(rs.randn() * np.exp(rs.uniform(-3, 8)))
        qs.append(base[331].copy())
        qs.append((orth * 3.0).astype(np.float32))
        ids = np.arange(n, dtype=np.int32)
        lids = np.concatenate([np.arange(l, n, 2) for l in range(2)]).astype(np.int32)
        off = np.array([0, len(np.arange(0, n, 2)), n], np.int64)
        with eng.Index(base, metric) as idx:
            idx.set_rejection_test(2)
            idx.set_ivf(base[:2].copy(), off, lids)
            for qi, q in enumerate(qs):
                d = idx.batch_distances(q, ids)
                lb, ub = idx.distance_bounds(q, ids)                                      # int8, base order
                ok = ~np.isnan(lb) & ~np.isnan(d)
                assert np.all(lb[ok] <= d[ok]), "int8 lb > d: %s dim %d rep %d query %d rows %s" % (metric, dim, rep, qi, np.nonzero(ok & ~(lb <= d))[0][:6])
                oku = ~np.isnan(ub) & ~np.isnan(d)
                assert np.all(d[oku] <= ub[oku]), "int8 ub < d: %s dim %d rep %d query %d rows %s" % (metric, dim, rep, qi, np.nonzero(oku & ~(d <= ub))[0][:6])
                hl, hu = idx.ivf_half_bounds(q, ids)                                      # fp16, list order
                dl = d[lids]
                ok = ~np.isnan(hl) & ~np.isnan(dl)
                assert np.all(hl[ok] <= dl[ok]), "fp16 lb > d: %s dim %d rep %d query %d list rows %s" % (metric, dim, rep, qi, np.nonzero(ok & ~(hl <= dl))[0][:6])
                oku = ~np.isnan(hu) & ~np.isnan(dl)
                assert np.all(dl[oku] <= hu[oku]), "fp16 ub < d: %s dim %d rep %d query %d list rows %s" % (metric, dim, rep, qi, np.nonzero(oku & ~(dl <= hu))[0][:6])
            if True:                                                                      # fp16 on the matrix cores (the home-list pass), list order
                Ml, Mu = idx.ivf_home_bounds(np.stack(qs), 0, n)
                for qi, q in enumerate(qs):
                    dl = idx.batch_distances(q, ids)[lids]
                    ok = ~np.isnan(Ml[qi]) & ~np.isnan(dl)
                    assert np.all(Ml[qi][ok] <= dl[ok]), "mfma fp16 lb > d: %s dim %d rep %d query %d list rows %s" % (metric, dim, rep, qi, np.nonzero(ok & ~(Ml[qi] <= dl))[0][:6])
                    oku = ~np.isnan(Mu[qi]) & ~np.isnan(dl)
                    assert np.all(dl[oku] <= Mu[qi][oku]), "mfma fp16 ub < d: %s dim %d rep %d query %d list rows %s" % (metric, dim, rep, qi, np.nonzero(oku & ~(dl <= Mu[qi]))[0][:6])


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_ivf_half_precision_pass(eng, oracle, metric, tune):
    """The half-precision pass between the int8 bounds and the f32 rows (production: batches with 1.5 M candidates and
    more), bit-equal to the oracle: at its production threshold (a Euclidean batch of 170 over all 9000 rows), forced on for small batches in
    every slice configuration, next to survivor lists that overflow (those queries skip it and take the fallback), and
    with it the finish kernel's threshold from upper bounds -- for a k of one, a k beyond a wave, and ties."""
    O = oracle
    code = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    base = _data(O, 9000, 200, "clustered", num_clusters=40, noise_level=0.25, seed=73)
    base[4000:4030] = base[11]                               # exact ties
    Q = np.concatenate([_data(O, 169, 200, "clustered", num_clusters=40, noise_level=0.25, seed=74), base[11:12]]).astype(np.float32)
    with eng.Index(base, metric) as idx:
        idx.ivf_build(50, 4, 42)
        cen, off, lids = idx.get_ivf()
        idx.set_rejection_test(2)
        idx.set_profiling(True)

        def check(nq, k, nprobe, what, expect_few=True):
            idx.rejection_stats(reset=True)
            ids, d = idx.ivf_search(Q[-nq:], k, nprobe)
            surv, cand = idx.rejection_stats(reset=True)
            oi, od, _ = O.ivf_search(base, cen, off, lids, Q[-nq:], k, nprobe, metric=code, mode=O.MODE_DEV)
            assert_exact(ids, d, oi, od, "%s %s nq=%d k=%d nprobe=%d" % (what, metric, nq, k, nprobe))
            if expect_few:                                    # it ran: f32 rows for little more than k candidates
                assert cand > 0 and surv <= nq * max(k + 40, 128), (what, surv, cand, nq, k)   # (<= 128 int8 survivors: all fetched)

        if metric == "l2":                                   # (cosine / dot: the suite pins such a batch to the tile scan)
            check(170, 10, 50, "production threshold")       # 170 x 9000 candidates
            check(150, 10, 50, "below the threshold", expect_few=False)
        tune.set("IVF_CODES", "1")
        tune.set("STREAM_MID", "1")        # from one query on
        for nq, k, nprobe in [(1, 10, 8), (3, 1, 12), (12, 10, 12), (41, 10, 5), (41, 70, 12)]:
            if metric != "l2" and nq * nprobe > 12 * 50:
                continue
            check(nq, k, nprobe, "forced")
        for sl in ("1", "3", "64"):
            tune.set("MID_SLICES", sl)
            tune.set("FINISH_SLICES", sl)
            check(12, 10, 12, "slices " + sl)
        tune.unset("MID_SLICES")
        tune.unset("FINISH_SLICES")
        tune.set("STREAM_CAP", "300")      # some survivor lists overflow: those queries take the fallback
        check(12, 10, 12, "mixed fallback", expect_few=False)
        # large batches give a query ONE workgroup per pass; the queries that is too little for (many survivors, or the
        # fallback's scan of every candidate) are listed and served by 64 slices each (ivf_heavy_kernel): forced here by
        # ordering from one query on (one workgroup per query) and a threshold of 8 / 100 survivors
        tune.set("FINISH_ORDER", "1")
        tune.set("FINISH_SLICES", "1")
        tune.set("STREAM_HEAVY_MEAN", "0")  # (production: also at least four times the batch's mean)
        for thr in ("8", "100"):
            tune.set("STREAM_HEAVY_MIN", thr)
            check(12, 10, 12, "heavy + fallback, threshold " + thr, expect_few=False)
            check(41, 33, 12 if metric == "l2" else 5, "heavy + fallback, threshold " + thr, expect_few=False)
        tune.unset("STREAM_CAP")
        tune.set("STREAM_HEAVY_MIN", "8")
        check(41, 10, 5, "every query heavy", expect_few=False)
        check(3, 1, 12, "every query heavy", expect_few=False)
        tune.set("STREAM_HEAVY_MEAN", "1")  # above the mean: about half of them
        check(41, 10, 5, "half the queries heavy", expect_few=False)
        idx.set_profiling(False)


@pytest.mark.parametrize("n,dim,nlist,metric", [(6000, 48, 40, 0), (3000, 100, 17, 2), (2500, 32, 12, 1)])
def test_ivf_build_exact_in_engine_arithmetic(eng, oracle, n, dim, nlist, metric):
    """hnswgpu_ivf_build against the oracle's restatement of the SAME arithmetic (f32 distances in kernel order,
    f64 means, sequential f64 D^2 sampling): identical k-means++ picks, identical assignments, bit-identical
    centroids -- at a size where f64-vs-f32 rounding would already flip the odd assignment."""
    O = oracle
    base = _data(O, n, dim, "clustered", num_clusters=9, noise_level=0.5)
    chosen, cen, assign = O.ivf_build_dev(base, nlist, 4, metric, 42)
    with eng.Index(base, metric) as idx:
        np.testing.assert_array_equal(idx.kmeanspp(nlist, 42), chosen)
        idx.ivf_build(nlist, 4, 42)
        gc, off, lids = idx.get_ivf()
        got = np.empty(n, np.int32)
        for l in range(nlist):
            got[lids[off[l]:off[l + 1]]] = l
        np.testing.assert_array_equal(got, assign)
        np.testing.assert_array_equal(gc.view(np.uint32), cen.view(np.uint32))


def test_ivf_build_soak(eng, oracle):
    """Random (n, dim, nlist, metric): the device k-means build against the restatement of its arithmetic, as above.  One
    random configuration in the default run, HNSWGPU_SOAK=<n> of them in a soak run."""
    O = oracle
    rs = np.random.RandomState(77)
    for case in range(int(os.environ.get("HNSWGPU_SOAK", "1"))):
        n = int(rs.choice([150, 900, 2600, 5000]))
        dim = int(rs.choice([3, 33, 100, 260, 768, 1000]))
        nlist = int(rs.choice([2, 9, 33, 70]))
        metric = int(rs.choice([O.COSINE, O.L2, O.DOT]))
        base = _data(O, n, dim, "clustered", num_clusters=7, noise_level=0.5, seed=600 + case)
        tag = "case %d n=%d dim=%d nlist=%d metric=%d" % (case, n, dim, nlist, metric)
        chosen, cen, assign = O.ivf_build_dev(base, nlist, 2, metric, 42)
        with eng.Index(base, metric) as idx:
            np.testing.assert_array_equal(idx.kmeanspp(nlist, 42), chosen, err_msg=tag)
            idx.ivf_build(nlist, 2, 42)
            gc, off, lids = idx.get_ivf()
            got = np.empty(n, np.int32)
            for l in range(nlist):
                got[lids[off[l]:off[l + 1]]] = l
            np.testing.assert_array_equal(got, assign, err_msg=tag)
            np.testing.assert_array_equal(gc.view(np.uint32), cen.view(np.uint32), err_msg=tag)


def test_ivf_large_batch_tiled_scan(eng, oracle):
    """nq * nprobe >= 4 * nlist: the (query, list) pairs are grouped by list and scanned by the MFMA tile
    kernel (routing included).  Bit-exact against the oracle's MFMA-order mode; groups of 32 overflow
    (one list probed by > 32 queries), empty lists, ragged list lengths."""
    O = oracle
    base = _data(O, 3000, 72, "clustered", num_clusters=5, noise_level=0.4)
    Q = _data(O, 150, 72, "clustered", num_clusters=5, noise_level=0.4, seed=43)
    for metric in (O.COSINE, O.DOT):
        with eng.Index(base, metric) as idx:
            idx.ivf_build(12, 4, 42)
            cen, off, lids = idx.get_ivf()
            for nprobe, k in [(4, 10), (12, 3), (1, 70)]:
                ids, d, pr = idx.ivf_search(Q, k, nprobe, want_probes=True)
                mode = _ivf_mode(O, metric, 72, 150, nprobe, 12)
                oi, od, opr = O.ivf_search(base, cen, off, lids, Q, k, nprobe, metric=metric, mode=mode)
                np.testing.assert_array_equal(pr, opr)
                assert_exact(ids, d, oi, od, "tiled ivf nprobe=%d metric=%d" % (nprobe, metric))
                fi, fd, _ = O.ivf_search(base, cen, off, lids, Q, k, nprobe, metric=metric)
                assert_topk_parity(ids, d, fi, fd, "tiled ivf f64", metric_scale(metric, Q, base))
            # a small batch of the same queries takes the GEMV path: same ids, distances within tolerance
            i1, d1 = idx.ivf_search(Q[:2], 10, 4)
            i2, d2 = idx.ivf_search(Q, 10, 4)
            assert_topk_parity(i1, d1, i2[:2], d2[:2], "gemv vs tile", metric_scale(metric, Q, base))


@pytest.mark.parametrize("k", [10, 100])
def test_ivf_single_query_many_partials(eng, oracle, k):
    """One query against long lists: the scan is cut into many chunks, so the per-query merge folds tens of
    thousands of partial keys with several waves (two-level merge), for k in registers (<= 64) and in LDS."""
    O = oracle
    base = _data(O, 20000, 32)
    Q = _data(O, 3, 32, seed=43)
    with eng.Index(base) as idx:
        idx.ivf_build(16, 3, 42)
        cen, off, lids = idx.get_ivf()
        for nq in (1, 3):
            ids, d = idx.ivf_search(Q[:nq], k, 16)
            oi, od, _ = O.ivf_search(base, cen, off, lids, Q[:nq], k, 16, mode=_ivf_mode(O, O.COSINE, 32, nq, 16, 16))
            assert_exact(ids, d, oi, od, "many partials nq=%d k=%d" % (nq, k))
        ei, ed = idx.exact_knn(Q[:1], k)           # probing every list == brute force (GEMV order on both sides)
        ids, d = idx.ivf_search(Q[:1], k, 16)
        assert_exact(ids, d, ei, ed, "ivf(all lists) == exact")


@pytest.mark.parametrize("nlist,n", [(3, 900), (5, 2600), (7, 5000), (13, 1300)])
def test_ivf_tile_path_small_work_lists(eng, oracle, nlist, n):
    """Few lists and few queries on the MFMA tile path: work lists of 1 .. ~40 items, i.e. not a multiple of the 8
    XCD slices the kernel deals them into (a grid that covered only `nitems` workgroups left candidates unwritten),
    several chunks per list, groups of 1 .. 9 queries, k beyond the candidate count."""
    O = oracle
    base = _data(O, n, 40)
    Q = _data(O, 20, 40, seed=43)
    with eng.Index(base) as idx:
        idx.ivf_build(nlist, 2, 42)
        cen, off, lids = idx.get_ivf()
        for nq in (2, 5, 9, 20):
            for nprobe, k in [(nlist, 10), (max(1, nlist // 2), 64), (nlist, 1000)]:
                mode = _ivf_mode(O, O.COSINE, 40, nq, nprobe, nlist)
                ids, d = idx.ivf_search(Q[:nq], k, nprobe)
                oi, od, _ = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, mode=mode)
                assert_exact(ids, d, oi, od, "nlist=%d nq=%d nprobe=%d k=%d mode=%d" % (nlist, nq, nprobe, k, mode))


@pytest.mark.parametrize("dim", [72, 300, 768, 1024, 1100])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_ivf_group_regime_keeps_gemv_bits(eng, oracle, metric, dim):
    """1.5 to 2 (query, list) pairs per list: the register-row group kernel serves the scan (ivf.hip: use_group; every
    row-loader width, and dim 1100 which is past it and stays on the GEMV scan).  Lists are read once per group instead
    of once per pair, but the summation order -- and so every bit of the result -- is the GEMV scan's."""
    O = oracle
    base = _data(O, 4000, dim, "clustered", seed=5)
    Q = _data(O, 16, dim, "clustered", seed=6)
    with eng.Index(base, ["cosine", "l2", "dot"][metric]) as idx:
        idx.ivf_build(32, 3, 42)
        cen, off, lids = idx.get_ivf()
        for nq, nprobe, k in [(12, 4, 10), (16, 4, 10), (13, 4, 200), (16, 3, 1)]:
            assert nq * nprobe <= 12 * 32                      # the GEMV-order side of the boundary
            ids, d, pr = idx.ivf_search(Q[:nq], k, nprobe, want_probes=True)
            oi, od, opr = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, metric=metric, mode=O.MODE_DEV)
            np.testing.assert_array_equal(pr, opr)
            assert_exact(ids, d, oi, od, "group regime metric=%d dim=%d nq=%d" % (metric, dim, nq))


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_ivf_many_equal_distances(eng, oracle, metric):
    """Hundreds of candidates tie on the distance bits (duplicated rows, the query among them): every top-k fold
    (register lists, LDS lists, the k-th-key bound that seeds them, the several-waves-per-query select and its
    second-level merge) must fall back on the order key exactly like the reference's stable sort
    (ivf_flat.clj:229-233,291-294).  Small and large batches: GEMV scan + partial-list merge, and tile scan + select."""
    O = oracle
    m = {"cosine": O.COSINE, "dot": O.DOT, "l2": O.L2}[metric]
    rs = np.random.RandomState(5)
    base = _data(O, 3000, 40)
    dup = rs.choice(3000, 700, replace=False)
    base[dup[:400]] = base[dup[0]]            # 400 copies of one row
    base[dup[400:]] = base[dup[400]] * 2.0    # 300 copies of another (same cosine distance as its original)
    Q = np.concatenate([base[dup[:1]], base[dup[400:401]], _data(O, 10, 40, seed=43)]).astype(np.float32)
    with eng.Index(base, metric) as idx:
        idx.ivf_build(6, 2, 42)
        cen, off, lids = idx.get_ivf()
        for nq in (1, 2, 12):
            for k in (10, 64, 500):
                mode = _ivf_mode(O, m, 40, nq, 6, 6)
                ids, d = idx.ivf_search(Q[:nq], k, 6)
                oi, od, _ = O.ivf_search(base, cen, off, lids, Q[:nq], k, 6, metric=m, mode=mode)
                assert_exact(ids, d, oi, od, "ties %s nq=%d k=%d" % (metric, nq, k))
        ei, ed = idx.exact_knn(Q, 450)
        oi, od, _ = O.exact_knn(base, Q, 450, metric=m, mode=O.MODE_DEV if (m == O.L2 or len(Q) < 16) else O.MODE_MFMA)
        assert_exact(ei, ed, oi, od, "ties exact %s" % metric)


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
@pytest.mark.parametrize("dim", [5, 300, 768, 1000, 1536, 2048, 3072])
def test_ivf_survivor_stream_every_row_width(eng, oracle, metric, dim, tune):
    """The survivor stream for every row-loader width (NCH = 1, 2, 3, 4, 6, 8, 12: 8 .. 96 MFMA steps per 32-row block, the
    operand pipeline with zero to eleven trips of its main loop), with both epilogues -- a handful of queries (one work item
    per pair), few queries per list (lane = row), many (lane = query) --, ragged lists over several tiles, exact ties and
    a zero row, without and with the half-precision pass (its row loader per width, entries appended without bounds by the
    wide epilogue): ids and distance bits equal the oracle's device-order mode."""
    O = oracle
    code = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    n = 2600
    base = _data(O, n, dim, "clustered", num_clusters=9, noise_level=0.4, seed=91)
    base[900:912] = base[4]
    base[913] = 0.0
    Q = np.concatenate([_data(O, 60, dim, "clustered", num_clusters=9, noise_level=0.4, seed=92), base[4:5]]).astype(np.float32)
    with eng.Index(base, metric) as idx:
        idx.ivf_build(7, 3, 42)
        cen, off, lids = idx.get_ivf()
        assert np.diff(off).max() > 256                           # lists of several tiles
        idx.set_profiling(True)
        for nq, nprobe, k in [(2, 4, 10), (11, 3, 10), (61, 7, 10) if metric == "l2" else (12, 7, 40)]:
            assert metric == "l2" or nq * nprobe <= 12 * 7        # the GEMV-order side of the (pinned) boundary
            oi, od, _ = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, metric=code, mode=O.MODE_DEV)
            for mid in ("0", "1"):
                tune.set("STREAM_MID", mid)
                idx.rejection_stats(reset=True)
                ids, d = idx.ivf_search(Q[:nq], k, nprobe)
                surv, cand = idx.rejection_stats(reset=True)
                assert cand > 0, "the bounds pass did not run"
                assert_exact(ids, d, oi, od, "stream %s dim=%d nq=%d nprobe=%d k=%d mid=%s" % (metric, dim, nq, nprobe, k, mid))
        idx.set_profiling(False)


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_ivf_routing_and_merge_break_ties_by_position(eng, oracle, metric, tune):
    """The probed lists and the final k are picked by bisecting the KEY space (kernels.hpp: wave_topk_sorted): the
    distance words first, then -- only when equal distances straddle the k-th place -- the positions.  Centroids in
    identical groups of eight make the nprobe-th place fall inside a tie for every query (ivf_flat.clj:266-268 sorts
    stably: the lower centroid index wins), many lists (2100 > 4 x 256: the carried chunks of the per-wave selection),
    duplicated rows put ties across the k-th result; nprobe and k from 1 to 64, one query and a batch, with and without
    the half-precision pass."""
    O = oracle
    code = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    rs = np.random.RandomState(5)
    dim, nlist, n = 136, 2100, 6300
    uniq = rs.randn(nlist // 8 + 1, dim).astype(np.float32)
    cen = np.repeat(uniq, 8, axis=0)[:nlist].copy()              # centroid c == centroid c ^ 1 == ... within its group of eight
    base = (cen[rs.randint(0, nlist, n)] + 0.05 * rs.randn(n, dim)).astype(np.float32)
    base[100:140] = base[7]                                      # forty identical rows: ties across the k-th place
    lids = rs.permutation(n).astype(np.int32)                    # rows dealt to the lists at random: three per list
    off = (np.arange(nlist + 1, dtype=np.int64) * 3)
    Q = np.concatenate([base[7:8], cen[40:41], (cen[rs.randint(0, nlist, 20)] + 0.05 * rs.randn(20, dim))]).astype(np.float32)
    with eng.Index(base, metric) as idx:
        idx.set_rejection_test(2)
        idx.set_ivf(cen, off, lids)
        tune.set("IVF_CODES", "1")
        for mid in ("0", "1"):
            tune.set("STREAM_MID", mid)
            for nq, nprobe, k in [(1, 5, 10), (1, 64, 64), (3, 1, 1), (22, 12, 33), (22, 33, 10), (5, 60, 5)]:
                if metric != "l2" and nq * nprobe > 12 * nlist:
                    continue
                ids, d, probes = idx.ivf_search(Q[:nq], k, nprobe, want_probes=True)
                oi, od, op = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, metric=code, mode=O.MODE_DEV)
                np.testing.assert_array_equal(probes, op)
                assert_exact(ids, d, oi, od, "ties %s mid=%s nq=%d nprobe=%d k=%d" % (metric, mid, nq, nprobe, k))


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_ivf_small_batch_schedules_of_round_5(eng, oracle, metric, tune):
    """Round 5's schedules of small batches, each on and off, against the oracle: the k smallest of <= 1024 keys by LDS
    histograms (kernels.hpp: topk_hist_wg -- 700 centroids of which 300 are IDENTICAL put hundreds of equal distances across
    the nprobe-th place: the candidate buffer overflows and the call bisects; groups of eight identical ones put a handful
    there), the bounds pass's work list inside the routing tail's launch (worklist_part_wg: 700 lists are not a multiple of
    the four lists a thread scans; batches of 6 = the one-launch routing, 14 and 40 = the tail launch), a key per survivor to
    the finish kernel's last workgroup (400 identical rows: more than 256 equal keys), the first threshold from half rows."""
    O = oracle
    code = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    rs = np.random.RandomState(11)
    dim, nlist, n = 136, 700, 9100
    uniq = rs.randn(nlist, dim).astype(np.float32)
    cen = uniq.copy()
    cen[100:400] = uniq[100]                                     # 300 identical centroids
    cen[400:560] = np.repeat(uniq[400:420], 8, axis=0)           # groups of eight identical ones
    base = (cen[rs.randint(0, nlist, n)] + 0.05 * rs.randn(n, dim)).astype(np.float32)
    base[1000:1400] = base[7]                                    # 400 identical rows
    lids = rs.permutation(n).astype(np.int32)
    off = (np.arange(nlist + 1, dtype=np.int64) * 13)
    Q = np.concatenate([base[7:8], cen[100:101], cen[400:401],
                        (cen[rs.randint(0, nlist, 37)] + 0.05 * rs.randn(37, dim))]).astype(np.float32)
    with eng.Index(base, metric) as idx:
        idx.set_rejection_test(2)
        idx.set_ivf(cen, off, lids)
        tune.set("IVF_CODES", "1")
        want = {}
        for nq, nprobe, k in [(1, 7, 10), (6, 64, 10), (14, 7, 64), (40, 33, 10), (40, 64, 64)]:
            want[(nq, nprobe, k)] = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, metric=code, mode=O.MODE_DEV)
        for fold, direct, half in [(1, 1024, 1), (0, 1024, 1), (1, 0, 1), (1, 1024, 0), (0, 0, 0), (1, 300, 1)]:
            tune.set("WORKLIST_FOLD", fold)
            tune.set("FINISH_DIRECT", direct)
            tune.set("SEED_HALF", half)
            for (nq, nprobe, k), (oi, od, op) in want.items():
                ids, d, probes = idx.ivf_search(Q[:nq], k, nprobe, want_probes=True)
                what = "%s fold=%d direct=%d half=%d nq=%d nprobe=%d k=%d" % (metric, fold, direct, half, nq, nprobe, k)
                np.testing.assert_array_equal(probes, op, err_msg=what)
                assert_exact(ids, d, oi, od, what)


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_ivf_wave_per_query_kernels_with_short_home_lists(eng, oracle, metric, tune):
    """The wave-per-query routing tail and home-list selection of large batches (forced here): queries whose NEAREST list
    holds fewer rows than k get their first threshold from the wave itself (the home-list pass has nothing to give them),
    next to queries with ordinary home lists and to empty lists -- probes, ids and distance bits against the oracle."""
    O = oracle
    code = {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]
    rs = np.random.RandomState(3)
    dim, nlist, n = 256, 48, 6000
    cen = rs.randn(nlist, dim).astype(np.float32)
    sizes = np.array([3] * 6 + [0] * 2 + [1] * 2 + [0] * (nlist - 10))
    rest = n - sizes.sum()
    sizes[10:] = rest // (nlist - 10)
    sizes[-1] += n - sizes.sum()
    assign = np.repeat(np.arange(nlist), sizes)
    base = (cen[assign] + 0.1 * rs.randn(n, dim)).astype(np.float32)
    off, lids = O.lists_from_assign(assign, nlist)
    Q = np.concatenate([cen[:10] + 0.01 * rs.randn(10, dim), cen[rs.randint(10, nlist, 90)] + 0.1 * rs.randn(90, dim)]).astype(np.float32)
    with eng.Index(base, metric) as idx:
        idx.set_rejection_test(2)
        idx.set_ivf(cen, off, lids)
        for key, v in (("TILE_PAIRS", 1 << 40), ("IVF_CODES", 1), ("STREAM_MID", 1), ("FINISH_ORDER", 1), ("STREAM_HOME", 1), ("QUERY_WAVES", 1)):
            tune.set(key, v)
        tw0 = eng.debug_counter("route_tail_waves")
        for nq, k, nprobe in [(100, 10, 6), (100, 2, 12), (37, 64, 20)]:
            ids, d, pr = idx.ivf_search(Q[:nq], k, nprobe, want_probes=True)
            oi, od, opr = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, metric=code, mode=O.MODE_DEV)
            what = "%s nq=%d k=%d nprobe=%d" % (metric, nq, k, nprobe)
            np.testing.assert_array_equal(pr, opr, err_msg=what)
            assert_exact(ids, d, oi, od, what)
        assert eng.debug_counter("route_tail_waves") >= tw0 + 3
        tune.set("STREAM_BUCKET", 3)       # three pairs per list's bucket: most queries overflow one and take the plain f32 scan
        for nq, k, nprobe in [(100, 10, 6), (37, 5, 20)]:
            ids, d, pr = idx.ivf_search(Q[:nq], k, nprobe, want_probes=True)
            oi, od, opr = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, metric=code, mode=O.MODE_DEV)
            np.testing.assert_array_equal(pr, opr)
            assert_exact(ids, d, oi, od, "%s tiny buckets nq=%d k=%d nprobe=%d" % (metric, nq, k, nprobe))
        tune.unset("STREAM_BUCKET")
    # 300 lists of which 200 have the SAME centroid: the nprobe-th place of the wave's selection falls inside a tie of hundreds
    nlist2 = 300
    cen2 = rs.randn(nlist2, dim).astype(np.float32)
    cen2[50:250] = cen2[50]
    assign2 = rs.randint(0, nlist2, n)
    base2 = (cen2[assign2] + 0.1 * rs.randn(n, dim)).astype(np.float32)
    off2, lids2 = O.lists_from_assign(assign2, nlist2)
    Q2 = (cen2[rs.randint(0, nlist2, 64)] + 0.1 * rs.randn(64, dim)).astype(np.float32)
    Q2[:8] = cen2[50] + 0.01 * rs.randn(8, dim).astype(np.float32)
    with eng.Index(base2, metric) as idx:
        idx.set_rejection_test(2)
        idx.set_ivf(cen2, off2, lids2)
        for nq, k, nprobe in [(64, 10, 8), (64, 10, 64)]:
            ids, d, pr = idx.ivf_search(Q2[:nq], k, nprobe, want_probes=True)
            oi, od, opr = O.ivf_search(base2, cen2, off2, lids2, Q2[:nq], k, nprobe, metric=code, mode=O.MODE_DEV)
            np.testing.assert_array_equal(pr, opr, err_msg="%s duplicated centroids nprobe=%d" % (metric, nprobe))
            assert_exact(ids, d, oi, od, "%s duplicated centroids nprobe=%d" % (metric, nprobe))


def test_ivf_randomised_small_batches(eng, oracle, tune):
    """Random IVF configurations in the regime round 5 rescheduled -- 1 to 60 queries through the survivor stream: list counts
    around and beyond the 1024 keys the histogram selection takes in one chunk, nprobe / k from 1 to 64, three metrics, rows with
    duplicates, lists of very different lengths (empty ones included) -- against the oracle's GEMV order, probes included.
    HNSWGPU_SOAK=<n>: n more seeds."""
    O = oracle
    tune.set("IVF_CODES", "1")
    for seed in [77] + [7700 + i for i in range(int(os.environ.get("HNSWGPU_SOAK", "0")))]:
        rs = np.random.RandomState(seed)
        for case in range(14):
            dim = int(rs.choice([130, 256, 768]))
            nlist = int(rs.choice([37, 300, 700, 1023, 1024, 1500]))
            n = int(rs.choice([3000, 8000]))
            metric = int(rs.choice([O.COSINE, O.L2, O.DOT]))
            cen = _data(O, nlist, dim, "gaussian", seed=seed + case)
            if rs.rand() < 0.5:
                cen[nlist // 3:nlist // 3 + min(nlist // 4, 280)] = cen[0]   # many identical centroids: equal routing distances
            w = rs.rand(nlist) ** 3                                          # a few long lists, many short or empty ones
            assign = rs.choice(nlist, n, p=w / w.sum())
            base = (cen[assign] + 0.1 * rs.randn(n, dim)).astype(np.float32)
            if rs.rand() < 0.5:
                base[rs.randint(0, n, n // 8)] = base[5]                     # hundreds of identical rows
            off, lids = O.lists_from_assign(assign, nlist)
            nq = int(rs.choice([1, 3, 6, 13, 32, 60]))
            nprobe = int(rs.choice([1, 8, 32, 64]))
            k = int(rs.choice([1, 10, 40]))
            if metric != O.L2 and nq * min(nprobe, nlist) > 12 * nlist:      # (beyond it cosine / dot take the k-ordered tile scan)
                nq = max(1, 12 * nlist // min(nprobe, nlist))
            Q = np.vstack([base[5:6], (cen[rs.randint(0, nlist, nq)] + 0.1 * rs.randn(nq, dim))]).astype(np.float32)[:nq]
            tag = "seed %d case %d dim=%d nlist=%d n=%d metric=%d nq=%d nprobe=%d k=%d" % (seed, case, dim, nlist, n, metric, nq, nprobe, k)
            with eng.Index(base, metric) as idx:
                idx.set_rejection_test(2)
                idx.set_ivf(cen, off, lids)
                ids, d, pr = idx.ivf_search(Q, k, nprobe, want_probes=True)
                oi, od, opr = O.ivf_search(base, cen, off, lids, Q, k, nprobe, metric=metric, mode=O.MODE_DEV)
                np.testing.assert_array_equal(pr[:, :min(nprobe, nlist)], opr, err_msg=tag)
                assert_exact(ids, d, oi, od, tag)


@pytest.mark.parametrize("kind", ["gaussian", "clustered"])
def test_ivf_calibration_keeps_the_stream_for_data_it_helps(eng, oracle, kind):
    """Mode 1 (the default outside this suite) measures once per set of lists what the int8 bounds separate on the
    handle's rows (ivf.hip: ivf_calibrate): on i.i.d. gaussian rows every candidate lies within the bounds' width of the
    k-th -- the stream would be the f32 scan behind a wasted bounds pass -- and the handle takes the f32 paths from
    then on; on clustered rows the stream stays.  Either way the results are the oracle's; mode 2 forces the stream, and
    setting the mode measures again."""
    O = oracle
    rs = np.random.RandomState(21)
    n, dim, nlist, nprobe, k = 12_000, 768, 16, 8, 10
    if kind == "gaussian":
        base = rs.randn(n, dim).astype(np.float32)
        Q = rs.randn(40, dim).astype(np.float32)
    else:
        cen = rs.randn(nlist, dim).astype(np.float32)
        base = (cen[rs.randint(0, nlist, n)] + 0.3 * rs.randn(n, dim)).astype(np.float32)
        Q = (cen[rs.randint(0, nlist, 40)] + 0.3 * rs.randn(40, dim)).astype(np.float32)
    with eng.Index(base, "l2") as idx:
        idx.ivf_build(nlist, 3, 42)
        cen_, off, lids = idx.get_ivf()
        oi, od, _ = O.ivf_search(base, cen_, off, lids, Q, k, nprobe, metric=O.L2, mode=O.MODE_DEV)
        idx.set_profiling(True)
        for mode, expect_stream in [(1, kind == "clustered"), (2, True), (1, kind == "clustered")]:
            idx.set_rejection_test(mode)
            for rep in range(2):                               # the first search of a mode-1 handle calibrates
                idx.rejection_stats(reset=True)
                ids, d = idx.ivf_search(Q, k, nprobe)
                surv, cand = idx.rejection_stats(reset=True)
                assert_exact(ids, d, oi, od, "%s mode %d rep %d" % (kind, mode, rep))
                assert (cand > 0) == expect_stream, (kind, mode, rep, surv, cand)
        idx.set_profiling(False)


@pytest.mark.parametrize("kind", ["gaussian", "clustered"])
def test_ivf_stream_equals_the_f32_scan_at_scale(eng, kind):
    """A size-independent property at a size the oracle does not reach: the Euclidean IVF search has ONE arithmetic, so the
    survivor stream (int8 bounds, half-precision pass, compaction, ordered queries: a batch of 700 over 150k rows) must
    return exactly what the plain f32 scans return with the compact copies switched off -- on clustered rows, where the
    bounds leave a handful of candidates, and on i.i.d. gaussian rows, where distances concentrate and they leave many."""
    rs = np.random.RandomState(11)
    n, dim, nlist, nprobe, nq, k = 150_000, 160, 128, 16, 700, 10
    if kind == "gaussian":
        base = rs.randn(n, dim).astype(np.float32)
        Q = rs.randn(nq, dim).astype(np.float32)
    else:
        cen = rs.randn(nlist, dim).astype(np.float32)
        base = (cen[rs.randint(0, nlist, n)] + 0.3 * rs.randn(n, dim)).astype(np.float32)
        Q = (cen[rs.randint(0, nlist, nq)] + 0.3 * rs.randn(nq, dim)).astype(np.float32)
    with eng.Index(base, "l2") as idx:
        idx.ivf_build(nlist, 3, 42)
        idx.set_profiling(True)
        got = {}
        for mode in (2, 0):
            idx.set_rejection_test(mode)
            idx.rejection_stats(reset=True)
            got[mode] = idx.ivf_search(Q, k, nprobe)
            surv, cand = idx.rejection_stats(reset=True)
            assert (cand > 0) == (mode == 2)
        idx.set_profiling(False)
        np.testing.assert_array_equal(got[2][0], got[0][0])
        np.testing.assert_array_equal(got[2][1].view(np.uint32), got[0][1].view(np.uint32))
        assert (got[2][0] >= 0).all() and (np.diff(got[2][1], axis=1) >= 0).all()


@pytest.mark.parametrize("dim", [900, 1536, 2500])
def test_ivf_tile_path_several_k_phases(eng, oracle, dim):
    """Rows longer than 896 floats: the query group is resident in LDS one 768-column phase at a time and is refilled
    per tile and phase (2 / 2 / 4 phases here, the last one short and odd), with the tile's accumulators carried
    across the phases.  Lists of several tiles with ragged ends, groups of 1 .. 32 queries, all on the MFMA tile path."""
    O = oracle
    base = _data(O, 2300, dim)
    Q = _data(O, 70, dim, seed=43)
    with eng.Index(base) as idx:
        idx.ivf_build(5, 2, 42)
        cen, off, lids = idx.get_ivf()
        for nq, nprobe, k in [(70, 5, 10), (33, 2, 40), (13, 5, 3)]:
            mode = _ivf_mode(O, O.COSINE, dim, nq, nprobe, 5)
            assert mode == O.MODE_MFMA
            ids, d = idx.ivf_search(Q[:nq], k, nprobe)
            oi, od, _ = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, mode=mode)
            assert_exact(ids, d, oi, od, "dim=%d nq=%d nprobe=%d k=%d" % (dim, nq, nprobe, k))


@pytest.mark.parametrize("dim", [7, 100, 300, 768, 1000, 1100])
def test_l2_batched_group_scan(eng, oracle, dim):
    """Euclidean metric, batches large enough for the group path: the query group resident in LDS, rows in registers
    (l2_group_kernel, dim <= 1024; dim 1100 stays on the GEMV scan).  Same arithmetic as the GEMV kernel, so every
    result equals the oracle's device-order mode bit for bit: exact kNN, k-means assignment (fused argmin), dense
    distances and IVF search over ragged multi-chunk lists."""
    O = oracle
    base = _data(O, 2100, dim)
    base[40:60] = base[40]                                     # exact zeros and ties
    Q = np.vstack([_data(O, 38, dim, seed=43), base[40:42]]).astype(np.float32)
    with eng.Index(base, "l2") as idx:
        ei, ed = idx.exact_knn(Q, 12)
        oi, od, _ = O.exact_knn(base, Q, 12, metric=O.L2, mode=O.MODE_DEV)
        assert_exact(ei, ed, oi, od, "l2 exact dim=%d" % dim)
        assert ed[38, 0] == 0.0 and ed[39, 0] == 0.0             # d(x, x) = 0 exactly (core_test.clj:9-31)
        cen = _data(O, 45, dim, seed=5)
        a, ad = idx.kmeans_assign(cen)
        oa, oad = O.kmeans_assign_f32(base, cen, O.L2, O.MODE_DEV)
        np.testing.assert_array_equal(a, oa)
        np.testing.assert_array_equal(ad.view(np.uint32), oad.view(np.uint32))
        dd = idx.dense_distances(Q[:20])
        want = _dense_oracle(O, base, Q[:20], O.L2, O.MODE_DEV)
        np.testing.assert_array_equal(dd.view(np.uint32), want.astype(np.float32).view(np.uint32))
        idx.ivf_build(6, 2, 42)
        cen, off, lids = idx.get_ivf()
        for nq, nprobe, k in [(40, 6, 10), (17, 3, 64), (5, 6, 200)]:
            ids, d = idx.ivf_search(Q[:nq], k, nprobe)
            oi, od, _ = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, metric=O.L2, mode=O.MODE_DEV)
            assert_exact(ids, d, oi, od, "l2 ivf dim=%d nq=%d nprobe=%d k=%d" % (dim, nq, nprobe, k))


def test_ivf_many_lists_many_probes(eng, oracle):
    """300 lists, 70 .. 300 probes per query: centroid routing selects more than 64 centroids (top-k lists in LDS
    instead of registers, dense routing + select for small batches, tile routing for large ones), hundreds of
    (query, list) pairs per query run in list order."""
    O = oracle
    base = _data(O, 6000, 16, "clustered", num_clusters=12, noise_level=0.5)
    Q = _data(O, 33, 16, seed=43)
    with eng.Index(base) as idx:
        idx.ivf_build(300, 2, 42)
        cen, off, lids = idx.get_ivf()
        for nq, nprobe, k in [(2, 70, 10), (2, 300, 100), (33, 128, 10), (33, 300, 5)]:
            mode = _ivf_mode(O, O.COSINE, 16, nq, nprobe, 300)
            ids, d, pr = idx.ivf_search(Q[:nq], k, nprobe, want_probes=True)
            oi, od, opr = O.ivf_search(base, cen, off, lids, Q[:nq], k, nprobe, mode=mode)
            np.testing.assert_array_equal(pr, opr, err_msg="probes nq=%d nprobe=%d" % (nq, nprobe))
            assert_exact(ids, d, oi, od, "many lists nq=%d nprobe=%d k=%d mode=%d" % (nq, nprobe, k, mode))


def test_ivf_ragged_lists_and_full_probe(eng, oracle):
    """Empty lists, a list holding almost everything, nprobe > nlist, k > candidates."""
    O = oracle
    base = _data(O, 700, 48)
    Q = _data(O, 10, 48, seed=43)
    rs = np.random.RandomState(3)
    assign = np.where(rs.rand(700) < 0.8, 2, rs.randint(0, 9, 700))   # list 2 is huge
    assign[assign == 5] = 6                                          # list 5 is empty
    cen = _data(O, 9, 48, seed=99)
    off, lids = O.lists_from_assign(assign, 9)
    with eng.Index(base) as idx:
        idx.set_ivf(cen, off, lids)
        for nprobe, k in [(1, 5), (3, 10), (9, 10), (50, 10), (2, 300)]:
            ids, d = idx.ivf_search(Q, k, nprobe)
            oi, od, _ = O.ivf_search(base, cen, off, lids, Q, k, nprobe, mode=_ivf_mode(O, O.COSINE, 48, len(Q), nprobe, 9))
            assert_exact(ids, d, oi, od, "ragged nprobe=%d k=%d" % (nprobe, k))
        # probing every list == exact kNN (size-independent property)
        ids, d = idx.ivf_search(Q, 10, 9)
        ei, ed = idx.exact_knn(Q, 10)
        np.testing.assert_array_equal(np.sort(ids, 1), np.sort(ei, 1))
        with pytest.raises(Exception, match="two lists"):
            idx.set_ivf(cen, off, np.zeros_like(lids))


# ---- BASELINE.json full-size shapes: size-independent properties --------------------------------------------
def test_full_size_31k_properties(eng, oracle):
    """31,173 x 768 (configs[0]/[1]): sortedness, idempotence, self-match, GPU brute force as ground
    truth for recall, IVF(all lists) == exact."""
    from hnsw_clj_amd import datagen

    base = datagen.generate_dataset(31173, 768)
    Q = np.vstack([base[:100], datagen.generate_dataset(100, 768, seed=43)])
    with eng.Index(base) as idx:
        ei, ed = idx.exact_knn(Q, 10)
        assert (ei[:100, 0] == np.arange(100)).all() and (np.abs(ed[:100, 0]) < 1e-5).all()
        assert (np.diff(ed, axis=1) >= 0).all()
        idx.hnsw_build(16, 200, 42)
        ids, d, st = idx.hnsw_search(Q, 10, 200, want_stats=True)
        ids2, d2 = idx.hnsw_search(Q, 10, 200)
        assert np.array_equal(ids, ids2) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))
        assert (np.diff(d, axis=1) >= 0).all() and (ids >= 0).all() and (ids < 31173).all()
        assert all(len(set(r.tolist())) == 10 for r in ids)
        assert (ids[:100, 0] == np.arange(100)).all()
        # every returned distance is the true distance of that id
        for q in (0, 57, 150):
            np.testing.assert_array_equal(idx.batch_distances(Q[q], ids[q]).view(np.uint32), d[q].view(np.uint32))
        # i.i.d. gaussian in 768-d is the hardest case for any graph index: the reference-structure
        # graph built by the oracle reaches 0.80 here at ef=200 ("Datasets and recall")
        assert oracle.recall(ids[:100], ei[:100]) >= 0.75
        assert st[:, 0].min() > 200 and st[:, 1].min() >= 200
        idx.ivf_build(24, 2, 42)   # the reference's default nlist (ivf_flat.clj:144); 2 Lloyd passes keep it short
        ii, dd = idx.ivf_search(Q, 10, 24)
        # the list scan (GEMV order) and the brute force (MFMA tile order) sum in different orders
        assert_topk_parity(ii, dd, ei, ed, "ivf(all lists) vs exact")


@pytest.mark.parametrize("dist,builder,ef,nsub", [("clustered", "heuristic", 640, 48), ("manifold", "ultra_fast.clj", 100, 64),
                                                  ("gaussian", "graph.clj", 2400, 24), ("uniform01", "heuristic", 3200, 16)])
def test_timed_launch_configurations_against_oracle(eng, oracle, dist, builder, ef, nsub):
    """The launches bench.py times, under the oracle: bench.make_31k's 31,173 x 768 sets, the graph built on the
    device by bench.py's builders, 4,096 held-out queries in ONE launch with the DEFAULT rejection mode -- the int8
    rejection test on, waves per query by the LDS residency rule, the in-place merge of a long list -- at the headline's
    operating point (S1's clustered set, heuristic builder, ef 640), at round 3's (manifold, closest-m, ef 100) and at the ef
    the i.i.d. sets need (2400 / 3200: lists of thousands of entries, two and four waves per query).
    A subsample of the batch: ids, distance bits and both traversal counters equal the oracle's device-order mode; ids and
    distances agree with its f64 reference-order mode within the north_star's tolerance (ultra_fast.clj:151-212, 346-374)."""
    import bench

    O = oracle
    base = bench.make_31k(dist, 42, bench.N31K)
    Q = bench.make_31k(dist, 43, 4096)
    with eng.Index(base, "cosine") as idx:
        idx.set_rejection_test(1)                 # the default of a new handle outside the test processes
        idx.hnsw_build(bench.M, bench.EFC, 42, **bench.BUILDERS[builder])
        g = idx.get_graph()
        idx.set_profiling(True)
        idx.rejection_stats(reset=True)
        ids, d, st = idx.hnsw_search(Q, 10, ef, want_stats=True)
        f32_rows, neighbours = idx.rejection_stats(reset=True)
        idx.set_profiling(False)
        # (on the clustered set's seed-43 queries the bounds reject about half of the neighbours, on the others 80 - 85 %)
        assert 0 < f32_rows < 0.7 * neighbours, "the rejection test did not run on the timed configuration"
        sub = np.linspace(0, len(Q) - 1, nsub).astype(np.int64)
        oi, od, ost, _ = O.hnsw_search(base, g, Q[sub], 10, ef=ef, mode=O.MODE_DEV, nthreads=8)
        assert_exact(ids[sub], d[sub], oi, od, "%s ef %d vs oracle (device order)" % (dist, ef))
        np.testing.assert_array_equal(st[sub], ost)
        fi, fd, _, _ = O.hnsw_search(base, g, Q[sub[:16]], 10, ef=ef, nthreads=8)
        assert_topk_parity(ids[sub[:16]], d[sub[:16]], fi, fd, "%s ef %d vs oracle (f64 reference order)" % (dist, ef))


def test_hnsw_add_keeps_the_builder_of_the_graph(eng, oracle):
    """hnswgpu_hnsw_add inserts with the options the handle's graph was built with: rows added to a graph built by the
    heuristic builder (graph.clj:162-232) are linked by the heuristic too -- the grown graph passes the validator, its
    search equals the oracle's on the export, and clustered rows stay reachable (closest-m links would not reach them)."""
    O = oracle
    n0, n1, dim = 6000, 7000, 64
    base = O.generate_dataset(n1, dim, "clustered", num_clusters=40, noise_level=0.3).astype(np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    Q = base[n0:n0 + 200] + 0.01
    with eng.Index(base[:n0]) as idx:
        idx.hnsw_build(16, 100, 42, heuristic=True)
        idx.hnsw_add(base[n0:n0 + 300], 100, 42)
        idx.hnsw_add(base[n0 + 300:], 100, 42)
        assert idx.n == n1
        g = idx.get_graph()
        deg = (g.l0_adj.reshape(n1, -1) >= 0).sum(1)
        assert deg.min() >= 1 and deg.mean() < 31, "heuristic lists are not full: mean degree %.1f" % deg.mean()
        ids, d, st = idx.hnsw_search(Q, 10, 200, want_stats=True)
        oi, od, ost, _ = O.hnsw_search(base, g, Q, 10, ef=200, mode=O.MODE_DEV)
        assert_exact(ids, d, oi, od, "search of the grown heuristic graph vs oracle")
        np.testing.assert_array_equal(st, ost)
        ex, _ = idx.exact_knn(Q, 10)
        assert O.recall(ids, ex) > 0.9
        with eng.Index(base) as chk:
            chk.set_graph(g)


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_hnsw_add_to_a_live_index(eng, oracle, metric):
    """insert-single on a live index (ultra_fast.clj:216-275; add-vector!, api.clj:30-33): a graph built over 20,000 rows
    takes 4,000 more in calls of 1, 64 and 1,024 rows.  The grown graph is a valid graph (a fresh handle accepts it through
    hnswgpu_set_graph's validation), the device search of it equals the oracle's search of the exported graph (ids,
    distance bits, counters), the new rows find themselves, levels continue the build's seeded sequence, and recall stays
    within 0.02 of a from-scratch build over all 24,000 rows."""
    O = oracle
    m = O.METRICS[metric]
    n0, n1, dim, ef = 20_000, 24_000, 64, 120
    base = O.generate_dataset(n1, dim, "clustered", num_clusters=60, noise_level=0.6).astype(np.float32)
    Q = O.generate_dataset(200, dim, "clustered", num_clusters=60, noise_level=0.6, seed=43).astype(np.float32)
    with eng.Index(base, metric) as full:
        full.hnsw_build(16, 200, 42)
        gfull = full.get_graph()
        ti, _ = full.exact_knn(Q, 10)
        fi, _ = full.hnsw_search(Q, 10, ef)
        rec_full = O.recall(fi, ti)
        si, _ = full.hnsw_search(base[n0:n0 + 300], 1, ef)
        self_full = float((si[:, 0] == np.arange(n0, n0 + 300)).mean())
    with eng.Index(base[:n0], metric) as idx:
        idx.hnsw_build(16, 200, 42)
        pos = n0
        for step in [1] * 8 + [64] * 6 + [1024] * 3 + [n1]:      # calls of 1, 64, 1024 rows, then the rest
            take = min(step, n1 - pos)
            ids = idx.hnsw_add(base[pos:pos + take], 200, 42)
            assert ids[0] == pos and len(ids) == take
            pos += take
        assert idx.n == n1 and pos == n1
        g = idx.get_graph()
        np.testing.assert_array_equal(g.levels, gfull.levels)       # the same java.util.Random(42) draws, row by row
        ids, d, st = idx.hnsw_search(Q, 10, ef, want_stats=True)
        oi, od, ost, _ = O.hnsw_search(base, g, Q, 10, ef=ef, metric=m, mode=O.MODE_DEV, nthreads=8)
        assert_exact(ids, d, oi, od, "search of the grown graph vs oracle")
        np.testing.assert_array_equal(st, ost)
        si, sd = idx.hnsw_search(base[n0:n0 + 300], 1, ef)          # the added rows are reachable: they find themselves
        self_add = float((si[:, 0] == np.arange(n0, n0 + 300)).mean())   # ... as often as in the from-scratch graph
        assert self_add >= self_full - 0.05, (self_add, self_full)
        rec = O.recall(ids, ti)
        assert rec >= rec_full - 0.02, (rec, rec_full)
        with eng.Index(base, metric) as chk:                        # the validator: a fresh handle installs the export
            chk.set_graph(g)
            ci, cd = chk.hnsw_search(Q[:20], 10, ef)
            np.testing.assert_array_equal(ci, ids[:20])
        with pytest.raises(Exception, match="IVF"):                 # lists cover the rows they were built over
            idx.ivf_build(8, 2, 42)
            idx.hnsw_add(base[:1], 200, 42)


def test_device_build_vs_reference_structure_on_clustered_data(eng, oracle):
    """The batched device build (nodes of a batch do not see each other) against the oracle's sequential
    reference-structure build (orc_hnsw_build, ultra_fast.clj:216-299) where it matters most: 31,173 x 128 clustered
    (256 centres, noise 0.3, normalised), the shape on which closest-m pruning without a diversity heuristic
    (:279-299) leaves the graph disconnected between clusters.  Both graphs searched by the same device kernel at equal
    ef: the device-built graph may not be worse by more than 0.03 recall@10 (measured: 0.042 against 0.011 -- both
    low, the batched build the better of the two; profiles/r03_build_compare_clustered_31k.txt)."""
    O = oracle
    n, dim, ncl = 31173, 128, 256
    base = O.generate_dataset(n, dim, "clustered", num_clusters=ncl, noise_level=0.3).astype(np.float64)
    base = (base / np.linalg.norm(base, axis=1, keepdims=True)).astype(np.float32)
    Q = O.generate_dataset(400, dim, "clustered", num_clusters=ncl, noise_level=0.3, seed=43).astype(np.float64)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    gref = O.hnsw_build(base, O.COSINE, 16, 200, seed=42)
    with eng.Index(base, "cosine") as idx:
        ti, _ = idx.exact_knn(Q, 10)
        idx.hnsw_build(16, 200, 42)
        dev = {ef: O.recall(idx.hnsw_search(Q, 10, ef)[0], ti) for ef in (50, 200)}
        idx.set_graph(gref)
        for ef in (50, 200):
            ids, d, st = idx.hnsw_search(Q, 10, ef, want_stats=True)
            ref = O.recall(ids, ti)
            assert dev[ef] >= ref - 0.03, (ef, dev[ef], ref)
            if ef == 50:      # ... and the device searches the reference-structure graph as the oracle does
                oi, od, ost, _ = O.hnsw_search(base, gref, Q[:64], 10, ef=ef, mode=O.MODE_DEV, nthreads=8)
                assert_exact(ids[:64], d[:64], oi, od, "reference-structure graph, clustered")
                np.testing.assert_array_equal(st[:64], ost)


def test_persistence_and_lightning(eng, oracle, tmp_path):
    """Binary index file (replaces helper/index_io.clj's EDN): save -> load gives the same ids and the same
    bits; damaged files are rejected.  Lightning partitions reuse the list-scan kernel."""
    from hnsw_clj_amd import datagen, index_io, ivf_flat, lightning, ultra_fast

    vecs = datagen.generate_dataset(600, 40)
    data = datagen.indexed(vecs)
    g = ultra_fast.build_index(data, show_progress=False)
    path = str(tmp_path / "index.bin")
    index_io.save_index(g, path)
    assert index_io.index_exists(path) and os.path.getsize(path) < 600 * (40 * 4 + 33 * 4 + 200)
    g2 = index_io.load_index(path, ultra_fast.cosine_distance_ultra)
    for q in vecs[:5]:
        assert ultra_fast.search_knn(g, q, 7) == ultra_fast.search_knn(g2, q, 7)      # integration_test.clj:68-78 intent
    assert index_io.load_index(str(tmp_path / "nope.bin"), ultra_fast.cosine_distance_ultra) is None
    with pytest.raises(ValueError, match="metric"):
        index_io.load_index(path, ultra_fast.euclidean_distance_ultra)
    raw = bytearray(open(path, "rb").read())
    sec = index_file.section_offsets(index_file.unpack_header(raw))                    # the layout: tests/index_file.py
    assert (sec["base"], sec["levels"], sec["l0_adj"]) == (64, 64 + 600 * 40 * 4, 64 + 600 * 40 * 4 + 600 * 4)
    raw[sec["l0_adj"] + 8] = 0x7f                                                     # an edge pointing far outside
    raw[sec["l0_adj"] + 11] = 0x7f
    open(str(tmp_path / "bad.bin"), "wb").write(raw)
    with pytest.raises(Exception, match="out of range"):
        eng.Index.load(str(tmp_path / "bad.bin"))
    with pytest.raises(Exception, match="truncated"):
        open(str(tmp_path / "short.bin"), "wb").write(raw[:5000])
        eng.Index.load(str(tmp_path / "short.bin"))
    # the header's up_blocks and the body's up_off must describe the same array (set_graph indexes one with the other)
    raw = bytearray(open(path, "rb").read())
    upoff_end = sec["up_adj"] - 8                                                     # up_off[n], the last of n + 1 offsets
    assert upoff_end == 64 + 600 * 40 * 4 + 600 * 4 + 600 * 32 * 4 + 600 * 8
    raw[upoff_end:upoff_end + 8] = (10 ** 9).to_bytes(8, "little")
    open(str(tmp_path / "upoff.bin"), "wb").write(raw)
    with pytest.raises(Exception, match="up_off"):
        eng.Index.load(str(tmp_path / "upoff.bin"))
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]           # saved beside, renamed over
    with pytest.raises(Exception, match="cannot open"):
        g.index.save(str(tmp_path / "no_such_dir" / "x.bin"))
    g.close(), g2.close()
    ivf = ivf_flat.build_index(data, num_partitions=6, show_progress=False)
    index_io.save_index(ivf, path)
    ivf2 = index_io.load_index(path)
    assert ivf_flat.search_knn(ivf, vecs[3], 5, "precise") == ivf_flat.search_knn(ivf2, vecs[3], 5, "precise")
    ivf.close(), ivf2.close()
    li = lightning.build_index(data, num_partitions=24, show_progress=False, seed=1)
    _, off, lids = li.index.get_ivf()
    assert np.diff(off).max() == 25 and sorted(lids.tolist()) == list(range(600))     # equal random slices
    r = lightning.search_knn(li, vecs[9], 3, "precise")
    assert len(r) == 3 and all(len(x) == 2 for x in r)
    full = lightning.search_lightning(li, vecs[9], 3, search_percent=1.0)
    assert full[0][0] == "vec_9" and abs(full[0][1]) < 1e-6
    cen = li.index.list_means(off, lids)
    want = np.stack([vecs[lids[off[l]:off[l + 1]]].astype(np.float64).mean(0) for l in range(24)])
    assert np.allclose(cen, want, rtol=1e-6, atol=1e-7)
    li.close()


def test_concurrent_searches_from_host_threads(eng, oracle):
    """core_test.clj:112-121: 20 concurrent searches on one index all return 10 results -- here from 20 host
    threads through the C ABI (ctypes drops the GIL), and every result equals the serial one."""
    import threading

    O = oracle
    base = _data(O, 3000, 64)
    Q = _data(O, 20, 64, seed=43)
    with eng.Index(base) as idx:
        idx.hnsw_build(16, 100, 42)
        idx.ivf_build(8, 2, 42)
        want_h = [idx.hnsw_search(q, 10, 64) for q in Q]
        want_i = [idx.ivf_search(q, 10, 4) for q in Q]
        got_h, got_i, errs = [None] * 20, [None] * 20, []

        def work(t):
            try:
                for _ in range(5):
                    got_h[t] = idx.hnsw_search(Q[t], 10, 64)
                    got_i[t] = idx.ivf_search(Q[t], 10, 4)
            except Exception as e:  # pragma: no cover
                errs.append(e)

        th = [threading.Thread(target=work, args=(t,)) for t in range(20)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert not errs
        for t in range(20):
            assert (got_h[t][0] >= 0).sum() == 10
            assert np.array_equal(got_h[t][0], want_h[t][0]) and np.array_equal(got_h[t][1], want_h[t][1])
            assert np.array_equal(got_i[t][0], want_i[t][0]) and np.array_equal(got_i[t][1], want_i[t][1])


def test_concurrent_ivf_callers_with_mixed_nprobe_keep_their_bits(eng, oracle):
    """The combiner must serve every caller with the kernel it would get alone, whoever leads the batch: a thread asking
    for nprobe 1 beside threads asking for nprobe 32 (which, combined without care, cross the GEMV -> MFMA boundary of
    2 pairs per list) -- every result bit-equal to the same call made alone."""
    import threading

    O = oracle
    base = _data(O, 6000, 48, "clustered", num_clusters=8, noise_level=0.5)
    Q = _data(O, 48, 48, "clustered", num_clusters=8, noise_level=0.5, seed=43)
    with eng.Index(base) as idx:
        idx.ivf_build(64, 2, 42)
        probes = [1 if t % 6 == 0 else 32 for t in range(48)]           # 40 x 32 pairs >> 2 x 64 lists when combined
        want = [idx.ivf_search(Q[t], 10, probes[t]) for t in range(48)]
        got, errs = [None] * 48, []

        def work(t):
            try:
                for _ in range(8):
                    got[t] = idx.ivf_search(Q[t], 10, probes[t])
            except Exception as e:  # pragma: no cover
                errs.append(e)

        th = [threading.Thread(target=work, args=(t,)) for t in range(48)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert not errs
        for t in range(48):
            assert np.array_equal(got[t][0], want[t][0]), "thread %d (nprobe %d): ids" % (t, probes[t])
            assert np.array_equal(got[t][1].view(np.uint32), want[t][1].view(np.uint32)), "thread %d: distance bits" % t


def test_full_size_ivf_1m_properties(eng):
    """BASELINE.json configs[2] at full size (1M x 768, nlist 1024, nprobe 32): size-independent properties.
    Sorted output, idempotence, ids valid and unique, returned distances are the rows' true distances, probing
    every list reproduces GPU brute force, both scan kernels (GEMV for small batches, MFMA tiles for large) agree
    within tolerance, lists partition the rows, recall of the configuration."""
    import torch

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    n, nlist = 1_000_000, 1024
    cen = torch.randn(nlist, 768, generator=g, device=dev)
    x = cen[torch.randint(0, nlist, (n,), generator=g, device=dev)] + 0.3 * torch.randn(n, 768, generator=g, device=dev)
    x /= x.norm(dim=1, keepdim=True)
    Q = (x[:160] + 0.05 * torch.randn(160, 768, generator=g, device=dev))
    Q = (Q / Q.norm(dim=1, keepdim=True)).contiguous()
    with eng.Index(x, "cosine") as idx:
        idx.ivf_build(nlist, 3, 42)
        _, off, lids = idx.get_ivf()
        assert off[0] == 0 and off[-1] == n and np.array_equal(np.sort(lids), np.arange(n, dtype=np.int32))
        big_i, big_d = idx.ivf_search_dev(Q, 10, 32)                       # 160 * 32 >= 4 * 1024: MFMA tile path
        big_i2, big_d2 = idx.ivf_search_dev(Q, 10, 32)
        torch.cuda.synchronize()
        assert torch.equal(big_i, big_i2) and torch.equal(big_d, big_d2)
        bi, bd = big_i.cpu().numpy(), big_d.cpu().numpy()
        assert (np.diff(bd, axis=1) >= 0).all() and (bi >= 0).all() and (bi < n).all()
        assert all(len(set(r.tolist())) == 10 for r in bi)
        small_i, small_d = idx.ivf_search_dev(Q[:8].contiguous(), 10, 32)  # GEMV path
        torch.cuda.synchronize()
        assert_topk_parity(small_i.cpu().numpy(), small_d.cpu().numpy(), bi[:8], bd[:8], "gemv vs tile at 1M")
        qh = Q.cpu().numpy()
        for r in (0, 77):
            true = idx.batch_distances(qh[r], bi[r])
            assert close(bd[r], true).all()
        ei, ed = idx.exact_knn_dev(Q[:32].contiguous(), 10)
        torch.cuda.synchronize()
        ei, ed = ei.cpu().numpy(), ed.cpu().numpy()
        hit = np.mean([len(set(bi[r]) & set(ei[r])) / 10 for r in range(32)])
        assert hit >= 0.95, hit
        ai, ad = idx.ivf_search(qh[:2], 10, nlist)                         # every list probed == brute force
        assert_topk_parity(ai, ad, ei[:2], ed[:2], "ivf(all lists) vs exact at 1M")


def test_c_abi_from_plain_c(native_lib, oracle, tmp_path):
    """examples/abi_demo.c: the library used the way a JNI / Panama binding uses it -- from C, without Python or
    torch in the process.  Its last part walks INTEGRATION.md section 5 (a graph held as per-node, per-level neighbour
    SETS is flattened and served through hnswgpu_set_graph); the migrated index and its answers are written out, and
    the CPU oracle must give the same answers on that very graph: ids, distance bits, traversal counters."""
    import subprocess

    O = oracle
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "abi_demo")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "abi_demo.c"),
                           "-L" + native_lib.PKG, "-lhnswgpu", "-Wl,-rpath," + native_lib.PKG, "-lm", "-o", exe])
    mig, res = str(tmp_path / "migrated.bin"), str(tmp_path / "results.bin")
    out = subprocess.run([exe, str(tmp_path / "demo.bin"), mig, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "abi_demo ok" in out.stdout
    # the flat index file (layout: hnsw-clj_amd/csrc/persist.hip): header, base, levels, l0_adj, up_off, up_adj
    f = index_file.read_index_file(mig)                       # (refuses a file whose size is not what its header implies)
    n, dim, flags, M, M0, entry, max_level = (f[key] for key in ("n", "dim", "flags", "M", "M0", "entry", "max_level"))
    assert f["magic"] == b"HNSWGPU1" and flags == 1 and (n, dim, M, M0) == (2000, 96, 16, 32)
    base, levels, l0, up_off, up = (f[key] for key in ("base", "levels", "l0_adj", "up_off", "up_adj"))
    assert f["size"] == 64 + 4 * n * dim + 4 * n + 4 * n * M0 + 8 * (n + 1) + 4 * f["up_blocks"] * M
    r = open(res, "rb").read()
    ids = np.frombuffer(r, np.int32, 40, 0).reshape(8, 5)
    d = np.frombuffer(r, np.float32, 40, 160).reshape(8, 5)
    st = np.frombuffer(r, np.int64, 16, 320).reshape(8, 2)
    og = O.Graph(levels, l0, up_off, up, M, entry, max_level)
    oi, od, ost, _ = O.hnsw_search(base, og, base[100:108], 5, ef=64, mode=O.MODE_DEV)
    assert_exact(ids, d, oi, od, "set_graph migration from C vs oracle")
    np.testing.assert_array_equal(st, ost)


def test_parallel_callers_from_plain_c(native_lib, tmp_path):
    """examples/parallel_callers.c: the reference's throughput protocol (helper/parallel_search.clj:15-49) -- 1 .. 200
    threads of single-query hnswgpu_hnsw_search calls on one handle.  The library combines concurrent callers into one
    launch; the program fails unless every thread count returns exactly the ids of one big batch."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "parallel_callers")
    subprocess.check_call(["gcc", "-O2", "-pthread", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "parallel_callers.c"), "-L" + native_lib.PKG, "-lhnswgpu",
                           "-Wl,-rpath," + native_lib.PKG, "-lm", "-o", exe])
    out = subprocess.run([exe, "6000", "64", "60"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "parallel_callers ok" in out.stdout and "DIFFER" not in out.stdout


def test_merge_topk_dev(eng):
    import torch

    rs = np.random.RandomState(0)
    ns, nq, k = 4, 37, 10
    d = np.sort(rs.rand(ns, nq, k).astype(np.float32), axis=2)
    ids = rs.randint(0, 1 << 30, (ns, nq, k)).astype(np.int32)
    ids[1, :, 7:] = -1
    d[1, :, 7:] = np.inf
    d[2, 5, 0] = d[0, 5, 0]                        # a cross-shard tie: lower shard first
    oi, od = eng.merge_topk_dev(torch.from_numpy(ids).cuda(), torch.from_numpy(d).cuda())
    oi, od = oi.cpu().numpy(), od.cpu().numpy()
    for q in range(nq):
        flat = [(d[s, q, r], s * k + r, ids[s, q, r]) for s in range(ns) for r in range(k) if ids[s, q, r] >= 0]
        flat.sort()
        assert [x[2] for x in flat[:k]] == oi[q].tolist()
        assert np.array_equal(np.array([x[0] for x in flat[:k]], np.float32), od[q])


# ---- the Python mirror of the reference API (names / shapes / edge cases of core_test.clj) ---------------
def _dense_oracle(O, base, Q, metric, mode):
    """[nq, n] distance matrix from the oracle's exact kNN with k = n."""
    ids, d, _ = O.exact_knn(base, Q, len(base), metric=metric, mode=mode)
    out = np.empty((len(Q), len(base)), np.float32)
    np.put_along_axis(out, ids.astype(np.int64), d.astype(np.float32), axis=1)
    return out


def _stable_topk(ids, d, k):
    """Collections/sort semantics: stable ascending by distance over the valid entries, first k, -1 padded."""
    oi = np.full((len(ids), k), -1, np.int32)
    od = np.full((len(ids), k), np.inf, np.float32)
    for q in range(len(ids)):
        keep = np.flatnonzero(ids[q] >= 0)
        order = keep[np.argsort(d[q][keep], kind="stable")][:k]
        oi[q, :len(order)] = ids[q][order]
        od[q, :len(order)] = d[q][order]
    return oi, od


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_ivf_search_given_lists_exact(eng, oracle, metric):
    """hnswgpu_ivf_search_lists (caller-chosen partitions: the reference's :turbo / lightning paths) with ragged probe
    rows (-1 = none), small and large batches (GEMV scan in list order with list-less pairs, tile / group scan):
    the expected top-k is the stable sort of the probed lists' rows, concatenated in probe order, by the distances of
    the kernel that serves the batch."""
    O = oracle
    m = {"cosine": O.COSINE, "dot": O.DOT, "l2": O.L2}[metric]
    rs = np.random.RandomState(21)
    n, dim, nlist = 1800, 40, 11
    base = _data(O, n, dim, "clustered", num_clusters=5, noise_level=0.5)
    assign = rs.randint(0, nlist, n)
    assign[assign == 4] = 5                                   # an empty list
    off, lids = O.lists_from_assign(assign, nlist)
    cen = _data(O, nlist, dim, seed=77)
    Qall = _data(O, 40, dim, seed=43)
    with eng.Index(base, metric) as idx:
        idx.set_ivf(cen, off, lids)
        for nq, nprobe, k in [(3, 4, 5), (12, 3, 50), (40, 4, 10), (40, 2, 300)]:
            Q = Qall[:nq]
            probes = np.full((nq, nprobe), -1, np.int32)
            for q in range(nq):
                pick = rs.permutation(nlist)[:nprobe]
                keep = rs.rand(nprobe) < 0.8
                probes[q, keep] = pick[keep]
            tiled = m != O.L2 and nq * nprobe > 12 * nlist
            dense = _dense_oracle(O, base, Q, m, O.MODE_MFMA if tiled else O.MODE_DEV)
            cand_ids = np.full((nq, n), -1, np.int32)
            cand_d = np.full((nq, n), np.inf, np.float32)
            for q in range(nq):
                rows = np.concatenate([lids[off[l]:off[l + 1]] for l in probes[q] if l >= 0] + [np.empty(0, np.int32)])
                cand_ids[q, :len(rows)] = rows
                cand_d[q, :len(rows)] = dense[q, rows.astype(np.int64)]
            want_i, want_d = _stable_topk(cand_ids, cand_d, k)
            ids, d = idx.ivf_search_lists(Q, k, probes)
            assert_exact(ids, d, want_i, want_d, "given lists %s nq=%d nprobe=%d k=%d" % (metric, nq, nprobe, k))


@pytest.mark.parametrize("metric,nq", [("cosine", 20), ("cosine", 5), ("dot", 33), ("l2", 20)])
def test_dense_distances_and_rerank(eng, oracle, metric, nq):
    O = oracle
    m = O.METRICS[metric]
    base = _data(O, 1500, 48)
    base[7] = base[3]                                                # duplicates: ties in the re-rank
    base[9] = base[3]
    Q = _data(O, nq, 48, seed=43)
    tiled = m != O.L2 and nq >= 16
    with eng.Index(base, metric) as idx:
        got = idx.dense_distances(Q)
        want = _dense_oracle(O, base, Q, m, O.MODE_MFMA if tiled else O.MODE_DEV)
        np.testing.assert_array_equal(got, want)
        # re-rank: own candidate list per query, with skips (-1), an out-of-range id and duplicated rows
        rng = np.random.default_rng(5)
        cand = rng.integers(0, len(base), size=(nq, 37)).astype(np.int32)
        cand[:, 5] = -1
        cand[:, 11] = len(base) + 3
        cand[:, 20:23] = [9, 3, 7]
        dev = _dense_oracle(O, base, Q, m, O.MODE_DEV)
        valid = (cand >= 0) & (cand < len(base))
        cd = np.where(valid, np.take_along_axis(dev, np.clip(cand, 0, len(base) - 1).astype(np.int64), axis=1), np.inf)
        for k in (1, 10, 37, 50):
            ids, d = idx.rerank(Q, cand, k)
            wi, wd = _stable_topk(np.where(valid, cand, -1), cd.astype(np.float32), k)
            np.testing.assert_array_equal(ids, wi)
            np.testing.assert_array_equal(d, wd)
        assert idx.dense_distances(Q[:0]).shape == (0, len(base))
    with eng.Index(np.zeros((0, 48), np.float32), metric) as empty:
        ids, d = empty.rerank(Q, cand, 3)
        assert (ids == -1).all() and np.isinf(d).all()


def test_partitioned_hnsw_mirror(eng, oracle):
    """partitioned_hnsw.clj: every mode's k-per-partition rule, searched per partition and merged like
    Collections/sort -- checked against the oracle searching the SAME partition graphs."""
    from hnsw_clj_amd import datagen, partitioned_hnsw as ph

    O = oracle
    vecs = _data(O, 2500, 32, "clustered", num_clusters=12, noise_level=0.4)
    Q = _data(O, 30, 32, seed=43)
    index = ph.build_index(datagen.indexed(vecs), num_partitions=8, ef_construction=60)
    assert len(index.partitions) == 8 and sorted(np.concatenate(index.rows).tolist()) == list(range(2500))
    assert ph.index_info(index)["avg-partition-size"] == 2500 / 8
    graphs = [p.get_graph() for p in index.partitions]
    for mode, k in (("lightning", 10), ("ultra", 10), ("turbo", 3), ("bogus", 4)):
        kpp = ph.k_per_partition(mode, 8, k)
        assert kpp == {"lightning": 3, "ultra": 2, "turbo": 3, "bogus": 3}[mode]
        allid, alld = [], []
        for r, g in zip(index.rows, graphs):
            oi, od, _, _ = O.hnsw_search(vecs[r], g, Q, kpp, mode=O.MODE_DEV)
            allid.append(np.where(oi >= 0, r[np.clip(oi, 0, None)], -1))
            alld.append(od)
        wi, wd = _stable_topk(np.concatenate(allid, 1), np.concatenate(alld, 1).astype(np.float32), k)
        got = ph.search_batch(index, Q, k, mode)
        for q in range(len(Q)):
            assert [r["id"] for r in got[q]] == ["vec_%d" % i for i in wi[q] if i >= 0]
            np.testing.assert_array_equal(np.float32([r["distance"] for r in got[q]]), wd[q][wi[q] >= 0])
        assert ph.search_knn(index, Q[4], k, mode) == got[4]
    # self-match through the String-id table (core_test.clj:33-47 protocol)
    assert ph.search_partitioned_lightning(index, vecs[17], 5)[0]["id"] == "vec_17"
    unshuffled = ph.build_index(datagen.indexed(vecs[:100]), num_partitions=3, shuffle=False, ef_construction=30)
    assert [len(r) for r in unshuffled.rows] == [34, 34, 32] and unshuffled.rows[1][0] == 34
    index.close()
    unshuffled.close()


def test_ivf_hnsw_mirror(eng, oracle):
    """ivf_hnsw.clj: centroid routing, 2k from each probed partition's graph, stable merge."""
    from hnsw_clj_amd import datagen, ivf_hnsw

    O = oracle
    vecs = _data(O, 3000, 32, "clustered", num_clusters=6, noise_level=0.5)
    index = ivf_hnsw.build_index(datagen.indexed(vecs), num_partitions=6, ef_construction=60, max_iterations=4)
    info = ivf_hnsw.index_info(index)
    assert info["vectors"] == 3000 and info["partitions"] == 6
    assert sorted(np.concatenate(index.rows).tolist()) == list(range(3000))
    graphs = [p.get_graph() if p is not None else None for p in index.partitions]
    k = 5
    for nq, mode, honour in ((40, "fast", False), (3, "balanced", False), (40, "accurate", True)):
        Q = _data(O, nq, 32, seed=43)
        cfg = ivf_hnsw.MODE_CONFIGS[mode]
        route_mode = O.MODE_MFMA if nq >= 16 else O.MODE_DEV
        probes, _, _ = O.exact_knn(index.centroids, Q, cfg["num-probes"], mode=route_mode)
        ef = max(cfg["ef-search"], 2 * k) if honour else None
        allid = np.full((nq, cfg["num-probes"] * 2 * k), -1, np.int64)
        alld = np.full((nq, cfg["num-probes"] * 2 * k), np.inf, np.float32)
        for q in range(nq):
            for r, p in enumerate(probes[q]):
                if graphs[p] is None:
                    continue
                oi, od, _, _ = O.hnsw_search(vecs[index.rows[p]], graphs[p], Q[q:q + 1], 2 * k, ef=ef, mode=O.MODE_DEV)
                allid[q, r * 2 * k:(r + 1) * 2 * k] = np.where(oi[0] >= 0, index.rows[p][np.clip(oi[0], 0, None)], -1)
                alld[q, r * 2 * k:(r + 1) * 2 * k] = od[0]
        wi, wd = _stable_topk(allid, alld, k)
        got = ivf_hnsw.search_batch(index, Q, k, mode, honour_modes=honour)
        for q in range(nq):
            assert [r["id"] for r in got[q]] == ["vec_%d" % i for i in wi[q] if i >= 0], (mode, q)
            np.testing.assert_array_equal(np.float32([r["distance"] for r in got[q]]), wd[q][wi[q] >= 0])
    assert ivf_hnsw.search_knn(index, vecs[11], 3)[0]["id"] == "vec_11"
    assert len(ivf_hnsw.search_knn(index, vecs[11], 3, 0.1)) == 3      # legacy search-percent: int(24 * 0.1) = 2 probes
    index.close()


def test_pcaf_mirror(eng, oracle):
    """pcaf.clj: Random(42) gaussian projection, brute-force phase 1 in the projected space, exact re-rank."""
    from hnsw_clj_amd import datagen, pcaf

    O = oracle
    vecs = _data(O, 2000, 96, "clustered", num_clusters=20, noise_level=0.6)
    T = 16
    P = pcaf.create_random_projection(96, T)
    jr = O.JavaRandom(42)
    want_p = np.float32([np.float32(0.25) * np.float32(jr.next_gaussian()) for _ in range(40)])
    np.testing.assert_array_equal(P.reshape(-1)[:40], want_p)         # pcaf.clj:36-45
    index = pcaf.build_index(datagen.indexed(vecs), n_components=T, k_filter=32)
    assert pcaf.index_info(index)["reduction-ratio"] == 6.0
    low = -_dense_oracle(O, P, vecs, O.DOT, O.MODE_MFMA)               # [n, T] projection, tile order (n >= 16)
    for nq, mode, k in ((25, None, 10), (25, "precise", 30), (2, "turbo", 4)):
        Q = _data(O, nq, 96, seed=43)
        qlow = -_dense_oracle(O, P, Q, O.DOT, O.MODE_MFMA if nq >= 16 else O.MODE_DEV)
        kf = min(pcaf.MODE_K_FILTER.get(mode, 32), 3 * k)
        cand, _, _ = O.exact_knn(low, qlow, kf, mode=O.MODE_MFMA if nq >= 16 else O.MODE_DEV)
        dev = _dense_oracle(O, vecs, Q, O.COSINE, O.MODE_DEV)
        cd = np.take_along_axis(dev, cand.astype(np.int64), axis=1)
        wi, wd = _stable_topk(cand, cd, k)
        got = pcaf.search_batch(index, Q, k, mode)
        for q in range(nq):
            assert [r["id"] for r in got[q]] == ["vec_%d" % i for i in wi[q] if i >= 0], (mode, q)
            gd = np.float32([r["distance"] for r in got[q]])
            np.testing.assert_array_equal(gd, wd[q][wi[q] >= 0])
            # and against the reference's f64 cosine on the same ids (north-star tolerance)
            f64 = np.array([O.cosine_distance_ultra(Q[q], vecs[i]) for i in wi[q] if i >= 0])
            assert np.all(np.abs(gd - f64) <= 1e-4 * np.abs(f64) + 1e-6)
    assert pcaf.search_knn(index, vecs[5], 3)[0]["id"] == "vec_5"
    pcaf.cleanup(index)


def test_reference_api_mirror(eng, oracle):
    from hnsw_clj_amd import datagen, ivf_flat, parallel_search, protocol, simd_optimized, ultra_fast

    vecs = datagen.generate_dataset(100, 128)
    data = datagen.indexed(vecs)                                     # [["vec_0", v] ...]
    index = ultra_fast.build_index(data, show_progress=False)
    res = ultra_fast.search_knn(index, vecs[0], 5)                   # core_test.clj:33-47
    assert len(res) == 5 and all("id" in r and "distance" in r for r in res)
    assert res[0]["id"] == "vec_0" and res[0]["distance"] < 0.01
    assert ultra_fast.search_knn(ultra_fast.build_index([], show_progress=False), [1, 2, 3], 5) == []
    batch = parallel_search.parallel_search_futures(index, list(vecs[:20]), 10, ultra_fast.search_knn, 8)
    assert len(batch) == 20 and all(len(r) == 10 for r in batch)     # core_test.clj:112-121
    assert batch[3] == ultra_fast.search_knn(index, vecs[3], 10)
    # a user's own search-fn: the reference's protocol as written (a pool of threads, one task per query), served by
    # combined launches -- same results, in query order
    calls = []

    def my_search(idx_, q, k_):
        calls.append(1)
        return ultra_fast.search_knn(idx_, q, k_, ef=64)

    threaded = parallel_search.parallel_search_futures(index, list(vecs[:20]), 10, my_search, 8)
    assert len(calls) == 20 and threaded == [ultra_fast.search_knn(index, v, 10, ef=64) for v in vecs[:20]]
    bm = parallel_search.benchmark_parallel_search(index, list(vecs[:30]), 5, my_search, 4)
    assert bm["completed"] == 30 and bm["threads"] == 4 and bm["qps"] > 0
    # route=True (not in the reference): the exact scan answers where the traversal would evaluate a third of the base and more
    # (on 100 rows even ef 10 evaluates more than a third of them -- 32 neighbours per expansion: the rule's "traversal" side
    # is checked on 3,000 rows, where ef 10 stays far below 1,000 evaluations and ef 1,500 cannot)
    big_v = datagen.generate_dataset(3000, 64)
    big = ultra_fast.build_index(datagen.indexed(big_v), show_progress=False)
    assert not ultra_fast.routed_to_exact_scan(big, big_v[:8], 5, ef=10) and ultra_fast.routed_to_exact_scan(big, big_v[:8], 5, ef=1500)
    assert ultra_fast.search_batch(big, big_v[:8], 5, ef=10, route=True) == ultra_fast.search_batch(big, big_v[:8], 5, ef=10)
    big.close()
    assert ultra_fast.routed_to_exact_scan(index, vecs[:8], 5, ef=100)
    ex_ids, _ = index.index.exact_knn(vecs[:8], 5)                   # (ef 100 on 100 rows evaluates every row)
    assert [[r["id"] for r in row] for row in ultra_fast.search_batch(index, vecs[:8], 5, ef=100, route=True)] == \
        [["vec_%d" % i for i in row] for row in ex_ids]
    gp = protocol.GpuHnswIndex(index)
    assert gp.search_batch_star(vecs[:3], 4)[2] == ultra_fast.search_knn(index, vecs[2], 4)
    assert protocol.default_batch_search(gp, vecs[:3], 4, None) == gp.search_batch_star(vecs[:3], 4)   # protocol.clj:92-95
    even = protocol.default_filtered_search(gp, vecs[8], 3, lambda i: int(i.split("_")[1]) % 2 == 0, None)   # :96-101
    assert [r["id"] for r in even][0] == "vec_8" and all(int(r["id"].split("_")[1]) % 2 == 0 for r in even) and len(even) <= 3
    assert even == [r for r in ultra_fast.search_knn(index, vecs[8], 9) if int(r["id"].split("_")[1]) % 2 == 0][:3]
    assert protocol.supports_batch_search(gp) and protocol.supports_persistence(gp)
    assert ultra_fast.graph_info(index)["num-elements"] == 100
    index.close()
    l2 = ultra_fast.build_index(data, distance_fn=simd_optimized.euclidean_distance, show_progress=False)
    assert ultra_fast.search_knn(l2, vecs[7], 1)[0] == {"id": "vec_7", "distance": 0.0}
    l2.close()
    ivf = ivf_flat.build_index(data, num_partitions=8, show_progress=False)
    r = ivf_flat.search_knn(ivf, vecs[5], 3, "precise")
    assert r[0]["id"] == "vec_5" and len(r) == 3
    assert len(ivf_flat.search_knn(ivf, vecs[5], 3, "turbo")) == 3
    assert ivf_flat.index_info(ivf)["partitions"] == 8
    ivf.close()
    from hnsw_clj_amd import pure_hnsw, ultra_optimized

    uo = ultra_optimized.build_index(data, show_progress=False)          # README `hnsw.ultra-optimized`
    assert ultra_optimized.search(uo, vecs[4], 5)[0]["id"] == "vec_4"
    uo.close()
    ph = pure_hnsw.build_index(data, show_progress=False)                 # README `hnsw.hnsw-search`
    r1 = pure_hnsw.search_knn(ph, vecs[6], 5, "turbo")
    r2 = pure_hnsw.search_knn(ph, vecs[6], 5, "precise")
    assert r1[0]["id"] == r2[0]["id"] == "vec_6" and len(r2) == 5
    # the drop-in default is what the reference DOES: graph/search-knn ignores the mode presets and searches with
    # ef = (max k 50) (graph.clj:304) -- checked against the oracle on the same graph; the presets are opt-in
    gg = ph.graph.index.get_graph()
    og = oracle.Graph(gg.levels, gg.l0_adj, gg.up_off, gg.up_adj, gg.M, gg.entry, gg.max_level)
    for qi, (k_, mode) in enumerate([(5, "turbo"), (5, "precise"), (60, "balanced"), (3, "no-such-mode")]):
        got = pure_hnsw.search_knn(ph, vecs[10 + qi] * 1.5, k_, mode)
        oi, od, _, _ = oracle.hnsw_search(vecs, og, vecs[10 + qi] * 1.5, k_, ef=max(k_, 50), mode=oracle.MODE_DEV)
        assert [r["id"] for r in got] == ["vec_%d" % i for i in oi[0] if i >= 0]
        assert np.array_equal(np.float32([r["distance"] for r in got]).view(np.uint32),
                              od[0][oi[0] >= 0].astype(np.float32).view(np.uint32))
        uo_got = ultra_fast.search_knn(ph.graph, vecs[10 + qi] * 1.5, k_)       # hnsw.ultra-optimized/search == base/search-knn
        assert uo_got == got
    wide = pure_hnsw.search_knn(ph, vecs[12] * 1.5, 5, "precise", honour_modes=True)  # opt-in: ef 500
    oi, od, _, _ = oracle.hnsw_search(vecs, og, vecs[12] * 1.5, 5, ef=500, mode=oracle.MODE_DEV)
    assert [r["id"] for r in wide] == ["vec_%d" % i for i in oi[0]]
    info = pure_hnsw.index_info(ph)
    assert info["vectors"] == 100 and info["params"]["M"] == 16 and info["avg-edges-per-node"] > 1
    ph.close()
    assert simd_optimized.cosine_distance([1, 0], [-1, 0]) == 2.0
    assert simd_optimized.dot_product([1, 2, 3], [4, 5, 6]) == 32.0
    bd = simd_optimized.batch_cosine_distances(vecs[0], vecs[:10])
    assert bd.shape == (10,) and abs(bd[0]) < 1e-6
    top = simd_optimized.top_k_distances(simd_optimized.euclidean_distance, vecs[0], vecs, 3)
    assert top[0] == [0, 0.0] and len(top) == 3
