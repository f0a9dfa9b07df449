"""The HNSW traversals' rejection test with the query in a 16-bit code (kernels.hpp: Query16, two int8 planes against the
int8 rows): hnswgpu_hnsw_rejection_bounds returns its lower bounds by the traversals' own device functions.  They must
never exceed the distance the exact path computes -- or a traversal would drop a neighbour the reference admits -- and
they must be tighter than the bounds with the query in int8 (hnswgpu_rejection_bounds), or the change buys nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(native_lib):
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    return engine


@pytest.mark.parametrize("dim", [24, 300, 768, 1024, 1030, 1536, 1538, 2048, 2050, 3072])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_hnsw_rejection_bounds_never_exceed_the_distance(eng, metric, dim):
    """The rows of test_rejection_bounds_never_exceed_the_distance (every row-loader width -- 2048: eight chunks; 1030, 1538, 2050:
    five, seven and nine chunks in loaders of six, eight and twelve, the last one padding from end to end --, rows of scales e^+-6, a zero
    row, a row with one huge component, a duplicate, non-finite rows) against a gaussian query, duplicates of rows (one
    scaled by 1000, one with the huge component), a zero query, tiny queries (1e-15 times a gaussian, and 1e-25: below the
    size that still gets a code) and non-finite queries: wherever the 16-bit bound is
    not NaN it is <= the distance hnswgpu_batch_distances reports; non-finite rows and queries abstain; on the
    well-behaved block the bound exists for every row and its mean gap to the distance is below the int8 query's."""
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
    q_nan, q_inf = rs.randn(dim).astype(np.float32), rs.randn(dim).astype(np.float32)
    q_nan[dim // 2] = np.nan
    q_inf[0] = -np.inf
    g = rs.randn(dim)
    queries = [rs.randn(dim).astype(np.float32), base[5].copy(), (base[7] * 1000).astype(np.float32),
               np.zeros(dim, np.float32), base[201].copy(), (g * 1e-15).astype(np.float32), (g * 1e-25).astype(np.float32),
               q_nan, q_inf]
    with eng.Index(base, metric) as idx:
        idx.set_rejection_test(2)          # int8 rows whatever the default mode and the dim
        for qi, q in enumerate(queries):
            lb = idx.hnsw_rejection_bounds(q, ids)
            d = idx.batch_distances(q, ids)
            ok = ~np.isnan(lb)
            assert np.all(lb[ok] <= d[ok]), "metric %s dim %d query %d: bound above the distance at rows %s" % (
                metric, dim, qi, np.nonzero(ok & ~(lb <= d))[0][:8])
            assert np.isnan(lb[203]) and np.isnan(lb[204])            # non-finite rows abstain
            if qi >= 7:
                assert not ok.any(), "metric %s dim %d: a non-finite query got a bound" % (metric, dim)
            if qi == 0:                                               # tightness on the well-behaved block
                lb8 = idx.rejection_bounds(q, ids)
                gap16, gap8 = (d[:200] - lb[:200]).astype(np.float64), (d[:200] - lb8[:200]).astype(np.float64)
                print("metric %s dim %d: mean gap 16-bit query %.6g, int8 query %.6g" % (metric, dim, gap16.mean(), gap8.mean()))
                assert ok[:200].all() and not np.isnan(lb8[:200]).any()
                assert gap16.mean() < gap8.mean(), (gap16.mean(), gap8.mean())


@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_hnsw_rejection_bounds_reject_more_rows(eng, metric):
    """The filter's gain without a traversal, on the kind of rows the headline searches: clustered, L2-normalised, 768-d.
    For a held-out query the threshold is its 640th-smallest exact distance (the worst of a full list at ef 640); a row
    whose lower bound is >= the threshold needs no f32 fetch.  The 16-bit query code must find MORE such rows than the
    int8 query code for every query (the two sets need not nest: the two codes round differently).  Queries: four further
    draws of the base's mixture, four of another seed's (other centres, as bench.py's held-out queries are)."""
    from hnsw_clj_amd import datagen

    n, dim, nclu = 8000, 768, 64
    x = datagen.generate_dataset(n + 4, dim, "clustered", num_clusters=nclu, noise_level=0.3, seed=42, dtype=np.float64)
    y = datagen.generate_dataset(4, dim, "clustered", num_clusters=nclu, noise_level=0.3, seed=43, dtype=np.float64)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    base = x[:n].astype(np.float32)
    queries = np.concatenate([x[n:], y]).astype(np.float32)
    ids = np.arange(n, dtype=np.int32)
    with eng.Index(base, metric) as idx:
        idx.set_rejection_test(2)
        for qi, q in enumerate(queries):
            d = idx.batch_distances(q, ids)
            thr = np.sort(d)[639]
            lb16, lb8 = idx.hnsw_rejection_bounds(q, ids), idx.rejection_bounds(q, ids)
            assert np.all(lb16 <= d) and np.all(lb8 <= d)
            n16, n8 = int((lb16 >= thr).sum()), int((lb8 >= thr).sum())
            exact = int((d >= thr).sum())
            print("metric %s query %d: rows decided without f32 fetch: 16-bit query %d, int8 query %d, exact test %d of %d"
                  % (metric, qi, n16, n8, exact, n))
            assert n8 < n16 <= exact, (metric, qi, n8, n16, exact)
