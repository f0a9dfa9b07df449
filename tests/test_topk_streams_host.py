"""The premise of tests/test_topk_streams_gpu.py, pinned on the CPU: rows v[i] * e0 make any float32 stream v the exact
distance stream of a search, in the GEMV and in the MFMA summation order alike, so the oracle's exact kNN and IVF routing
over them equal a plain stable argsort of the stream (topk_streams.expected) in ids and in float32 values."""
import numpy as np
import pytest

import topk_streams as ts

SCALES = (1.0, 2.0, -1.0)
CASES = [(700, 10), (1025, 65)]      # (n, the k that places the two_values / plateau boundaries and is searched for)


def _check(got, stream, k, what):
    ids, d = got
    for qi in range(len(stream)):
        wi, wd = ts.expected(stream[qi], k)
        ts.assert_same(ids[qi], d[qi].astype(np.float32), wi, wd, "%s query %d" % (what, qi))


@pytest.mark.parametrize("dim", [4, 128])
@pytest.mark.parametrize("n,k", CASES)
def test_streams_are_the_oracles_distances(oracle, n, k, dim):
    O = oracle
    rs = np.random.RandomState(n + dim)
    for name, v in ts.families(n, k, rs):
        what = "%s n=%d dim=%d" % (name, n, dim)
        # dot: query -s * e0, distance s * v[i]
        v1 = ts.fit_scale(v, max(SCALES, key=abs))                  # one set of rows serves every scale
        base = ts.rows_of(v1, dim)
        Q = np.stack([ts.unit_query(-s, dim) for s in SCALES])
        streams = [ts.dot_stream(v1, s) for s in SCALES]
        assert all(np.isfinite(s).all() for s in streams), what
        for mode in (O.MODE_DEV, O.MODE_MFMA):
            oi, od, _ = O.exact_knn(base, Q, k, metric=O.DOT, mode=mode)
            _check((oi, od), streams, k, "dot exact mode %d %s" % (mode, what))
        # the IVF routing over "row i is centroid i, list i holds row i": the probes are the selection, the result the same list
        off, lids = np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32)
        for mode in (O.MODE_DEV, O.MODE_MFMA):
            oi, od, pr = O.ivf_search(base, base, off, lids, Q, k, k, metric=O.DOT, mode=mode)
            for qi in range(len(Q)):
                wi, wd = ts.expected(streams[qi], k)
                np.testing.assert_array_equal(pr[qi], wi, err_msg="dot ivf probes mode %d %s" % (mode, what))
            _check((oi, od), streams, k, "dot ivf mode %d %s" % (mode, what))
        # l2: zero query, distance |v[i]| (squares exact)
        if name == "grid":
            oi, od, _ = O.exact_knn(base, np.zeros((1, dim), np.float32), k, metric=O.L2, mode=O.MODE_DEV)
            _check((oi, od), [np.abs(v1)], k, "l2 exact " + what)
            oi, od, pr = O.ivf_search(base, base, off, lids, np.zeros((1, dim), np.float32), k, k, metric=O.L2, mode=O.MODE_DEV)
            np.testing.assert_array_equal(pr[0], ts.expected(np.abs(v1), k)[0], err_msg="l2 ivf probes " + what)
        # cosine: query e0, distance 0 / 1 / 2 (moderate families)
        if name.split("_")[0] in ("equal", "two", "plateau"):
            r, cs = ts.cosine_rows(v, k)
            cbase = ts.rows_of(r, dim)
            q = ts.unit_query(1.0, dim)[None, :]
            for mode in (O.MODE_DEV, O.MODE_MFMA):
                oi, od, _ = O.exact_knn(cbase, q, k, metric=O.COSINE, mode=mode)
                _check((oi, od), [cs], k, "cosine exact mode %d %s" % (mode, what))
                oi, od, pr = O.ivf_search(cbase, cbase, off, lids, q, k, k, metric=O.COSINE, mode=mode)
                np.testing.assert_array_equal(pr[0], ts.expected(cs, k)[0], err_msg="cosine ivf probes mode %d %s" % (mode, what))
                _check((oi, od), [cs], k, "cosine ivf mode %d %s" % (mode, what))


def test_expectations_on_hand_made_cases():
    """The expectation helpers against cases small enough to write down."""
    v = np.array([2.0, 1.0, 2.0, -0.0, 0.0, 1.0], np.float32)
    ids, d = ts.expected(v, 8)
    assert ids.tolist() == [3, 4, 1, 5, 0, 2, -1, -1] and d[:6].tolist() == [0, 0, 1, 1, 2, 2] and np.isinf(d[6:]).all()
    ids, d = ts.expected_mapped(v, [5, -1, 9, 1, 1, 0], 3)          # -1 and ids >= n are skipped, repeats stay
    assert ids.tolist() == [5, 1, 1] and d.tolist() == [1, 1, 1]
    li = np.array([[7, 8, -1], [9, -1, -1], [-1, -1, -1]])
    ld = np.array([[1.0, np.inf, np.inf], [1.0, np.inf, np.inf], [np.inf] * 3], np.float32)
    ids, d = ts.expected_merge(li, ld, 4)                           # ties to the lower list; a valid +inf before the padding
    assert ids.tolist() == [7, 9, 8, -1] and d[:2].tolist() == [1, 1] and np.isinf(d[2:]).all()
    order = np.array([[5, 0xfffffffe, 0], [0, 0, 0], [0, 0, 0]], np.uint32)
    ids, _ = ts.expected_merge(li, ld, 2, order=order)              # ties to the lower order word whatever the list
    assert ids.tolist() == [9, 7]
    for n, k in [(63, 10), (1025, 64), (1024, 1024)]:               # every variant that fits really straddles the boundary
        rs = np.random.RandomState(n)
        for name, s in ts.families(n, k, rs):
            assert s.dtype == np.float32 and s.shape == (n,) and not np.isnan(s).any(), name
            if name.startswith("plateau"):
                t = int(name.split("_")[1])
                srt = np.sort(s)
                kth = srt[min(k, n) - 1]
                assert (s == kth).sum() == t, name
                first = int(np.searchsorted(srt, kth))
                want = {"first": first == min(k, n) - 1, "last": first + t == min(k, n) or first == 0,
                        "inside": first <= min(k, n) - 1 < first + t}[name.split("_")[2]]
                assert want, name
    names = {nm for nm, _, _, _ in ts.sample([1, 2, 63, 1025], [1, 10, 64, 65], 1)}
    assert {"equal", "two_values_k", "low_bits_256", "low_bits_65536", "descending", "ascending", "straddle", "grid",
            "gaussian", "plateau_2_first"} <= names
