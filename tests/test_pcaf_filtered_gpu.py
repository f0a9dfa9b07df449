"""The allow-mask through P-HNSW's low-dimensional filter (hnswgpu_pcaf_search_filtered / _each / _dev; pcaf_filter_masked_kernel)
against the float64 restatement of the unfiltered search applied to the passing rows alone, and against the entry points
themselves where the contract says "bit for bit"."""
import numpy as np
import pytest

import util
from hnsw_clj_amd import datagen, engine, pcaf
from test_pcaf_one_handle_gpu import clustered, reference

pytestmark = pytest.mark.gpu


def make_bits(n, nq, rates, seed, clear=(0, 0)):
    """bool [nq][n]: query q lets a row of the lower / upper half of the id range pass with probability
    rates[q % len(rates)][0] / [1]; the rows clear[0] .. clear[1] pass for nobody."""
    rng = np.random.RandomState(seed)
    b = np.stack([rng.rand(n) < np.repeat(rates[q % len(rates)], (n + 1) // 2)[:n] for q in range(nq)])
    b[:, clear[0]:clear[1]] = False
    return b


def build(n, dim, T, nq):
    base, Q = clustered(n, dim), clustered(nq, dim, seed=44)
    idx = engine.Index(base, "cosine", 0)
    idx.pcaf_build(T, 42)
    return base, Q, idx


def run(idx, form, Q, k, bits, kf):
    if form == "one":
        return idx.pcaf_search_filtered(Q, k, engine.pack_mask(bits[0], idx.n), kf)
    return idx.pcaf_search_filtered_each(Q, k, engine.pack_masks(bits, idx.n), kf)


# (plans at 256 CUs; mask seed: the f64 reference alone leaves at most 1 sampled query in 8 undecided, in both forms)
SHAPES = {
    # two query blocks, the second ragged; 6 slabs of 256 rows, one word per wave, every step partial; ~50 % pass -- seed 1
    "ragged": (1500, 96, 16, 33, 10, 32, [(0.5, 0.5)], 1, (0, 0)),
    # ~3 % pass: clear words, slabs 1 and 2 clear, fewer than kf per slab; each: every 4th query under k rows, q3 none, q7 all -- seed 2
    "sparse": (1500, 100, 20, 33, 10, 32, [(0.03, 0.03)] * 3 + [(0.004, 0.004)], 2, (256, 768)),
    # nine query blocks, 27 slabs of 1536 rows, 6 words per wave, 2 to 5 steps per wave and slab by the halves' density -- seed 3
    "steps": (40000, 32, 8, 260, 10, 32, [(0.7, 0.1), (0.1, 0.7), (0.4, 0.4)], 3, (0, 0)),
    # 256 query blocks: ONE slab, 157 words per wave, three 64-word loads (shared mask only) -- seed 4
    "refill": (40000, 32, 8, 8192, 10, 32, [(0.7, 0.1)], 4, (0, 0)),
    # kf = 64 against a 2 kf buffer that refills many times, with gathered rows; ~70 % pass -- seed 10
    "cuts": (300, 36, 8, 5, 30, 64, [(0.7, 0.7)], 10, (0, 0)),
}


@pytest.mark.parametrize("shape,form", [(s, f) for s in SHAPES for f in ("one", "each") if (s, f) != ("refill", "each")])
def test_parity(native_lib, shape, form):
    n, dim, T, nq, k, k_filter, rates, seed, clear = SHAPES[shape]
    bits = make_bits(n, nq if form == "each" else 1, rates, seed, clear)
    if shape == "sparse" and form == "each":
        bits[3], bits[7] = False, True
    base, Q, idx = build(n, dim, T, nq)
    with idx:
        P = idx.pcaf_get()[0]
        ids, d = run(idx, form, Q, k, bits, k_filter)
    assert ids.shape == d.shape == (nq, k)
    sample = np.arange(nq) if nq <= 64 else np.unique(np.r_[np.arange(16) * (nq // 16), nq - 1])
    undecided = 0
    for q in sample:
        allow = bits[q if form == "each" else 0]
        rows = np.flatnonzero(allow)
        wi, wd, decided, _, _ = reference(base[rows], P, Q[q:q + 1], k, k_filter)
        want = np.where(wi >= 0, rows[np.maximum(wi, 0)] if len(rows) else -1, -1)
        got = ids[q][ids[q] >= 0]
        assert allow[got].all(), (q, "a row whose bit is clear was returned")
        if decided[0]:
            util.assert_topk_parity(ids[q:q + 1], d[q:q + 1], want, wd, "q%d" % q)
            continue
        undecided += 1   # the returned distances are those of the returned ids
        assert len(got) == min(k, k_filter, 3 * k, len(rows)) and len(set(got.tolist())) == len(got)
        a, b = np.float64(Q[q]), np.float64(base[got])
        f64 = 1.0 - b @ a / (np.linalg.norm(b, axis=1) * np.linalg.norm(a))
        assert util.close(d[q][:len(got)], f64).all() and np.isinf(d[q][len(got):]).all()
    print("undecided queries: %d of %d" % (undecided, len(sample)))
    assert undecided * 8 <= len(sample)


@pytest.mark.parametrize("shape", ["ragged", "steps"])
def test_identities(native_lib, shape):
    import torch

    n, dim, T, nq, k, k_filter, rates, seed, _ = SHAPES[shape]
    bits = make_bits(n, nq, rates, seed)
    bits[1], bits[2] = False, True
    words = engine.pack_masks(bits, n)
    base, Q, idx = build(n, dim, T, nq)

    def same(a, b):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))

    with idx:
        ones = np.ones(n, bool)
        plain = idx.pcaf_search(Q, k, k_filter)
        same(idx.pcaf_search_filtered(Q, k, engine.pack_mask(ones, n), k_filter), plain)
        same(idx.pcaf_search_filtered_each(Q, k, engine.pack_masks(np.tile(ones, (nq, 1)), n), k_filter), plain)
        one, each = idx.pcaf_search_filtered(Q, k, words[0], k_filter), idx.pcaf_search_filtered_each(Q, k, words, k_filter)
        assert (each[0][1] == -1).all() and np.isinf(each[1][1]).all()
        for q in [0, 1, 2, 31, 32, nq - 1]:
            single = idx.pcaf_search_filtered(Q[q:q + 1], k, words[q], k_filter)
            same((each[0][q:q + 1], each[1][q:q + 1]), single)
        dev = torch.device("cuda", 0)
        tq, tw = torch.from_numpy(Q).to(dev), torch.from_numpy(words.view(np.int32)).to(dev)
        di, dd = idx.pcaf_search_filtered_dev(tq, k, tw[0], k_filter)
        ei, ed = idx.pcaf_search_filtered_each_dev(tq, k, tw, k_filter)
        torch.cuda.synchronize()
        same((di.cpu().numpy(), dd.cpu().numpy()), one)
        same((ei.cpu().numpy(), ed.cpu().numpy()), each)


def test_mirror(native_lib):
    vecs, Q, k = clustered(1500, 96), clustered(7, 96, seed=43), 10
    data = datagen.indexed(vecs)
    one, three = pcaf.build_index(data, n_components=16, one_handle=True), pcaf.build_index(data, n_components=16)
    try:
        preds = [lambda i: int(i.split("_")[1]) % 3 == 0, lambda i: int(i.split("_")[1]) < 40, make_bits(1500, 1, [(0.2, 0.6)], 6)[0]]
        fns = [preds[q % 3] for q in range(len(Q))]
        batch = pcaf.search_batch_filtered_each(one, Q, k, fns, "fast")
        assert batch == [pcaf.search_knn_filtered(one, Q[q], k, fns[q], "fast") for q in range(len(Q))]
        assert all(len(r) == k and all(preds[0](x["id"]) for x in r) for r in batch[0::3])
        assert pcaf.search_batch_filtered_each(one, Q, k, [preds[1]] * len(Q)) == pcaf.search_batch_filtered(one, Q, k, preds[1])
        with pytest.raises(ValueError, match="one_handle=True"):
            pcaf.search_knn_filtered(three, Q[0], k, preds[0])
    finally:
        pcaf.cleanup(one)
        pcaf.cleanup(three)


ROWS, QS = clustered(200, 32), clustered(3, 32, seed=43)
ONES = engine.pack_mask(np.ones(200, bool), 200)
OUT = np.empty((3, 5), np.int32), np.empty((3, 5), np.float32)


def _null_mask(i, name):
    engine.check(getattr(engine.lib(), name)(i._h, engine._p(QS), 3, 5, 0, None, engine._p(OUT[0]), engine._p(OUT[1])))


@pytest.mark.parametrize("state,call,error,code", [
    (True, lambda i: _null_mask(i, "hnswgpu_pcaf_search_filtered"), engine._native.HnswGpuError, -1),
    (True, lambda i: _null_mask(i, "hnswgpu_pcaf_search_filtered_each"), engine._native.HnswGpuError, -1),
    (False, lambda i: i.pcaf_search_filtered(QS, 5, ONES), engine._native.HnswGpuError, -3),
    (False, lambda i: i.pcaf_search_filtered_each(QS, 5, np.tile(ONES, (3, 1))), engine._native.HnswGpuError, -3),
    (True, lambda i: i.pcaf_search_filtered(QS, 43, ONES, 129), engine._native.HnswGpuError, -5),
    (True, lambda i: i.pcaf_search_filtered_each(QS, 43, np.tile(ONES, (3, 1)), 129), engine._native.HnswGpuError, -5),
    (True, lambda i: i.pcaf_search_filtered(QS, 5, ONES[:-1]), ValueError, None),
    (True, lambda i: i.pcaf_search_filtered_each(QS, 5, np.tile(ONES, (2, 1))), ValueError, None),
])
def test_refusals(native_lib, state, call, error, code):
    with engine.Index(ROWS, "cosine", 0) as idx:
        if state:
            idx.pcaf_build(8, 42)
        half = engine.pack_mask(np.arange(200) % 2 == 0, 200)
        search = (lambda: idx.pcaf_search_filtered(QS, 5, half)) if state else (lambda: idx.exact_knn(QS, 5))
        before = search()
        with pytest.raises(error) as e:
            call(idx)
        assert code is None or e.value.code == code, str(e.value)
        after = search()
        np.testing.assert_array_equal(before[0], after[0])
        np.testing.assert_array_equal(before[1], after[1])
