"""The allow-mask through the hybrid LSH bucket scan (hnswgpu_lsh_search_filtered / _each / _dev) against two yardsticks that do
not run the new code: the filtered numpy model (lsh_filtered_model.py) fed with the CPU oracle's dense device-order distances --
ids and distance bits equal -- and the unfiltered search of a handle created over the passing rows alone."""
import numpy as np
import pytest

import lsh_filtered_model as F
import lsh_model as M
from util import assert_exact, close, metric_scale

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "l2", "dot"]
K = 10
# (num_probes, probe_radius, take_main, take_flip): test_lsh_gpu's six -- the five modes and search-hybrid's default form
CONFIGS = [(p, r, 2 * K, K) for p, r in M.MODES.values()] + [(2, 0, 3 * K, K)]
N, NQ = 2000, 33
MASK_NAMES = ["p50", "p10", "p02", "ones", "zeros"]


def _om(O, metric):
    return {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]


def _dense(O, base, Q, metric, mode):
    """Every query's distance to every row, [nq][n], from one exact_knn over the whole base (-0 canonicalised as the keys do)"""
    ids, d, _ = O.exact_knn(base, Q, len(base), metric=_om(O, metric), mode=mode)
    D = np.empty((len(Q), len(base)), np.float64)
    np.put_along_axis(D, ids.astype(np.int64), d, axis=1)
    return D + 0.0


def _oracle_codes(O, X, planes):
    """bit i of table t = the oracle's negated GEMV-order dot with the plane in the query's role >= 0 (as test_lsh_gpu's)"""
    T, B, dim = planes.shape
    X, planes = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(planes, np.float32)
    fn, pp = O.lib().orc_dist_dev, [[O._p(planes[t, i]) for i in range(B)] for t in range(T)]
    dist = np.array([[[fn(O.DOT, pp[t][i], xp, dim, 1.0, 1.0) for i in range(B)] for t in range(T)] for xp in map(O._p, X)])
    return M.codes_from_dots(-dist)


def make_data():
    rng = np.random.default_rng(2000)
    base = rng.standard_normal((N, 128)).astype(np.float32)
    Q = rng.standard_normal((NQ, 128)).astype(np.float32)
    Q[::2] = base[rng.integers(0, N, 17)] + 0.05 * rng.standard_normal((17, 128)).astype(np.float32)   # near a base row
    return base, Q


def make_masks(n=N):
    rng = np.random.default_rng(77)
    u = rng.random(n)
    return {"p50": u < 0.5, "p10": u < 0.1, "p02": u < 0.02, "ones": np.ones(n, np.bool_), "zeros": np.zeros(n, np.bool_)}


def make_codes(O, base, Q):
    """The reference's hyperplanes (Random(42), 8 x 64 x dim, the first 12 rows of a table) and the 12-bit codes under them, from
    the oracle alone; a build with fewer bits keeps the low bits."""
    r = O.JavaRandom(42)
    planes = np.array([r.next_gaussian() for _ in range(8 * 64 * 128)]).reshape(8, 64, 128)[:, :12].astype(np.float32)
    return planes, _oracle_codes(O, base, planes), _oracle_codes(O, Q, planes)


def non_vacuity(D, qcodes, off, ids, bits, masks):
    """What makes the parity test bite at 8 x 4 bits, from the model alone: (a probed bucket with more passing rows than its take
    under the 50 % mask, a padded result under the 2 % mask, a query where filter-then-take differs from post-filtering a 3 k
    unfiltered search)"""
    cfg = CONFIGS[2]   # balanced
    over = any(c > take for q in range(len(qcodes)) for c, take in F.passing_per_probe(qcodes[q], off, ids, bits, *cfg, masks["p50"]))
    gi, _ = F.search_batch(D, qcodes, off, ids, bits, K, *CONFIGS[0], masks["p02"])   # turbo: 4 buckets of 16 x 2 tables
    padded = bool((gi[:, -1] < 0).any())
    differs = False
    p, r = cfg[:2]
    for q in range(len(qcodes)):
        post = [x for x in M.search(D[q], qcodes[q], off, ids, bits, 3 * K, p, r, 6 * K, 3 * K) if masks["p10"][x]][:K]
        differs = differs or post != F.search(D[q], qcodes[q], off, ids, bits, K, *cfg, masks["p10"])
    return over, padded, differs


@pytest.fixture(scope="module")
def data2000():
    return make_data()


@pytest.fixture(scope="module")
def codes2000(oracle, data2000):
    return make_codes(oracle, *data2000)


@pytest.fixture(scope="module")
def masks2000():
    return make_masks()


@pytest.fixture(scope="module")
def dense2000(oracle, data2000):
    """(metric, oracle mode) -> the dense distances of data2000, computed once and shared (read only)"""
    cache = {}

    def get(metric, mode):
        if (metric, mode) not in cache:
            cache[metric, mode] = _dense(oracle, *data2000, metric, mode)
            cache[metric, mode].setflags(write=False)
        return cache[metric, mode]
    return get


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a[0]), np.asarray(b[0])) and \
        np.array_equal(np.asarray(a[1], np.float32).view(np.uint32), np.asarray(b[1], np.float32).view(np.uint32))


def _passing_only(gi, allow, what=""):
    got = gi[gi >= 0]
    assert allow[got].all(), "%s: a returned row's bit is clear" % what


@pytest.mark.parametrize("bits", [4, 12])
@pytest.mark.parametrize("metric", METRICS)
def test_model_parity(native_lib, oracle, data2000, codes2000, masks2000, dense2000, metric, bits):
    from hnsw_clj_amd import engine

    O = oracle
    base, Q = data2000
    planes, codes, qcodes = codes2000
    codes, qcodes = codes & ((1 << bits) - 1), qcodes & ((1 << bits) - 1)
    off, ids = M.buckets(codes, bits)
    D = dense2000(metric, O.MODE_DEV)
    D64 = dense2000(metric, O.MODE_F64)
    scale = metric_scale(metric, Q, base)
    if bits == 4:
        over, padded, differs = non_vacuity(D, qcodes, off, ids, bits, masks2000)
        print("non-vacuity %s: over-take bucket %s, padded %s, differs from post-filter %s" % (metric, over, padded, differs))
        assert over and padded and differs
    with engine.Index(base, metric, 0) as idx:
        idx.lsh_build(8, bits, 64, 42)
        _, gc, goff, gids = idx.lsh_get()
        assert np.array_equal(gc, codes) and np.array_equal(goff, off) and np.array_equal(gids, ids)
        assert np.array_equal(idx.lsh_hash(Q), qcodes)
        for name in MASK_NAMES:
            allow = masks2000[name]
            words = engine.pack_mask(allow, N)
            for cfg in CONFIGS:
                ei, ed = F.search_batch(D, qcodes, off, ids, bits, K, *cfg, allow)      # per query: the rows of a smaller batch too
                for nq in (1, 7, 33):
                    what = "%s %s nq %d %s" % (name, metric, nq, cfg)
                    gi, gd = idx.lsh_search_filtered(Q[:nq], K, words, *cfg)
                    assert_exact(gi, gd, ei[:nq], ed[:nq], what)
                    _passing_only(gi, allow, what)
                    for q in range(nq):
                        c = int((gi[q] >= 0).sum())
                        assert (gi[q, c:] == -1).all() and np.isinf(gd[q, c:]).all() and len(set(gi[q, :c].tolist())) == c
                        assert close(gd[q, :c], D64[q, gi[q, :c]], scale).all()
                if name == "zeros":
                    assert (ei == -1).all()


@pytest.mark.parametrize("bits", [4, 12])
@pytest.mark.parametrize("metric", METRICS)
def test_sub_index_cross_check(native_lib, data2000, masks2000, metric, bits):
    """The filtered call == the unfiltered search of a handle over the passing rows alone under the same planes, ids mapped back."""
    from hnsw_clj_amd import engine

    base, Q = data2000
    with engine.Index(base, metric, 0) as idx:
        idx.lsh_build(8, bits, 64, 42)
        planes = idx.lsh_get()[0]
        for name in ("p50", "p10"):
            allow = masks2000[name]
            rows = np.flatnonzero(allow)
            words = engine.pack_mask(allow, N)
            with engine.Index(base[allow], metric, 0) as sub:
                sub.set_lsh(planes)
                for cfg in CONFIGS:
                    si, sd = sub.lsh_search(Q, K, *cfg)
                    gi, gd = idx.lsh_search_filtered(Q, K, words, *cfg)
                    mapped = np.where(si >= 0, rows[np.maximum(si, 0)], -1)
                    assert np.array_equal(gi, mapped), (name, metric, cfg)
                    assert np.array_equal(gd.view(np.uint32), sd.view(np.uint32)), (name, metric, cfg)


@pytest.mark.parametrize("n", [2000, 1999])
def test_all_ones_is_the_unfiltered_search(native_lib, data2000, n):
    """Single and _each, bit for bit; n = 1999 leaves 17 garbage bits set beyond n in the last word."""
    from hnsw_clj_amd import engine

    base, Q = data2000
    W = (n + 31) // 32
    words = np.full(W, 0xFFFFFFFF, np.uint32)
    assert n % 32 == 0 or (words[-1] >> (n % 32)) != 0
    for metric, bits in (("cosine", 4), ("l2", 12), ("dot", 4)):
        with engine.Index(base[:n], metric, 0) as idx:
            idx.lsh_build(8, bits, 64, 42)
            for cfg in CONFIGS:
                want = idx.lsh_search(Q, K, *cfg)
                assert (want[0] < n).all()
                assert _bits_equal(want, idx.lsh_search_filtered(Q, K, words, *cfg)), (metric, cfg)
                assert _bits_equal(want, idx.lsh_search_filtered_each(Q, K, np.tile(words, (len(Q), 1)), *cfg)), (metric, cfg)


def _patterns(RB, size, rng):
    """name -> bool[size]: which positions j of a bucket pass"""
    j = np.arange(size)
    return {
        "none": np.zeros(size, np.bool_),
        "all": np.ones(size, np.bool_),
        "even": j % 2 == 0,
        "first": j == 0,
        "last": j == size - 1,
        "le_RB": j <= RB,                       # RB + 1 pass: one full step and a flush of one
        "tail_of_block0": j >= 64 - (RB - 1),   # RB - 1 leftovers carried from block 0 into block 1
        "one_per_block": j % 64 == 63,          # the queue fills across blocks
        "random30": rng.random(size) < 0.3,
    }


@pytest.mark.parametrize("dim,RB", [(128, 8), (1536, 4), (3072, 2)])
def test_queue_edges(native_lib, oracle, dim, RB):
    """One table of 4 axis-aligned bits: bucket b holds sizes[b] rows; masks by position inside the bucket, around the blocks of 64
    positions a wave reads, the RB rows of a step and both key stores' takes."""
    from hnsw_clj_amd import engine

    O = oracle
    sizes = sorted({0, 1, RB, 63, 64, 65, 64 + RB, 127, 128, 129, 200} | ({64 * RB + 1} if dim == 128 else set()))
    assert len(sizes) <= 16
    rng = np.random.default_rng(dim)
    sign = lambda b: np.array([1.0 if (b >> i) & 1 else -1.0 for i in range(4)], np.float32)
    rows, Q, code = [], [], []
    for b, s in enumerate(sizes):
        x = rng.standard_normal((s + 1, dim)).astype(np.float32)
        x[:, :4] = np.abs(x[:, :4]) * sign(b)
        rows.append(x[:s])
        Q.append(x[s])
        code += [b] * s
    perm = rng.permutation(len(code))
    base = np.concatenate(rows)[perm]
    codes = np.array(code, np.uint16)[perm][:, None]
    n = len(base)
    Q = np.stack(Q)
    qcodes = np.arange(len(sizes), dtype=np.uint16)[:, None]
    planes = np.zeros((1, 4, dim), np.float32)
    planes[0, np.arange(4), np.arange(4)] = 1
    off, ids = M.buckets(codes, 4)       # membership from the crafted codes
    assert np.diff(off[0])[:len(sizes)].tolist() == sizes
    names = list(_patterns(RB, 1, rng))
    masks = {name: np.zeros(n, np.bool_) for name in names}
    for b, s in enumerate(sizes):
        members = ids[0, off[0, b]:off[0, b + 1]]
        for name, pat in _patterns(RB, s, rng).items():
            masks[name][members[pat]] = True
    passing = {name: [int(masks[name][ids[0, off[0, b]:off[0, b + 1]]].sum()) for b in range(len(sizes))] for name in names}
    assert passing["le_RB"][sizes.index(200)] == RB + 1 and passing["tail_of_block0"][sizes.index(65)] == RB
    assert passing["tail_of_block0"][sizes.index(64)] == RB - 1 and passing["one_per_block"][sizes.index(200)] == 3
    # every pattern at once: one query per bucket repeated per pattern, neighbouring waves of a workgroup hold different masks
    Qe = np.repeat(Q, len(names), axis=0)
    qce = np.repeat(qcodes, len(names), axis=0)
    me = np.stack([masks[name] for _ in sizes for name in names])
    for metric in ("cosine", "l2"):
        D = _dense(O, base, Q, metric, O.MODE_DEV)
        De = np.repeat(D, len(names), axis=0)
        with engine.Index(base, metric, 0) as idx:
            idx.set_lsh(planes)
            _, gc, goff, gids = idx.lsh_get()
            assert np.array_equal(gc, codes) and np.array_equal(goff, off) and np.array_equal(gids, ids)
            assert np.array_equal(idx.lsh_hash(Q), qcodes)
            we = engine.pack_masks(me, n)
            for take in (64, 66, 1, RB):
                cfg = (1, 0, take, take)
                for name in names:
                    what = "edges %s %s take %d" % (metric, name, take)
                    gi, gd = idx.lsh_search_filtered(Q, 70, engine.pack_mask(masks[name], n), *cfg)
                    ei, ed = F.search_batch(D, qcodes, off, ids, 4, 70, *cfg, masks[name])
                    assert_exact(gi, gd, ei, ed, what)
                    _passing_only(gi, masks[name], what)
                    assert [int((g >= 0).sum()) for g in gi] == [min(c, take) for c in passing[name]], what
                gi, gd = idx.lsh_search_filtered_each(Qe, 70, we, *cfg)
                ei, ed = F.search_batch(De, qce, off, ids, 4, 70, *cfg, me)
                assert_exact(gi, gd, ei, ed, "edges each %s take %d" % (metric, take))
                assert [int((g >= 0).sum()) for g in gi] == [min(passing[name][b], take) for b in range(len(sizes)) for name in names]
            cfg = (1, 4, 66, 64)   # radius 4: both key stores in one launch
            for name in names:
                gi, gd = idx.lsh_search_filtered(Q, 256, engine.pack_mask(masks[name], n), *cfg)
                ei, ed = F.search_batch(D, qcodes, off, ids, 4, 256, *cfg, masks[name])
                assert_exact(gi, gd, ei, ed, "edges flips %s %s" % (metric, name))
            gi, gd = idx.lsh_search_filtered_each(Qe, 256, we, *cfg)
            ei, ed = F.search_batch(De, qce, off, ids, 4, 256, *cfg, me)
            assert_exact(gi, gd, ei, ed, "edges flips each %s" % metric)


@pytest.mark.parametrize("metric,bits", [("cosine", 4), ("l2", 12)])
def test_each_equals_the_singles(native_lib, oracle, data2000, codes2000, masks2000, dense2000, metric, bits):
    """33 queries, 5 distinct masks interleaved (all-zeros and all-ones among them): row q is the single-mask call of (query q,
    mask q), and the model's."""
    from hnsw_clj_amd import engine

    O = oracle
    base, Q = data2000
    _, codes, qcodes = codes2000
    codes, qcodes = codes & ((1 << bits) - 1), qcodes & ((1 << bits) - 1)
    off, ids = M.buckets(codes, bits)
    D = dense2000(metric, O.MODE_DEV)
    which = [MASK_NAMES[q % 5] for q in range(NQ)]
    each = np.stack([masks2000[w] for w in which])
    words = engine.pack_masks(each, N)
    with engine.Index(base, metric, 0) as idx:
        idx.lsh_build(8, bits, 64, 42)
        for cfg in (CONFIGS[2], CONFIGS[4], CONFIGS[5]):
            gi, gd = idx.lsh_search_filtered_each(Q, K, words, *cfg)
            ei, ed = F.search_batch(D, qcodes, off, ids, bits, K, *cfg, each)
            assert_exact(gi, gd, ei, ed, "each %s %s" % (metric, cfg))
            for q in range(NQ):
                si, sd = idx.lsh_search_filtered(Q[q:q + 1], K, words[q], *cfg)
                assert _bits_equal((gi[q:q + 1], gd[q:q + 1]), (si, sd)), (metric, cfg, q)
                _passing_only(gi[q], each[q])
            assert (gi[4::5] == -1).all()                                                # the all-zeros rows
            want = idx.lsh_search(Q, K, *cfg)
            assert _bits_equal((gi[3::5], gd[3::5]), (want[0][3::5], want[1][3::5]))       # the all-ones rows


def test_dev_entries(native_lib, data2000, masks2000):
    """Torch tensors for the queries, the mask and the outputs on a stream of the caller's: the host entries' results."""
    import torch

    from hnsw_clj_amd import engine

    base, Q = data2000
    dev = torch.device("cuda", 0)
    each = np.stack([masks2000[MASK_NAMES[q % 5]] for q in range(NQ)])
    words1 = engine.pack_mask(masks2000["p10"], N)
    words = engine.pack_masks(each, N)
    with engine.Index(base, "cosine", 0) as idx:
        idx.lsh_build(8, 4, 64, 42)
        for cfg in (CONFIGS[2], (2, 1, 66, 64)):
            host1 = idx.lsh_search_filtered(Q, K, words1, *cfg)
            host = idx.lsh_search_filtered_each(Q, K, words, *cfg)
            s = torch.cuda.Stream(dev)
            with torch.cuda.stream(s):
                tq = torch.from_numpy(Q).to(dev)
                t1 = torch.from_numpy(words1.view(np.int32)).to(dev)
                te = torch.from_numpy(words.view(np.int32)).to(dev)
                out = (torch.empty((NQ, K), dtype=torch.int32, device=dev), torch.empty((NQ, K), dtype=torch.float32, device=dev))
                di, dd = idx.lsh_search_filtered(tq, K, t1, *cfg, out=out)
                assert di is out[0] and dd is out[1]
                ei, ed = idx.lsh_search_filtered_each(tq, K, te, *cfg)
            s.synchronize()
            assert _bits_equal(host1, (di.cpu().numpy(), dd.cpu().numpy())), cfg
            assert _bits_equal(host, (ei.cpu().numpy(), ed.cpu().numpy())), cfg


def test_state_and_errors(native_lib, oracle, data2000):
    from hnsw_clj_amd import engine
    from hnsw_clj_amd._native import HnswGpuError

    O = oracle
    base, Q = data2000
    n0, m = 600, 101
    n1 = n0 + m
    rows = base[:n1]
    cfg = CONFIGS[2]
    L = native_lib.lib()

    def code_of(fn):
        with pytest.raises(HnswGpuError) as e:
            fn()
        return e.value.code

    def raw(idx, nq, k, take_main, take_flip, allow, each=False):
        gi, gd = np.empty((max(nq, 1), k), np.int32), np.empty((max(nq, 1), k), np.float32)
        fn = L.hnswgpu_lsh_search_filtered_each if each else L.hnswgpu_lsh_search_filtered
        return fn(idx._h, engine._p(Q), nq, k, 6, 2, take_main, take_flip, engine._p(allow), engine._p(gi), engine._p(gd))

    with engine.Index(rows[:n0], "cosine", 0) as idx:
        ones0 = engine.pack_mask(np.ones(n0, np.bool_), n0)
        # a handle without tables
        assert code_of(lambda: idx.lsh_search_filtered(Q, K, ones0)) == -3
        assert code_of(lambda: idx.lsh_search_filtered_each(Q, K, np.tile(ones0, (NQ, 1)))) == -3
        idx.lsh_build(8, 5, 64, 42)
        # arguments and limits
        for each in (False, True):
            allow = np.tile(ones0, (NQ, 1)) if each else ones0
            assert raw(idx, NQ, K, 20, 10, None, each) == -1 and b"allow is null" in L.hnswgpu_last_error()
            assert raw(idx, NQ, 257, 20, 10, allow, each) == -5
            assert raw(idx, NQ, K, 257, 10, allow, each) == -5 and raw(idx, NQ, K, 20, 257, allow, each) == -5
            assert raw(idx, NQ, 0, 20, 10, allow, each) == -1 and raw(idx, NQ, K, 0, 10, allow, each) == -1
            assert raw(idx, 0, K, 20, 10, allow, each) == 0 and raw(idx, 0, K, 20, 10, None, each) == 0
        before = idx.lsh_search_filtered(Q, K, ones0, *cfg)
        assert _bits_equal(before, idx.lsh_search(Q, K, *cfg))
        # rows join: the next call brings a longer mask (the mask is an argument, nothing of it is kept)
        idx.lsh_add(rows[n0:])
        assert idx.n == n1
        with pytest.raises(ValueError):
            idx.lsh_search_filtered(Q, K, ones0, *cfg)
        _, codes, off, ids = idx.lsh_get()
        qcodes = idx.lsh_hash(Q)
        D = _dense(O, rows, Q, "cosine", O.MODE_DEV)
        rng = np.random.default_rng(9)
        new = np.arange(n1) >= n0
        for name, allow in (("random", rng.random(n1) < 0.4), ("old only", ~new), ("new only", new)):
            gi, gd = idx.lsh_search_filtered(Q, K, engine.pack_mask(allow, n1), *cfg)
            ei, ed = F.search_batch(D, qcodes, off, ids, 5, K, *cfg, allow)
            assert_exact(gi, gd, ei, ed, "grown, " + name)
            _passing_only(gi, allow, name)
            assert (gi >= 0).any()
        gi, _ = idx.lsh_search_filtered(Q, K, engine.pack_mask(~new, n1), *cfg)
        assert (gi < n0).all()
        gi, _ = idx.lsh_search_filtered(Q, K, engine.pack_mask(new, n1), *cfg)
        assert ((gi >= n0) | (gi == -1)).all() and (gi >= n0).any()
    with engine.Index(np.zeros((0, 16), np.float32), "l2", 0) as empty:
        empty.lsh_build()
        Q16 = np.ones((3, 16), np.float32)
        gi, gd = empty.lsh_search_filtered(Q16, 4, np.zeros(0, np.uint32))
        assert (gi == -1).all() and np.isinf(gd).all()
        gi, gd = empty.lsh_search_filtered_each(Q16, 4, np.zeros((3, 0), np.uint32))
        assert (gi == -1).all() and np.isinf(gd).all()


def test_mirror(native_lib, data2000):
    from hnsw_clj_amd import engine
    from hnsw_clj_amd import hybrid_lsh as H
    from hnsw_clj_amd import protocol

    base, Q = data2000
    n = 500
    index = H.build_index([["v%d" % i, v] for i, v in enumerate(base[:n])], show_progress=False)
    try:
        third = lambda i: int(i[1:]) % 3 == 0
        rest = lambda i: int(i[1:]) % 3 != 0
        b3 = np.arange(n) % 3 == 0
        names = lambda ids: [["v%d" % i for i in row if i >= 0] for row in ids]
        for mode, (probes, radius) in H.MODE_CONFIGS.items():
            ids, d = index.index.lsh_search_filtered(Q[:4], K, engine.pack_mask(b3, n), probes, radius, 2 * K, K)
            got = H.search_batch_filtered(index, Q[:4], K, third, mode)
            assert [[r["id"] for r in rs] for rs in got] == names(ids)
            assert [[r["distance"] for r in rs] for rs in got] == [[float(x) for x, i in zip(dr, ir) if i >= 0] for dr, ir in zip(d, ids)]
            assert H.search_knn_filtered(index, Q[0], K, third, mode) == got[0]
            assert H.search_batch_filtered(index, Q[:4], K, b3, mode) == got              # a ready bool array
        fns = [third, rest, third, b3, rest]
        ids, _ = index.index.lsh_search_filtered_each(Q[:5], K, engine.pack_masks([b3, ~b3, b3, b3, ~b3], n), 6, 2, 2 * K, K)
        got = H.search_batch_filtered_each(index, Q[:5], K, fns)
        assert [[r["id"] for r in rs] for rs in got] == names(ids)
        assert all(H.search_knn_filtered(index, Q[q], K, fns[q]) == got[q] for q in range(5))
        p = protocol.GpuFilterableHybridLshIndex(index)
        assert protocol.supports_filtering(p) and not protocol.supports_filtering(protocol.GpuHybridLshIndex(index))
        assert p.search_knn_filtered_star(Q[1], K, rest, "fast") == H.search_knn_filtered(index, Q[1], K, rest, "fast")
        assert p.search_batch_filtered(Q[:5], K, fns) == got
    finally:
        index.close()
    # The hand example that separates the two classes: lsh_model's rows, k = 2, :turbo (both tables, bit 0 flipped), only the far
    # rows 2 and 3 pass.
    #   filtered class (takes 4 / 2 over the passing rows): table 0 own [0, 1, 2] -> [2], flipped [3, 4, 6] -> [3]; table 1 own
    #     [0, 1, 3, 4, 5, 6] -> [3], flipped [2] -> [2]; stream 2 3 | 3 2 -> [2, 3]
    #   plain class (default_filtered_search: search 3 k = 6 with takes 12 / 6, every bucket whole): distinct 0 1 2 3 4 6 5 ->
    #     sorted 0 1 4 6 5 2 3 -> cut to 6: row 3 is gone before the predicate is asked -> [2]
    hand = H.build_index([["r%d" % i, v] for i, v in enumerate(M.HAND_ROWS)], distance_fn=_euclid(), show_progress=False)
    try:
        hand.index.set_lsh(M.HAND_PLANES)
        far = lambda i: i in ("r2", "r3")
        plain = protocol.default_filtered_search(protocol.GpuHybridLshIndex(hand), M.HAND_QUERY, 2, far, "turbo")
        filt = protocol.GpuFilterableHybridLshIndex(hand).search_knn_filtered_star(M.HAND_QUERY, 2, far, "turbo")
        assert [r["id"] for r in plain] == ["r2"] and [r["id"] for r in filt] == ["r2", "r3"]
    finally:
        hand.close()


def _euclid():
    from hnsw_clj_amd import ultra_fast

    return ultra_fast.euclidean_distance_ultra
