"""The index file (hnswgpu_save / hnswgpu_load, hnsw-clj_amd/csrc/persist.hip) against a reader and a writer that are not the
product's: tests/index_file.py restates the documented layout in numpy, and the CPU oracle searches what that reader parsed.

  a. a file the product did not write loads, exports what was written and searches with the oracle's bits
  b. a file the product wrote, parsed without the product, holds what the handle held; the oracle on the PARSED arrays is the
     reference of the loaded handle's searches (and of the saved one's); c. saving is byte-stable
  d. the life cycle build -> save -> load -> add: a loaded graph keeps its builder (the header's builder word)
  e. n = 0 and n = 1; f. damaged bodies are refused by the host-side validation, each by the check that is there for it

Every comparison is bit for bit: ids, distance bits, traversal counters, file bytes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_file as IF  # noqa: E402
from util import assert_exact  # noqa: E402

pytestmark = pytest.mark.gpu

M, EFC, SEED = 8, 40, 42
K, EF, NLIST, NPROBE = 10, 60, 6, 2
NQS = (1, 33)                # one query; a batch (exact kNN: the MFMA tile scan from 16 queries on)
IVF_NQS = (1, 33, 40)        # 40 x 2 (query, list) pairs > 12 x 6: past the tile boundary the suite pins (HNSWGPU_TILE_PAIRS=12)
NQ_WAVE = 130                # more than the 128 queries of a small launch: the wave kernel can be forced
METRICS = ["cosine", "l2", "dot"]
BUILDERS = {"closest": {}, "heuristic": dict(heuristic=True), "heuristic+symmetric": dict(heuristic=True, symmetric=True),
            "heuristic+extend": dict(heuristic=True, extend=True), "sequential": dict(sequential=True)}
BUILDER_WORD = {"closest": 0, "sequential": 1, "heuristic": 2, "heuristic+symmetric": 2 | 4, "heuristic+extend": 2 | 8}


@pytest.fixture(scope="module")
def eng(native_lib):
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    return engine


def _data(O, n, dim, dist="gaussian", seed=42, **kw):
    return O.generate_dataset(n, dim, dist, seed=seed, **kw).astype(np.float32)


def _graph_of(O, f):
    """The oracle's graph from parsed file sections (or from an engine export)."""
    if isinstance(f, dict):
        return O.Graph(f["levels"], f["l0_adj"], f["up_off"], f["up_adj"], f["M"], f["entry"], f["max_level"])
    return O.Graph(f.levels, f.l0_adj.reshape(-1, f.M0), f.up_off, f.up_adj, f.M, f.entry, f.max_level)


def _same_graph(g, og, what):
    np.testing.assert_array_equal(g.levels, og.levels, err_msg=what + ": levels")
    assert (g.entry, g.max_level, g.M, g.M0) == (og.entry, og.max_level, og.M, og.M0), what
    np.testing.assert_array_equal(g.up_off, og.up_off, err_msg=what + ": up_off")
    a, b = np.asarray(g.l0_adj).reshape(-1, og.M0), np.asarray(og.l0_adj).reshape(-1, og.M0)
    assert a.shape == b.shape == (len(og.levels), og.M0), what
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert bad.size == 0, "%s: %d layer-0 rows differ, first at node %d: %s against %s" % (what, bad.size, bad[0], a[bad[0]], b[bad[0]])
    np.testing.assert_array_equal(np.ravel(g.up_adj), np.ravel(og.up_adj), err_msg=what + ": upper layers")


def _oracle_answers(O, base, om, Q, graph=None, lists=None):
    """What the three searches must return, from the oracle in the arithmetic of the kernel that serves each batch."""
    ans = {}
    for nq in NQS:
        mode = O.MODE_MFMA if (om != O.L2 and nq >= 16) else O.MODE_DEV
        ans["exact", nq] = O.exact_knn(base, Q[:nq], K, metric=om, mode=mode)[:2]
    if graph is not None:
        for nq in NQS + (NQ_WAVE,):
            ans["hnsw", nq] = O.hnsw_search(base, graph, Q[:nq], K, ef=EF, metric=om, mode=O.MODE_DEV)[:3]
    if lists is not None:
        cen, off, lids = lists
        for nq in IVF_NQS:
            tiled = om != O.L2 and nq * min(NPROBE, len(cen)) > 12 * len(cen)
            ans["ivf", nq] = O.ivf_search(base, cen, off, lids, Q[:nq], K, NPROBE, metric=om,
                                          mode=O.MODE_MFMA if tiled else O.MODE_DEV)[:2]
    return ans


def _handle_answers(eng, tune, h, Q, keys):
    """The same searches on a handle; the 130-query HNSW batch runs with the wave kernel forced (it must have run)."""
    got = {}
    for kind, nq in keys:
        if kind == "exact":
            got[kind, nq] = h.exact_knn(Q[:nq], K)
        elif kind == "ivf":
            got[kind, nq] = h.ivf_search(Q[:nq], K, NPROBE)
        elif nq == NQ_WAVE:
            tune.set("HNSW_WAVE", 2)
            before = eng.debug_counter("hnsw_wave")
            got[kind, nq] = h.hnsw_search(Q[:nq], K, EF, want_stats=True)
            assert eng.debug_counter("hnsw_wave") > before, "the wave kernel did not run"
            tune.restore()
        else:
            got[kind, nq] = h.hnsw_search(Q[:nq], K, EF, want_stats=True)
    return got


def _assert_answers(got, ans, what):
    assert got.keys() == ans.keys()
    for key, want in ans.items():
        w = "%s: %s, %d queries" % (what, key[0], key[1])
        assert_exact(got[key][0], got[key][1], want[0], want[1], w)
        if key[0] == "hnsw":
            np.testing.assert_array_equal(got[key][2], want[2], err_msg=w + ": traversal counters")


def _assert_handles_agree(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        for x, y in zip(a[key], b[key]):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "%s: %s differs" % (what, key)


def _ragged_lists(O, rs, n, dim):
    assign = rs.integers(0, NLIST, n)
    assign[assign == 4] = 5                                    # an empty list, and lists of unequal lengths
    off, lids = O.lists_from_assign(assign, NLIST)
    assert off[4] == off[5] and len(set(np.diff(off).tolist())) > 2
    return _data(O, NLIST, dim, seed=77), off, lids


def _no_tmp(tmp_path):
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")], "a temporary file was left behind"


# ---- a. a file the product did not write -----------------------------------------------------------------------------
def _foreign_file(O, path, om, n=300, dim=24, **header):
    """Rows, an oracle-built graph and oracle-built lists, written by the numpy writer."""
    base = _data(O, n, dim)
    g = O.hnsw_build_ex(base, om, M, EFC, SEED, 0, mode=O.MODE_DEV)
    _, cen, assign = O.ivf_build_dev(base, NLIST, 3, om, SEED)
    off, lids = O.lists_from_assign(assign, NLIST)
    sections = dict(levels=g.levels, l0_adj=g.l0_adj, up_off=g.up_off, up_adj=g.up_adj, M=g.M, entry=g.entry,
                    max_level=g.max_level, centroids=cen, list_off=off, list_ids=lids)
    IF.write_index_file(path, base, om, **dict(sections, **header))
    return base, g, (cen, off, lids), sections


@pytest.mark.parametrize("metric", METRICS)
def test_a_file_written_without_the_product_loads_and_searches(eng, oracle, tune, tmp_path, metric):
    O = oracle
    om = O.METRICS[metric]
    path = str(tmp_path / "foreign.bin")
    base, g, lists, _ = _foreign_file(O, path, om)
    Q = np.vstack([_data(O, NQ_WAVE - 2, 24, seed=43), base[:2]])
    with eng.Index.load(path) as idx:
        assert (idx.n, idx.dim, idx.metric, idx.nlist, idx.has_graph) == (300, 24, om, NLIST, True)
        _same_graph(idx.get_graph(), g, "export of the loaded handle against what was written")
        for got, want, name in zip(idx.get_ivf(), lists, ("centroids", "list_off", "list_ids")):
            assert got.dtype == want.dtype and got.tobytes() == np.ascontiguousarray(want).tobytes(), name
        np.testing.assert_array_equal(idx.norms().view(np.uint32), O.norms(base, O.MODE_DEV).view(np.uint32))
        ans = _oracle_answers(O, base, om, Q, g, lists)
        _assert_answers(_handle_answers(eng, tune, idx, Q, ans.keys()), ans, "numpy-written file, %s" % metric)


# ---- b. + c. a file the product wrote, read without the product ------------------------------------------------------
STATES = ["bare", "closest", "heuristic", "sequential", "ivf", "closest+ivf"]


@pytest.mark.parametrize("dim", [24, 30, 300])       # rows unpadded; rows padded to 32; rows wider than one wave's chunk
@pytest.mark.parametrize("metric", METRICS)
def test_a_saved_file_read_without_the_product(eng, oracle, tune, tmp_path, metric, dim):
    O = oracle
    om = O.METRICS[metric]
    n = 400
    base = _data(O, n, dim, "clustered", num_clusters=8, noise_level=0.4)
    Q = np.vstack([_data(O, NQ_WAVE - 2, dim, "clustered", num_clusters=8, noise_level=0.4, seed=43), base[:2]])
    lists_in = _ragged_lists(O, np.random.default_rng(21), n, dim)
    for state in STATES:
        what = "%s, dim %d, %s" % (metric, dim, state)
        builder = state.split("+")[0] if state.split("+")[0] in BUILDERS else None
        has_ivf = state.endswith("ivf")
        path, again, path2 = (str(tmp_path / (state + s)) for s in (".bin", ".again.bin", ".resaved.bin"))
        with eng.Index(base, metric) as idx:
            if builder:
                idx.hnsw_build(M, EFC, SEED, **BUILDERS[builder])
            if has_ivf:
                idx.set_ivf(*lists_in)
            idx.save(path)
            idx.save(again)
            f = IF.read_index_file(path)                     # ---- the file, read by a third party
            flags = (1 if builder else 0) | (2 if has_ivf else 0)
            assert (f["metric"], f["n"], f["dim"], f["flags"]) == (om, n, dim, flags), what
            assert f["base"].shape == (n, dim) and f["base"].tobytes() == base.tobytes(), what + ": base rows"
            g = lists = None
            up_blocks = 0
            if builder:
                g = idx.get_graph()
                up_blocks = len(g.up_adj) // M
                _same_graph(_graph_of(O, f), g, what + ": graph sections against get_graph()")
                assert (f["M"], f["M0"], f["up_blocks"], f["builder"]) == (M, 2 * M, up_blocks, BUILDER_WORD[builder]), what
                assert f["up_off"][-1] == up_blocks and f["levels"][f["entry"]] == f["max_level"] == f["levels"].max()
            else:
                assert f["builder"] == 0, what
            if has_ivf:
                lists = idx.get_ivf()
                for key, got, put in zip(("centroids", "list_off", "list_ids"), lists, lists_in):
                    assert f[key].tobytes() == got.tobytes() == np.ascontiguousarray(put).tobytes(), what + ": " + key
            assert f["nlist"] == (NLIST if has_ivf else 0), what
            size = IF.expected_size(n, dim, flags, M if builder else 0, 2 * M if builder else 0, up_blocks, NLIST if has_ivf else 0)
            assert f["size"] == os.path.getsize(path) == size, what + ": file size"
            # ---- the oracle on the PARSED arrays is the reference of the loaded handle (and of the saved one)
            fl = (f["centroids"], f["list_off"], f["list_ids"]) if has_ivf else None
            ans = _oracle_answers(O, f["base"], f["metric"], Q, _graph_of(O, f) if builder else None, fl)
            with eng.Index.load(path) as back:
                assert (back.n, back.dim, back.metric, back.nlist, back.has_graph) == (n, dim, om, f["nlist"], bool(builder)), what
                got_back = _handle_answers(eng, tune, back, Q, ans.keys())
                _assert_answers(got_back, ans, what + ", loaded handle")
                got_saved = _handle_answers(eng, tune, idx, Q, ans.keys())
                _assert_answers(got_saved, ans, what + ", saved handle")
                _assert_handles_agree(got_saved, got_back, what + ": saved against loaded handle")
                assert back.norms().tobytes() == idx.norms().tobytes(), what + ": norms"
                if builder:
                    _same_graph(back.get_graph(), g, what + ": get_graph() of the loaded handle")
                if has_ivf:
                    for a, b in zip(back.get_ivf(), lists):
                        assert a.tobytes() == b.tobytes(), what + ": get_ivf() of the loaded handle"
                back.save(path2)                             # ---- c. byte stability
            raw = open(path, "rb").read()
            assert open(again, "rb").read() == raw, what + ": two saves of one handle differ"
            assert open(path2, "rb").read() == raw, what + ": save(load(f)) differs from f"
    _no_tmp(tmp_path)


# ---- d. the life cycle: build -> save -> load -> add ----------------------------------------------------------------
@pytest.mark.parametrize("builder", ["closest", "heuristic", "heuristic+symmetric", "heuristic+extend"])
def test_a_loaded_graph_grows_as_the_built_one(eng, oracle, tune, tmp_path, builder):
    """Handle A: build, add.  Handle B: build, save, load, the same adds.  Handle C: A after its adds, saved and loaded.  B's
    graph must equal A's edge for edge -- the file carries the builder, hnswgpu_hnsw_add on the loaded handle links by it --
    and C must be A.  500 rows and 200 more in calls of 1, 64 and 135; with java.util.Random(42)'s draws row 571 gets a
    level above every earlier row, so the adds also move the entry point and raise max_level."""
    O = oracle
    n0, n1, dim = 500, 700, 24
    base = _data(O, n1, dim, "clustered")
    Q = np.vstack([_data(O, NQ_WAVE - 2, dim, "clustered", seed=43), base[n0:n0 + 2]])
    r = O.JavaRandom(SEED)
    draws = np.array([min(int((1.0 / np.log(2.0)) * -np.log(r.next_double())), 30) for _ in range(n1)])
    assert draws[571] > draws[:571].max() and draws[571] == draws.max(), "the data of this test: row 571 must top every level"
    p0, p1, p2 = (str(tmp_path / name) for name in ("built.bin", "grown.bin", "grown_resaved.bin"))

    def grow(h):
        pos = n0
        for take in (1, 64, n1 - n0 - 65):
            ids = h.hnsw_add(base[pos:pos + take], EFC, SEED)
            assert ids[0] == pos and len(ids) == take
            pos += take
        assert pos == n1 and h.n == n1
        return h.get_graph()

    with eng.Index(base[:n0], "cosine") as A:
        A.hnsw_build(M, EFC, SEED, **BUILDERS[builder])
        g0 = A.get_graph()
        A.save(p0)
        with eng.Index.load(p0) as B:
            _same_graph(B.get_graph(), g0, "%s: the loaded graph before the adds" % builder)
            gA = grow(A)
            gB = grow(B)
            np.testing.assert_array_equal(gA.levels, draws)
            assert gA.entry == 571 != g0.entry and gA.max_level == draws[571] > g0.max_level, "the adds must move the entry point"
            _same_graph(gB, gA, "%s: build, save, load, add against build, add" % builder)
            assert IF.read_index_file(p0)["builder"] == BUILDER_WORD[builder]      # (how the file told B: the header's last word)
            A.save(p1)
            f1 = IF.read_index_file(p1)
            assert (f1["n"], f1["entry"], f1["max_level"], f1["builder"]) == (n1, 571, draws[571], BUILDER_WORD[builder])
            assert f1["base"].tobytes() == base.tobytes()
            with eng.Index.load(p1) as C:
                assert C.n == n1
                _same_graph(C.get_graph(), gA, "%s: the grown handle, saved and loaded" % builder)
                ans = {("hnsw", nq): O.hnsw_search(base, _graph_of(O, gA), Q[:nq], K, ef=EF, mode=O.MODE_DEV)[:3]
                       for nq in NQS + (NQ_WAVE,)}
                for name, h in (("A", A), ("B", B), ("C", C)):
                    _assert_answers(_handle_answers(eng, tune, h, Q, ans.keys()), ans, "%s: handle %s" % (builder, name))
                C.save(p2)
    assert open(p2, "rb").read() == open(p1, "rb").read(), "C's file differs from A's second save"
    _no_tmp(tmp_path)


# ---- e. degenerate sizes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_empty_and_single_row_indexes_round_trip(eng, oracle, tmp_path, metric):
    O = oracle
    om = O.METRICS[metric]
    dim = 24
    Q = _data(O, 5, dim, seed=43)
    one = _data(O, 1, dim, seed=9)
    cen = _data(O, 2, dim, seed=77)
    none = np.zeros((0, dim), np.float32)

    def fill_only(ids, d, have=0):
        return (ids[:, have:] == -1).all() and np.isposinf(d[:, have:]).all()

    for state in ("bare", "graph", "ivf", "graph+ivf"):
        for n, base in ((0, none), (1, one)):
            what = "%s, n = %d, %s" % (metric, n, state)
            path = str(tmp_path / ("%s_%d.bin" % (state.replace("+", "_"), n)))
            graph, ivf = "graph" in state, "ivf" in state
            with eng.Index(base, metric) as idx:
                if graph:
                    idx.hnsw_build(M, EFC, SEED)
                if ivf:
                    idx.set_ivf(cen, np.array([0, 0, n], np.int64), np.arange(n, dtype=np.int32))   # n = 0: all-zero offsets
                g = idx.get_graph() if graph else None
                idx.save(path)
            f = IF.read_index_file(path)
            flags = (1 if graph else 0) | (2 if ivf else 0)
            up_blocks = int(g.up_off[-1]) if graph else 0          # (a single row may draw an upper level)
            assert f["size"] == IF.expected_size(n, dim, flags, M if graph else 0, 2 * M if graph else 0, up_blocks, 2 if ivf else 0), what
            assert (f["n"], f["dim"], f["metric"], f["flags"], f["nlist"]) == (n, dim, om, flags, 2 if ivf else 0), what
            assert f["base"].tobytes() == base.tobytes(), what
            if graph:
                assert (f["M"], f["M0"], f["up_blocks"], f["max_level"], f["entry"]) == (M, 2 * M, up_blocks, g.max_level, 0 if n else -1), what
                _same_graph(_graph_of(O, f), g, what + ": graph sections against get_graph()")
                assert (f["l0_adj"] == -1).all() and (f["up_adj"] == -1).all(), what
            with eng.Index.load(path) as back:
                assert (back.n, back.dim, back.metric, back.nlist, back.has_graph) == (n, dim, om, f["nlist"], graph), what
                assert back.norms().tobytes() == (O.norms(base, O.MODE_DEV).astype(np.float32).tobytes() if n else b""), what
                results = [back.exact_knn(Q, 3)]
                if graph:
                    results.append(back.hnsw_search(Q, 3, 20))
                if ivf:
                    results.append(back.ivf_search(Q, 3, 2))
                    ii, dd, pr = back.ivf_search(Q, 3, 2, want_probes=True)
                    results.append((ii, dd))
                    if n == 0:
                        assert (pr == -1).all(), what + ": no list of an empty index is scanned"
                want = np.array([O.distance_dev(om, q, one[0]) for q in Q], np.float32)
                for ids, d in results:
                    assert fill_only(ids, d, have=n), what + ": the -1 / +inf fill"
                    if n == 1:
                        assert (ids[:, 0] == 0).all() and d[:, 0].tobytes() == want.tobytes(), what
                back.save(path + ".resaved")
            assert open(path + ".resaved", "rb").read() == open(path, "rb").read(), what
    _no_tmp(tmp_path)


@pytest.mark.parametrize("builder", ["closest", "heuristic"])
def test_rows_added_to_a_loaded_empty_graph(eng, oracle, tmp_path, builder):
    """An empty index with an (empty) graph, saved and loaded, takes its first 40 rows as the same handle does without the
    file between: the first row becomes the entry point, the rest are linked by the builder the empty graph was made with."""
    O = oracle
    dim = 24
    rows = _data(O, 40, dim, "clustered", num_clusters=4, noise_level=0.3)
    Q = _data(O, 5, dim, seed=43)
    path = str(tmp_path / "empty_graph.bin")
    with eng.Index(np.zeros((0, dim), np.float32), "cosine") as A:
        A.hnsw_build(M, EFC, SEED, **BUILDERS[builder])
        A.save(path)
        with eng.Index.load(path) as B:
            for h in (A, B):
                assert h.hnsw_add(rows[:1], EFC, SEED).tolist() == [0]
                assert h.hnsw_add(rows[1:], EFC, SEED).tolist() == list(range(1, 40))
            gA, gB = A.get_graph(), B.get_graph()
            _same_graph(gB, gA, "40 rows added to a loaded empty graph (%s)" % builder)
            assert IF.read_index_file(path)["builder"] == BUILDER_WORD[builder]
            assert gA.levels[gA.entry] == gA.max_level == gA.levels.max() and (gA.l0_adj.reshape(40, -1)[:, 0] >= 0).all()
            oi, od, ost, _ = O.hnsw_search(rows, _graph_of(O, gA), Q, K, ef=EF, mode=O.MODE_DEV)
            for h in (A, B):
                ids, d, st = h.hnsw_search(Q, K, EF, want_stats=True)
                assert_exact(ids, d, oi, od, "search of the grown empty graph")
                np.testing.assert_array_equal(st, ost)
            with eng.Index(rows, "cosine") as chk:            # the validator accepts what the adds made
                chk.set_graph(gA)


# ---- f. damaged bodies -----------------------------------------------------------------------------------------------
def _damage_cases(sections, n):
    """name -> (message of the check that must catch it, damaged sections, header fields to state).  One field wrong each."""
    lv, l0, up_off, up_adj = (np.array(sections[k]) for k in ("levels", "l0_adj", "up_off", "up_adj"))
    entry, top = sections["entry"], sections["max_level"]
    flat = int(np.nonzero(lv == 0)[0][0])                     # a node on layer 0 only
    tall = int(np.nonzero((lv >= 1) & (np.arange(n) != entry))[0][0])   # a node with an upper layer, not the entry point
    cases = {}

    def case(name, message, header=None, **changed):
        cases[name] = (message, dict(sections, **changed), header or {})

    def put(a, i, v):
        a = a.copy()
        a.reshape(-1)[i] = v
        return a

    case("a negative level", "node %d has a negative level" % flat, levels=put(lv, flat, -1))
    # a level above max_level, with up_off, up_adj and the header's up_blocks telling the same story: only the level is wrong
    lv_hi = put(lv, flat, top + 1)
    off_hi = np.concatenate([[0], np.cumsum(lv_hi)]).astype(np.int64)
    adj_hi = np.insert(up_adj.reshape(-1, M), [int(up_off[flat])] * (top + 1), -1, axis=0).reshape(-1)
    case("a level above max_level", "node %d level > max_level" % flat, levels=lv_hi, up_off=off_hi, up_adj=adj_hi)
    case("entry = n", "entry out of range", entry=n)
    case("entry = -1", "entry out of range", entry=-1)
    case("the entry's level below max_level", "entry level < max_level", max_level=top + 1)
    case("a negative max_level", "entry level < max_level", max_level=-1)
    case("a level-0 edge = n", "l0_adj entry out of range", l0_adj=put(l0, 3 * 2 * M + 1, n))
    case("a level-0 edge = -2", "l0_adj entry out of range", l0_adj=put(l0, 5 * 2 * M, -2))
    case("an upper edge = n", "up_adj entry out of range", up_adj=put(up_adj, int(up_off[tall]) * M, n))
    case("an upper edge to a node without that layer", r"edge %d->%d on layer 1: target has no such layer" % (tall, flat),
         up_adj=put(up_adj, int(up_off[tall]) * M, flat))
    case("up_off[0] = 1", r"up_off\[0\] != 0", up_off=put(up_off, 0, 1))
    mid = int(np.nonzero(lv[:-1] >= 1)[0][0])                 # up_off[mid + 1] is not the last entry: the header still agrees
    case("up_off not the prefix sum of levels", "up_off is not the prefix sum of levels at node %d" % mid,
         up_off=put(up_off, mid + 1, up_off[mid + 1] + 1))
    case("up_off ends elsewhere than the header says", "up_off ends at", header=dict(up_blocks=int(up_off[-1])),
         up_off=put(up_off, n, up_off[n] + 1))
    off, ids = np.array(sections["list_off"]), np.array(sections["list_ids"])
    case("list_off[0] = 1", "list_off must start at 0 and end at n", list_off=put(off, 0, 1))
    case("list_off not monotone", "list_off not monotone", list_off=put(off, 1, off[2] + 1))
    case("list_off[nlist] != n", "list_off must start at 0 and end at n", list_off=put(off, len(off) - 1, n - 1))
    case("a list id = n", r"list_ids\[7\] out of range", list_ids=put(ids, 7, n))
    case("a list id = -1", r"list_ids\[0\] out of range", list_ids=put(ids, 0, -1))
    case("a row in two lists", "row %d is in two lists" % ids[0], list_ids=put(ids, 1, ids[0]))
    return cases


def test_damaged_bodies_are_refused_by_the_check_that_is_there_for_them(eng, oracle, tune, tmp_path):
    """Valid numpy-written files of 40 rows with ONE field of the body wrong each: hnswgpu_load must refuse every one on the
    host (hnswgpu_set_graph's and validate_lists' checks; nothing of a damaged file reaches a kernel: the test only loads),
    with the message of the check that is there for it.  The undamaged file loads and searches with the oracle's bits
    afterwards."""
    O = oracle
    n = 40
    good = str(tmp_path / "good.bin")
    base, g, lists, sections = _foreign_file(O, good, O.COSINE, n=n)
    assert g.max_level >= 1 and (g.levels >= 1).sum() >= 3
    cases = _damage_cases(sections, n)
    assert len(cases) == 19
    for name, (message, damaged, header) in cases.items():
        path = str(tmp_path / "damaged.bin")
        IF.write_index_file(path, base, O.COSINE, **dict(damaged, **header))
        assert IF.unpack_header(open(path, "rb").read())["n"] == n
        with pytest.raises(eng._native.HnswGpuError, match=message) as e:
            eng.Index.load(path).close()
        assert e.value.code == -1, name                                      # HNSWGPU_EINVAL
    Q = np.vstack([_data(O, NQ_WAVE - 2, 24, seed=43), base[:2]])
    with eng.Index.load(good) as idx:
        ans = _oracle_answers(O, base, O.COSINE, Q, g, lists)
        _assert_answers(_handle_answers(eng, tune, idx, Q, ans.keys()), ans, "the undamaged file, after the damaged ones")
