"""A forest on one handle (include/hnswgpu.h: hnswgpu_set_graph_parts / hnswgpu_hnsw_build_parts / hnswgpu_hnsw_search_parts):
the reference's indexes of many small graphs (partitioned_hnsw.clj:149-196, ivf_hnsw.clj:286-325) searched in ONE traversal launch.

The contract is stated against what exists: item (query q, probe p) holds bit for bit what hnswgpu_hnsw_search returns on a handle
over part p's rows alone with part p's graph -- which the oracle's device-order mode reproduces --, ids shifted by the part's first
row; the result is the stable merge of a query's items in probe order.

Base: 2,500 x 32 clustered rows (test_partitioned_hnsw_mirror's), cut into 7 parts of 413, 0, 1, 700, 333, 650 and 403 rows: one
empty, one of a single row, every origin inside a 32-bit word of the visited set.  One cosine case at dim 768 (three 256-float
chunks per row instead of one)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [413, 0, 1, 700, 333, 650, 403]
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
NPARTS, N, NQ, KP, M, EFC, SEED = len(SIZES), 2500, 300, 10, 8, 60, 42
EMPTY = 1
EFS = (0, 64, 640)          # 0: the default, max(k_part, 50)
BUILD_HEURISTIC = 2


def _data(O, n, dim, dist="gaussian", seed=42, **kw):
    return O.generate_dataset(n, dim, dist, seed=seed, **kw).astype(np.float32)


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


def _sub_graph(O, g, parts, p):
    """Part p of a forest's arrays as a graph over the part's rows alone (ids shifted back by the part's first row)."""
    lo, hi = int(parts.part_off[p]), int(parts.part_off[p + 1])
    b0, b1 = int(g.up_off[lo]), int(g.up_off[hi])
    l0 = g.l0_adj.reshape(g.n, -1)[lo:hi].copy()
    up = g.up_adj.reshape(-1, g.M)[b0:b1].copy()
    l0[l0 >= 0] -= lo
    up[up >= 0] -= lo
    return O.Graph(g.levels[lo:hi].copy(), l0, g.up_off[lo:hi + 1] - b0, up.reshape(-1), g.M, int(parts.part_entry[p]) - lo,
                   int(parts.part_max_level[p]))


def _same_graph(a, b, what):
    np.testing.assert_array_equal(a.levels, b.levels, err_msg=what + ": levels")
    np.testing.assert_array_equal(a.l0_adj.reshape(len(a.levels), -1), b.l0_adj.reshape(len(b.levels), -1), err_msg=what + ": layer 0")
    np.testing.assert_array_equal(a.up_off, b.up_off, err_msg=what + ": up_off")
    nb = int(a.up_off[-1]) * a.M
    np.testing.assert_array_equal(a.up_adj.reshape(-1)[:nb], b.up_adj.reshape(-1)[:nb], err_msg=what + ": upper layers")


class _World:
    """Per (metric, dim): the base, the forest handle built by hnsw_build_parts, its arrays, and -- computed once, shared by every
    test -- the oracle's lists of all 300 queries in every part at every ef."""

    def __init__(self, eng, O):
        self.eng, self.O, self.made = eng, O, {}

    def get(self, metric, dim=32, sizes=SIZES, base_edit=None, M=M, efc=EFC, nq=NQ, tag=""):
        key = (metric, dim, tag)
        if key in self.made:
            return self.made[key]
        O, w = self.O, type("W", (), {})()
        w.metric, w.m = metric, O.METRICS[metric]
        w.off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        w.base = _data(O, N, dim, "clustered", num_clusters=12, noise_level=0.4)
        if base_edit:
            base_edit(w.base, w.off)
        w.Q = np.vstack([_data(O, nq - 2, dim, seed=43), w.base[5:6], w.base[int(w.off[3]) + 7:int(w.off[3]) + 8]]).astype(np.float32)
        w.idx = self.eng.Index(w.base, metric)
        w.idx.hnsw_build_parts(w.off, M, efc, SEED)
        w.g, w.parts = w.idx.get_graph(), w.idx.graph_parts()
        w.subs = [_sub_graph(O, w.g, w.parts, p) if sizes[p] else None for p in range(len(sizes))]
        w.lists = {}
        self.made[key] = w
        return w

    def lists(self, w, ef, kp=KP):
        """[nparts][nq][kp] ids (handle rows), distances, [nparts][nq][2] counters: the oracle, part by part."""
        if (ef, kp) not in w.lists:
            nq, P = len(w.Q), len(w.subs)
            ids = np.full((P, nq, kp), -1, np.int32)
            d = np.full((P, nq, kp), np.inf, np.float32)
            st = np.zeros((P, nq, 2), np.int64)
            for p, sg in enumerate(w.subs):
                if sg is None:
                    continue
                lo, hi = int(w.off[p]), int(w.off[p + 1])
                oi, od, ost, _ = self.O.hnsw_search(w.base[lo:hi], sg, w.Q, kp, ef=(ef or None), metric=w.m, mode=self.O.MODE_DEV)
                ids[p] = np.where(oi >= 0, oi + lo, -1)
                d[p] = od.astype(np.float32)
                st[p] = ost
            w.lists[(ef, kp)] = (ids, d, st)
        return w.lists[(ef, kp)]

    def close(self):
        for w in self.made.values():
            w.idx.close()


@pytest.fixture(scope="module")
def world(native_lib, oracle):
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    w = _World(engine, oracle)
    yield w
    w.close()


def _probe_tables(nq, nparts=NPARTS):
    rs = np.random.RandomState(11)
    rnd = np.full((nq, 4), -1, np.int32)
    for q in range(nq):
        pick = rs.permutation(nparts)[:4]
        keep = rs.rand(4) < 0.75
        rnd[q, keep] = pick[keep]
    named = np.tile(np.array([[3, EMPTY, 0, 2, nparts + 5]], np.int32), (nq, 1))      # the empty part, the one-row part, an id out of range
    named[::3, 0] = 5
    return [("every part", None), ("random with skips", rnd), ("names the empty part", named)]


def _expected(lists, probes, nq):
    """Items in probe order: ([nq][nprobe * kp] ids, distances, [nq][nprobe][2] counters)."""
    ids, d, st = lists
    P, _, kp = ids.shape
    if probes is None:
        probes = np.tile(np.arange(P, dtype=np.int32), (nq, 1))
    nprobe = probes.shape[1]
    ei = np.full((nq, nprobe, kp), -1, np.int32)
    ed = np.full((nq, nprobe, kp), np.inf, np.float32)
    es = np.zeros((nq, nprobe, 2), np.int64)
    for r in range(nprobe):
        p = probes[:, r]
        ok = (p >= 0) & (p < P)
        q = np.flatnonzero(ok)
        ei[q, r], ed[q, r], es[q, r] = ids[p[q], q], d[p[q], q], st[p[q], q]
    return ei.reshape(nq, -1), ed.reshape(nq, -1), es


def _search_dev(w, Q, probes, kp, k, ef):
    import torch

    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    pd = torch.from_numpy(probes).to(dev) if probes is not None else None
    nprobe = probes.shape[1] if probes is not None else len(w.subs)
    st = torch.full((len(Q), nprobe, 2), -7, dtype=torch.int64, device=dev)
    ids, d = w.idx.hnsw_search_parts_dev(Qd, kp, k, ef, probes=pd, stats=st)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), d.cpu().numpy(), st.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_items(world, w, what, nqs=(1, 40, 300), efs=EFS):
    """Case 2: k == nprobe * k_part, the merge drops nothing -- every item's ids, distance bits and counters are the oracle's."""
    for ef in efs:
        lists = world.lists(w, ef)
        for nq in nqs:
            for pname, probes in _probe_tables(nq, len(w.subs)):
                nprobe = probes.shape[1] if probes is not None else len(w.subs)
                ei, ed, es = _expected(lists, probes, nq)
                wi, wd = _stable_topk(ei, ed, nprobe * KP)
                ids, d, st = _search_dev(w, w.Q[:nq], probes, KP, nprobe * KP, ef)
                tag = "%s, nq %d, ef %d, probes: %s" % (what, nq, ef, pname)
                np.testing.assert_array_equal(ids, wi, err_msg=tag + ": ids")
                np.testing.assert_array_equal(_bits(d), _bits(wd), err_msg=tag + ": distance bits")
                np.testing.assert_array_equal(st, es, err_msg=tag + ": counters")


TUNES = [("default", {}, None), ("wave never", {"HNSW_WAVE": 0}, None), ("wave always", {"HNSW_WAVE": 2}, None),
         ("one wave per item", {"HNSW_NW": 1}, None), ("two waves", {"HNSW_NW": 2}, None), ("four waves", {"HNSW_NW": 4}, None),
         ("HBM stamps", {"VIS_GLOBAL": 1}, None), ("HBM stamps, wave kernel", {"VIS_GLOBAL": 1, "HNSW_WAVE": 2}, None),
         ("rejection test off", {}, 0), ("rejection test on, wave kernel", {"HNSW_WAVE": 2}, 2)]


# ---- 1. the forest is the per-part build ------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, BUILD_HEURISTIC])
def test_forest_equals_the_per_part_builds(world, flags):
    eng, O = world.eng, world.O
    base = _data(O, N, 32, "clustered", num_clusters=12, noise_level=0.4)
    with eng.Index(base, "cosine") as idx:
        idx.hnsw_build_parts(OFF, M, EFC, SEED, flags=flags)
        assert idx.has_graph
        g, parts = idx.get_graph(), idx.graph_parts()
        assert parts.nparts == NPARTS and parts.part_off.tolist() == OFF.tolist()
        assert g.entry == -1 and g.max_level == parts.part_max_level.max()            # hnswgpu_graph_sizes on a forest
        assert parts.part_entry[EMPTY] == -1 and parts.part_entry[2] == OFF[2] and parts.part_max_level[EMPTY] == 0
        for p in range(NPARTS):
            lo, hi = int(OFF[p]), int(OFF[p + 1])
            if lo == hi:
                continue
            with eng.Index(base[lo:hi], "cosine") as alone:
                alone.hnsw_build(M, EFC, SEED, heuristic=bool(flags))
                ga = alone.get_graph()
            sub = _sub_graph(O, g, parts, p)
            _same_graph(sub, ga, "flags %d, part %d" % (flags, p))
            assert (sub.entry, sub.max_level) == (ga.entry, ga.max_level), "flags %d, part %d: entry / top level" % (flags, p)
        # set_graph_parts(get_graph + graph_parts) round-trips, on a fresh handle and over a plain graph
        Q = _data(O, 40, 32, seed=43)
        want = idx.hnsw_search_parts(Q, KP, 3 * KP, 64, want_stats=True)
        with eng.Index(base, "cosine") as other:
            other.hnsw_build(M, 30, SEED)                                                  # a plain graph first: it is replaced
            other.set_graph_parts(g, parts)
            g2, p2 = other.get_graph(), other.graph_parts()
            _same_graph(g2, g, "round trip")
            assert g2.entry == -1 and g2.max_level == g.max_level
            for a, b in ((p2.part_off, parts.part_off), (p2.part_entry, parts.part_entry), (p2.part_max_level, parts.part_max_level)):
                np.testing.assert_array_equal(a, b)
            got = other.hnsw_search_parts(Q, KP, 3 * KP, 64, want_stats=True)
            for a, b in zip(got, want):
                np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
            other.hnsw_build(M, 30, SEED)                                                  # ... and the other way round
            with pytest.raises(eng._native.HnswGpuError) as e:
                other.graph_parts()
            assert e.value.code == -3
            assert other.hnsw_search(Q[:2], 3)[0].shape == (2, 3)


# ---- 2. every item against the oracle, under every kernel the plan may choose -------------------------------------------------
@pytest.mark.parametrize("tname,keys,rejection", TUNES, ids=[t[0] for t in TUNES])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_items_equal_the_oracle(world, tune, metric, tname, keys, rejection):
    eng = world.eng
    w = world.get(metric)
    for name, v in keys.items():
        tune.set(name, v)
    if rejection is not None:
        w.idx.set_rejection_test(rejection)
    before = {c: eng.debug_counter(c) for c in ("hnsw_wave", "hnsw_solo", "hnsw_helpers", "hnsw_rejection", "hnsw_plain")}
    try:
        _check_items(world, w, "%s, %s" % (metric, tname))
    finally:
        if rejection is not None:
            w.idx.set_rejection_test(2)
    after = {c: eng.debug_counter(c) for c in before}
    ncalls = 27
    assert after["hnsw_solo"] == before["hnsw_solo"] and after["hnsw_helpers"] == before["hnsw_helpers"], "a forest launch on a small-launch kernel"
    if keys.get("HNSW_WAVE") == 2:
        assert after["hnsw_wave"] - before["hnsw_wave"] == ncalls, "the wave-kernel cases did not all run on it"
    if keys.get("HNSW_WAVE") == 0 or "HNSW_NW" in keys:
        assert after["hnsw_wave"] == before["hnsw_wave"]
    if rejection == 0:
        assert after["hnsw_rejection"] == before["hnsw_rejection"]
    if rejection == 2:
        assert after["hnsw_rejection"] - before["hnsw_rejection"] >= ncalls


@pytest.mark.parametrize("tname,keys", [("default", {}), ("wave always", {"HNSW_WAVE": 2})])
def test_items_equal_the_oracle_dim_768(world, tune, tname, keys):
    """Three 256-float chunks per row (another instantiation of both kernels)."""
    w = world.get("cosine", dim=768, nq=40)
    for name, v in keys.items():
        tune.set(name, v)
    _check_items(world, w, "cosine 768, %s" % tname, nqs=(40,), efs=(0, 640))


# ---- 3. the merge ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_merged_results(world, metric):
    w = world.get(metric)
    for ef in (0, 64):
        lists = world.lists(w, ef)
        for nq, k in ((1, 1), (40, 7), (300, 25), (40, 39)):
            for pname, probes in _probe_tables(nq):
                ei, ed, es = _expected(lists, probes, nq)
                wi, wd = _stable_topk(ei, ed, k)
                ids, d, st = _search_dev(w, w.Q[:nq], probes, KP, k, ef)
                tag = "%s nq %d k %d ef %d, probes: %s" % (metric, nq, k, ef, pname)
                np.testing.assert_array_equal(ids, wi, err_msg=tag)
                np.testing.assert_array_equal(_bits(d), _bits(wd), err_msg=tag)
                np.testing.assert_array_equal(st, es, err_msg=tag)
                hi, hd, hs = w.idx.hnsw_search_parts(w.Q[:nq], KP, k, ef, probes=probes, want_stats=True)   # the host entry
                np.testing.assert_array_equal(hi, wi, err_msg=tag + " (host)")
                np.testing.assert_array_equal(_bits(hd), _bits(wd), err_msg=tag + " (host)")
                np.testing.assert_array_equal(hs, es, err_msg=tag + " (host)")


# ---- 4. the repeat pass, per item --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_ghost_overflow_is_repeated_per_item(world, metric):
    """Part 3 holds 300 bit-identical rows (+ 20 others): more tied candidates than the 32 ghost slots, the ghost-overflow case of
    test_hnsw_many_ties.  The items on that part are repeated with the largest list and equal the oracle, counters included; the
    items of the same queries on the other parts are what they are without it."""
    sizes = [413, 0, 1, 320, 713, 650, 403]

    def edit(base, off):
        lo = int(off[3])
        base[lo:lo + 300] = base[lo]

    w = world.get(metric, sizes=sizes, base_edit=edit, M=5, efc=40, nq=12, tag="ties")
    lo = int(w.off[3])
    w.Q[0], w.Q[1] = w.base[lo], w.base[lo + 3]
    w.lists.clear()
    for ef, kp in ((50, 10), (7, 3), (300, 70)):
        lists = world.lists(w, ef, kp)
        for pname, probes in [("every part", None), ("tied part between others", np.tile(np.array([[5, 3, 0]], np.int32), (12, 1)))]:
            nprobe = probes.shape[1] if probes is not None else len(sizes)
            ei, ed, es = _expected(lists, probes, 12)
            wi, wd = _stable_topk(ei, ed, nprobe * kp)
            ids, d, st = _search_dev(w, w.Q, probes, kp, nprobe * kp, ef)
            tag = "ties %s ef %d, probes: %s" % (metric, ef, pname)
            np.testing.assert_array_equal(ids, wi, err_msg=tag)
            np.testing.assert_array_equal(_bits(d), _bits(wd), err_msg=tag)
            np.testing.assert_array_equal(st, es, err_msg=tag)


# ---- 5. the mirrors ------------------------------------------------------------------------------------------------------------
def _same_dev(a, b, what):
    import torch

    assert torch.equal(a[0].cpu(), b[0].cpu()), what + ": ids"
    assert a[0].dtype == b[0].dtype
    assert torch.equal(a[1].cpu().view(torch.int32), b[1].cpu().view(torch.int32)), what + ": distance bits"


def test_partitioned_mirror_one_handle(world):
    import torch

    from hnsw_clj_amd import datagen, partitioned_hnsw as ph

    O = world.O
    vecs = _data(O, 2500, 32, "clustered", num_clusters=12, noise_level=0.4)
    Q = torch.from_numpy(_data(O, 30, 32, seed=43)).cuda()
    a = ph.build_index(datagen.indexed(vecs), num_partitions=8, ef_construction=60)
    b = ph.build_index(datagen.indexed(vecs), num_partitions=8, ef_construction=60, one_handle=True)
    try:
        assert b.handle is not None and not b.partitions and len(a.partitions) == 8
        for mode, k in (("lightning", 10), ("ultra", 10), ("turbo", 3), ("bogus", 4)):
            _same_dev(ph.search_batch_dev(b, Q, k, mode), ph.search_batch_dev(a, Q, k, mode), "partitioned, " + mode)
            assert ph.search_batch(b, Q.cpu().numpy(), k, mode) == ph.search_batch(a, Q.cpu().numpy(), k, mode)
        assert ph.search_partitioned_lightning(b, vecs[17], 5)[0]["id"] == "vec_17"
    finally:
        a.close()
        b.close()


def test_ivf_hnsw_mirror_one_handle(world):
    import torch

    from hnsw_clj_amd import datagen, ivf_hnsw

    O = world.O
    vecs = _data(O, 3000, 32, "clustered", num_clusters=6, noise_level=0.5)
    a = ivf_hnsw.build_index(datagen.indexed(vecs), num_partitions=6, ef_construction=60, max_iterations=4)
    b = ivf_hnsw.build_index(datagen.indexed(vecs), num_partitions=6, ef_construction=60, max_iterations=4, one_handle=True)
    try:
        assert b.handle is not None and all(p is None for p in b.partitions)
        for nq, mode, honour in ((40, "fast", False), (3, "balanced", False), (40, "accurate", True)):
            Q = torch.from_numpy(_data(O, nq, 32, seed=43)).cuda()
            _same_dev(ivf_hnsw.search_batch_dev(b, Q, 5, mode, honour_modes=honour),
                      ivf_hnsw.search_batch_dev(a, Q, 5, mode, honour_modes=honour), "ivf-hnsw, " + mode)
            assert ivf_hnsw.search_batch(b, Q.cpu().numpy(), 5, mode, honour_modes=honour) == \
                ivf_hnsw.search_batch(a, Q.cpu().numpy(), 5, mode, honour_modes=honour)
        assert ivf_hnsw.search_knn(b, vecs[11], 3)[0]["id"] == "vec_11"
    finally:
        a.close()
        b.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------
def _code(eng, fn):
    with pytest.raises(eng._native.HnswGpuError) as e:
        fn()
    return e.value.code


def test_bad_forests_leave_the_handle_unchanged(world, tmp_path):
    eng = world.eng
    w = world.get("cosine")
    Q = w.Q[:40]
    want = w.idx.hnsw_search_parts(Q, KP, 20, 64, want_stats=True)

    def unchanged(what):
        got = w.idx.hnsw_search_parts(Q, KP, 20, 64, want_stats=True)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b, err_msg=what)
        assert w.idx.graph_parts().part_entry.tolist() == w.parts.part_entry.tolist()

    def graph():
        return eng.Graph(w.g.levels.copy(), w.g.l0_adj.copy(), w.g.up_off.copy(), w.g.up_adj.copy(), w.g.M, -1, 0)

    # an edge that crosses parts (layer 0, then an upper layer)
    g = graph()
    g.l0_adj.reshape(N, -1)[3, 0] = int(OFF[3]) + 1
    assert _code(eng, lambda: w.idx.set_graph_parts(g, w.parts)) == -1
    unchanged("edge crossing parts")
    node = int(np.flatnonzero(w.g.levels[:SIZES[0]] > 0)[0])
    g = graph()
    g.up_adj.reshape(-1, g.M)[int(g.up_off[node]), 0] = int(w.parts.part_entry[3])
    assert _code(eng, lambda: w.idx.set_graph_parts(g, w.parts)) == -1
    unchanged("upper edge crossing parts")
    # an entry outside its part; an empty part with an entry; an entry below its stated level
    for p, ent, lv in ((0, int(OFF[3]), None), (EMPTY, 0, None), (3, None, 31)):
        e, l = w.parts.part_entry.copy(), w.parts.part_max_level.copy()
        if ent is not None:
            e[p] = ent
        if lv is not None:
            l[p] = lv
        assert _code(eng, lambda: w.idx.set_graph_parts(graph(), eng.GraphParts(w.parts.part_off, e, l))) == -1
        unchanged("bad entry of part %d" % p)
    # a node above its part's stated top level
    l = w.parts.part_max_level.copy()
    l[3] = 0
    top = int(w.g.levels[OFF[3]:OFF[4]].max())
    if top > 0:
        e = w.parts.part_entry.copy()
        assert _code(eng, lambda: w.idx.set_graph_parts(graph(), eng.GraphParts(w.parts.part_off, e, l))) == -1
        unchanged("node above part_max_level")
    # part_off: not monotone, not ending at n, not starting at 0
    for k, v in ((2, int(OFF[3]) + 5), (NPARTS, N - 1), (0, 1)):
        off = w.parts.part_off.copy()
        off[k] = v
        assert _code(eng, lambda: w.idx.set_graph_parts(graph(), eng.GraphParts(off, w.parts.part_entry, w.parts.part_max_level))) == -1
        unchanged("part_off[%d] = %d" % (k, v))
        assert _code(eng, lambda: w.idx.hnsw_build_parts(off, M, EFC, SEED)) == -1
        unchanged("hnsw_build_parts with part_off[%d] = %d" % (k, v))
    assert _code(eng, lambda: w.idx.hnsw_build_parts(OFF, M, 5000, SEED)) == -5
    assert _code(eng, lambda: w.idx.hnsw_build_parts(OFF, 40, EFC, SEED)) == -5
    unchanged("hnsw_build_parts limits")
    # what a forest does not serve: HNSWGPU_ESTATE, with a message that names the parts entry points
    allow = eng.pack_mask(np.ones(N, np.bool_), N)
    for what, fn in (("hnsw_search", lambda: w.idx.hnsw_search(Q, 5, 64)),
                     ("hnsw_search_filtered", lambda: w.idx.hnsw_search_filtered(Q, 5, allow, 64)),
                     ("hnsw_add", lambda: w.idx.hnsw_add(w.base[:2])),
                     ("save", lambda: w.idx.save(tmp_path / "forest.idx"))):
        with pytest.raises(eng._native.HnswGpuError, match="parts|forest") as e:
            fn()
        assert e.value.code == -3, what
    import torch

    Qd = torch.from_numpy(Q).cuda()
    assert _code(eng, lambda: w.idx.hnsw_search_dev(Qd, 5, 64)) == -3
    assert _code(eng, lambda: w.idx.hnsw_search_filtered_dev(Qd, 5, torch.from_numpy(allow.view(np.int32)).cuda(), 64)) == -3
    torch.cuda.synchronize()
    assert w.idx.n == N and not (tmp_path / "forest.idx").exists()
    unchanged("refused calls")


def test_argument_limits_as_hnsw_search(world):
    eng = world.eng
    w = world.get("cosine")
    Q = w.Q[:4]
    assert _code(eng, lambda: w.idx.hnsw_search_parts(Q, 0, 5)) == -1                  # k_part >= 1
    assert _code(eng, lambda: w.idx.hnsw_search_parts(Q, 5, 0)) == -1                  # k >= 1
    assert _code(eng, lambda: w.idx.hnsw_search_parts(Q, 5, 5, ef=4097)) == -5         # ef <= 4096
    assert _code(eng, lambda: w.idx.hnsw_search_parts(Q, 4097, 5)) == -5               # ef is raised to k_part first
    assert _code(eng, lambda: w.idx.hnsw_search_parts(Q, 5, 1025)) == -5               # the merge's limit
    assert _code(eng, lambda: w.idx.hnsw_search_parts(Q, 5, 5, probes=np.zeros((4, 0), np.int32))) == -1
    L, h = eng.lib(), w.idx._h
    ids, d = np.zeros((4, 5), np.int32), np.zeros((4, 5), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.hnswgpu_hnsw_search_parts(h, None, 4, 5, 0, None, 0, 5, p(ids), p(d), None) == -1
    assert L.hnswgpu_hnsw_search_parts(h, p(Q), 4, 5, 0, None, 0, 5, None, p(d), None) == -1
    assert L.hnswgpu_hnsw_search_parts(h, p(Q), 4, 5, 0, None, 0, 5, p(ids), None, None) == -1
    assert L.hnswgpu_hnsw_search_parts(h, p(Q), -1, 5, 0, None, 0, 5, p(ids), p(d), None) == -1
    assert L.hnswgpu_hnsw_search_parts(h, None, 0, 5, 0, None, 0, 5, None, None, None) == 0     # nq == 0: nothing to do
    n = C.c_int32(0)
    assert L.hnswgpu_graph_parts(h, C.byref(n), None, None, None) == 0 and n.value == NPARTS      # arrays may be NULL
    # ef below k_part is raised to it, ef <= 0 is max(k_part, 50): both as hnswgpu_hnsw_search
    a = w.idx.hnsw_search_parts(Q, 60, 60, ef=3)
    b = w.idx.hnsw_search_parts(Q, 60, 60, ef=60)
    c = w.idx.hnsw_search_parts(Q, 60, 60, ef=0)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[0], c[0])
    # a plain graph has no parts to search
    with eng.Index(w.base[:200], "cosine") as plain:
        plain.hnsw_build(M, 30, SEED)
        assert _code(eng, lambda: plain.hnsw_search_parts(Q, 5, 5, probes=np.zeros((4, 1), np.int32))) == -3
        assert _code(eng, lambda: plain.graph_parts()) == -3
    with eng.Index(w.base[:200], "cosine") as bare:
        assert _code(eng, lambda: bare.hnsw_search_parts(Q, 5, 5, probes=np.zeros((4, 1), np.int32))) == -3


def test_empty_forest(world):
    """No rows at all: every item is padding."""
    eng = world.eng
    with eng.Index(np.zeros((0, 32), np.float32), "cosine") as idx:
        idx.hnsw_build_parts(np.zeros(4, np.int64), M, EFC, SEED)
        assert idx.graph_parts().part_entry.tolist() == [-1, -1, -1]
        ids, d, st = idx.hnsw_search_parts(_data(world.O, 3, 32, seed=43), 4, 6, want_stats=True)
        assert (ids == -1).all() and np.isinf(d).all() and (st == 0).all() and st.shape == (3, 3, 2)


def test_calls_on_two_streams_around_another_handle_are_ordered(world):
    """The pattern of test_call_ordering.py: two hnsw_search_parts_dev calls of ONE forest handle on two streams, a plain-graph
    handle's search between them, no synchronise -- hg::Call orders the forest's shared scratch (item table, per-item lists) across
    the streams, so every call returns the bits it returns alone."""
    import torch

    eng = world.eng
    w = world.get("cosine")
    dev = torch.device("cuda", 0)
    Qa, Qb = (torch.from_numpy(np.ascontiguousarray(w.Q[s])).to(dev) for s in (slice(0, 64), slice(64, 300)))
    pb = torch.from_numpy(_probe_tables(236)[1][1]).to(dev)

    def out(nq, k):
        return torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev)

    with eng.Index(w.base[:800], "cosine") as plain:
        plain.hnsw_build(M, 40, SEED)
        calls = [lambda o: w.idx.hnsw_search_parts_dev(Qa, KP, 25, 64, out=o),
                 lambda o: plain.hnsw_search_dev(Qa, 25, 64, out=o),
                 lambda o: w.idx.hnsw_search_parts_dev(Qb, KP, 25, 640, probes=pb, out=o)]
        shapes = [(64, 25), (64, 25), (236, 25)]
        want = []
        for c, s in zip(calls, shapes):
            o = out(*s)
            c(o)
            torch.cuda.synchronize()
            want.append(o)
        streams = [torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.default_stream()]
        got = [[out(*s) for s in shapes] for _ in range(10)]
        torch.cuda.synchronize()
        for r in range(10):
            for j, c in enumerate(calls):
                with torch.cuda.stream(streams[(j + r) % 3]):
                    c(got[r][j])
        torch.cuda.synchronize()
        for r in range(10):
            for j in range(3):
                _same_dev(got[r][j], want[j], "repetition %d, call %d" % (r, j))
