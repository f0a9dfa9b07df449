"""Every HNSW traversal kernel at every loader width of pick_nch (engine.hip): hnsw_wave_kernel plain, ordered and reading the dense
bounds table, hnsw_search_kernel with 1 / 2 / 4 waves, the round-2 helper kernel, hnsw_solo_kernel and the repeat pass, each with the
int8 rejection test and without it where the launch keeps it.  Every width is another instantiation (HG_HNSW_ROWS, engine.hpp:
rows in flight 8/4, 8/4, 8/2, 4/4, 4/4, 2/2, 2/2 for the widths 1, 2, 3, 4, 6, 8, 12) with its own gather-trip length, code_dot16 and
rows_sum_to_lane; the other search tests run widths 1, 2, 3, 6 and 12 and the wave kernel at 1, 2 and 3 only.

Dims: one per width and the edges of a width -- rows padded to a float4 (ld != dim: 5, 257, 1030, 1538, 2050) and rows whose LAST
loader chunk is padding from end to end (1030: 5 chunks of 256 floats in a loader of 6; 1538: 7 in 8; 2050: 9 in 12).

Per dim: 1,200 rows of the oracle's clustered generator (10 clusters, noise 0.4), 100 of them overwritten with copies of row 17; 48
queries: 46 held-out draws, row 17 itself, a copy of the buffer's last row (asserted: the reference evaluates row 1,199).  Two
handles per dim, l2 and one of cosine / dot, rejection mode 2, built on the device (M 8, ef_construction 60; the heuristic builder at
every second dim) ONCE and shared by all families.  References per (handle, ef in {32, 200}), k 10, computed once: the oracle's
device-order search on the handle's own graph -- ids, distance BITS and both per-query counters of every launch equal it -- and its
f64 search, against which the first 16 queries are held to the suite's top-k parity.  Every launch asserts by the launch counters
(or the dense table's state entry) that the intended kernel ran.

THE REPEAT PASS.  A query whose list could not keep every candidate that ties its worst lists itself, and hnsw_search_kernel with
four waves and the largest list the LDS holds answers it again.  When that happens follows from the lists (K_GHOST = kGhost = cap - ef):
  * hnsw_search_kernel keeps the entries behind its ef nearest that tie the worst (ghosts) in cap - ef slots and flags the query when
    an UNEXPANDED tie falls behind them (kernels.hpp: sc[6]);
  * HnswList::compact (hnsw_list.hpp) keeps the run of ties behind `nearest` as far as min(64, cap - ef) entries go and flags the
    query when that room is all ties and entries were cut off; the level's last compact sees the level's last state.
Ties of one distance w are admitted only while the worst is above w, and leave only once it is w, so all of them were in `nearest`
together: at most ef - 1 can ever be out and tied.  Hence NO query overflows at ef 32, whatever the rows; and the query that IS the
duplicated row never does, at any number of copies: nothing is nearer to it than a copy, so no copy ever leaves its list.  (Measured
on the CPU model of these graphs: that query has none out, no query of the 48 more than 19 tied entries out.)  These launches are
therefore asserted to be the outcome WITHOUT a repeat pass: trace() (scripted_graphs.py) of every query on layer 0 of the handle's
own graph, from the entry point the upper layers hand down, with device-order distances, never shows K_GHOST tied entries out.
(At ef 32 every handle has queries whose full list loses older entries -- asserted; at ef 200 the closest-m graphs of 1,200 clustered
rows are too loosely connected for every list to fill: the long full list is the scripted launch's, below.)
The repeat pass itself runs on a graph that reaches it by construction: S-tie-many of scripted_graphs.py (ef 128: 64 entries leave
`nearest` and every one ties its worst), embedded so that a row fills EVERY loader chunk of its dim (embed_wide; the scripted
module's own embedding leaves all but two components zero, which a loader cut short would not notice).  Asserted on the CPU: the
scripted query ends with more than K_GHOST tied entries out (the wave list's last compact) and the reference expands one of them
after that number was passed (an unexpanded tie was cut: the single-workgroup kernel's flag); a row of the graph among the same
launch's queries never has K_GHOST out.  Both outcomes in one launch, at every dim, through families A - D.

Not searched: queries or rows holding NaN or infinity (test_hnsw_dense_bounds.py: test_search_of_special_queries_and_rows says why),
builds, forest launches, filtered search."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scripted_graphs as sg  # noqa: E402
from util import assert_exact, assert_topk_parity, metric_scale  # noqa: E402

# loader width (float4 chunks of 64 lanes per row) -> the dims that take it
WIDTHS = {
    1: [5, 128],           # padded to 8; the widest row of one chunk
    2: [257],              # padded to 260
    3: [768],
    4: [1000],
    6: [1030, 1536],       # 1030: padded to 1032, 5 chunks needed -- the sixth is padding from end to end
    8: [1538, 2048],       # 1538: padded to 1540, 7 of 8
    12: [2050, 3072],      # 2050: padded to 2052, 9 of 12; the limit
}
DIMS = [d for w in sorted(WIDTHS) for d in WIDTHS[w]]
ALT_METRIC_OF = {dim: ("cosine", "dot")[(j // 2) % 2] for j, dim in enumerate(DIMS)}
BUILDER_OF = {dim: ("closest", "heuristic")[j % 2] for j, dim in enumerate(DIMS)}
HANDLES = [(dim, which) for dim in DIMS for which in ("l2", "alt")]

N, NQ, NCOPY, SRC = 1200, 48, 100, 17
CLUSTERS, NOISE = 10, 0.4
M, EFC, SEED, K = 8, 60, 42, 10
EFS = (32, 200)
K_GHOST = 32                 # kernels.hpp: kGhost; every first-pass list has cap = ef + kGhost (hnsw.hip)
BATCHES = ((0, 1), (1, 4), (0, NQ))
SENT_ID, SENT_D, SENT_ST = -7, -1.0, -3
_DATA = {}


def _chunks(dim):
    """float4 chunks of 64 lanes a row of this dim needs: ld = dim rounded up to 4 floats, one float4 per lane and chunk."""
    return -(-((dim + 3) // 4) // 64)


def _pick_nch(dim):
    """pick_nch (engine.hip) of a handle of this dim."""
    return next((o for o in (1, 2, 3, 4, 6, 8, 12) if o >= _chunks(dim)), 0)


def test_the_width_table_keeps_its_shape():
    assert sorted(WIDTHS) == [1, 2, 3, 4, 6, 8, 12] and all(WIDTHS.values()), "a loader width went missing"
    for w, dims in WIDTHS.items():
        assert all(_pick_nch(d) == w for d in dims), "width %d: %s take %s" % (w, dims, [_pick_nch(d) for d in dims])
    for w in (6, 8, 12):
        assert any(_chunks(d) < w for d in WIDTHS[w]), "width %d: no dim whose last chunk is padding from end to end" % w
    assert any(d % 4 and _pick_nch(d) > 1 for d in DIMS), "no padded dim beyond one chunk"
    assert _pick_nch(3072) == 12 and _pick_nch(3073) == 0                      # (the limit is the limit)
    for metric in ("cosine", "dot"):
        assert len({_pick_nch(d) for d in DIMS if ALT_METRIC_OF[d] == metric}) >= 3, metric
        assert {BUILDER_OF[d] for d in DIMS if ALT_METRIC_OF[d] == metric} == {"closest", "heuristic"}, metric
    for builder in ("closest", "heuristic"):
        assert len({_pick_nch(d) for d in DIMS if BUILDER_OF[d] == builder}) >= 5, builder
    assert len(set(HANDLES)) == len(HANDLES) == 2 * len(DIMS)


# ---- the rows and the references ---------------------------------------------------------------------------------------------------
def _data(O, dim):
    """(rows f32 [N, dim], queries f32 [NQ, dim]), made once per dim, read-only."""
    if dim not in _DATA:
        rows = O.generate_dataset(N + NQ - 2, dim, "clustered", num_clusters=CLUSTERS, noise_level=NOISE, seed=7).astype(np.float32)
        base = np.ascontiguousarray(rows[:N])
        at = np.random.RandomState(dim).choice(np.setdiff1d(np.arange(N - 1), [SRC]), NCOPY, replace=False)
        base[at] = base[SRC]
        Q = np.ascontiguousarray(np.concatenate([rows[N:], base[SRC:SRC + 1], base[N - 1:N]]))
        assert Q.shape == (NQ, dim)
        base.flags.writeable = Q.flags.writeable = False
        _DATA[dim] = (base, Q)
    return _DATA[dim]


def dev_distance_rows(O, rows, Q, metric):
    """[nq, n] device-order distances of every query to every row, as the oracle's traversal computes them (its exact scan in
    the device mode, unsorted again)."""
    ids, d, _ = O.exact_knn(rows, Q, len(rows), metric=O.METRICS[metric], mode=O.MODE_DEV)
    out = np.empty_like(d)
    np.put_along_axis(out, ids.astype(np.int64), d, axis=1)
    return out


def layer_lists(g, level):
    """[n, slots] adjacency of one layer of a Graph (-1: no edge, or a node that does not reach the layer)."""
    if level == 0:
        return g.l0_adj.reshape(g.n, -1)
    adj = np.full((g.n, g.M), -1, np.int32)
    up = g.up_adj.reshape(-1, g.M)
    for u in np.flatnonzero(g.levels >= level):
        adj[u] = up[g.up_off[u] + level - 1]
    return adj


def search_trace(g, layers, dist, ef):
    """The reference's whole search of one query restated by scripted_graphs.trace: ef 1 on every upper layer (ultra_fast.clj:
    358-366), then layer 0 from the node they hand down.  layers[l]: layer_lists(g, l).  Returns (the layer-0 Trace, evaluations,
    expansions of all layers)."""
    entry, evals, hops = g.entry, 0, 0
    for level in range(g.max_level, 0, -1):
        tr = sg.trace(dist, layers[level], entry, 1)
        entry, evals, hops = int(tr.ids[0]), evals + tr.evals, hops + tr.hops
    tr = sg.trace(dist, layers[0], entry, ef)
    return tr, evals + tr.evals, hops + tr.hops


def overflows(tr, dist):
    """The trace proves that every first-pass list runs out of room for the candidates that tie its worst (module docstring)."""
    first = next((i for i, e in enumerate(tr.events) if e.n_tied_out > K_GHOST), None)
    if first is None or tr.events[-1].n_tied_out <= K_GHOST:
        return False
    w = tr.events[first].worst
    return tr.events[-1].worst == w and any(e.on_tie and dist[e.node] == w for e in tr.events[first + 1:])


def cannot_overflow(tr):
    """... that no list ever holds K_GHOST ties behind its ef nearest: none can be cut off."""
    return all(e.n_tied_out < K_GHOST for e in tr.events)


def check_traces(O, g, rows, Q, metric, refs, what):
    """{ef: [layer-0 Trace of every query]}, each compared with the oracle's device-order search as it is made."""
    dist = dev_distance_rows(O, rows, Q, metric)
    layers = [layer_lists(g, level) for level in range(g.max_level + 1)]
    out = {}
    for ef, (oi, od, ost) in refs.items():
        out[ef] = []
        for q in range(len(Q)):
            tr, evals, hops = search_trace(g, layers, dist[q], ef)
            assert (evals, hops) == tuple(int(x) for x in ost[q]), "%s ef %d query %d: the trace is not the oracle's search" % (what, ef, q)
            np.testing.assert_array_equal(tr.ids[:oi.shape[1]], oi[q], err_msg="%s ef %d query %d: trace ids" % (what, ef, q))
            out[ef].append(tr)
    return dist, out


class _Handle:
    """One built index with everything the families share."""

    def __init__(self, eng, O, dim, which):
        self.dim, self.metric = dim, "l2" if which == "l2" else ALT_METRIC_OF[dim]
        self.base, self.Q = _data(O, dim)
        self.what = "dim %d %s (%s builder)" % (dim, self.metric, BUILDER_OF[dim])
        if eng is None:      # (the CPU side alone: references() on a graph of the caller's)
            return
        self.idx = eng.Index(self.base, self.metric)
        self.idx.set_rejection_test(2)
        self.idx.hnsw_build(M, EFC, SEED, heuristic=BUILDER_OF[dim] == "heuristic")
        self.idx.set_profiling(True)         # the traversals count (f32 rows, neighbours)
        self.references(O, self.idx.get_graph())

    def references(self, O, g):
        """Everything that follows from the rows and the graph alone (no GPU)."""
        self.g = g
        code = O.METRICS[self.metric]
        self.ref = {ef: O.hnsw_search(self.base, self.g, self.Q, K, ef=ef, metric=code, mode=O.MODE_DEV)[:3] for ef in EFS}
        self.f64 = {ef: O.hnsw_search(self.base, self.g, self.Q[:16], K, ef=ef, metric=code)[:2] for ef in EFS}
        self.scale = metric_scale(self.metric, self.Q, self.base)
        # the launches of this handle are the outcome without a repeat pass, and the buffer's last row is read
        dist, traces = check_traces(O, self.g, self.base, self.Q, self.metric, self.ref, self.what)
        for ef in EFS:
            most = max(e.n_tied_out for tr in traces[ef] for e in tr.events)
            assert all(cannot_overflow(tr) for tr in traces[ef]), "%s ef %d: %d tied entries out of a list" % (self.what, ef, most)
        assert all(N - 1 in traces[ef][NQ - 1].visited for ef in EFS), self.what + ": the search does not reach the last row"
        assert all(len(tr.events) > 1 for ef in EFS for tr in traces[ef])
        assert sum(any(e.list_full and e.n_evicted_old for e in tr.events) for tr in traces[EFS[0]]) >= NQ // 2, \
            self.what + ": too few queries whose full list loses an older entry"

    def check(self, got, ef, lo, hi, tag):
        ids, d, st = got
        oi, od, ost = self.ref[ef]
        tag = "%s ef %d queries %d..%d, %s" % (self.what, ef, lo, hi, tag)
        np.testing.assert_array_equal(st, ost[lo:hi], err_msg=tag + ": counters")
        assert_exact(ids, d, oi[lo:hi], od[lo:hi], tag)
        top = min(hi, 16)
        if lo < top:
            fi, fd = self.f64[ef]
            assert_topk_parity(ids[:top - lo], d[:top - lo], fi[lo:top], fd[lo:top], tag + ", f64 reference", self.scale)


@pytest.fixture(scope="module")
def eng(native_lib):
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    return engine


@pytest.fixture(scope="module")
def handles(eng, oracle):
    made = {}

    def get(dim, which):
        if (dim, which) not in made:
            made[(dim, which)] = _Handle(eng, oracle, dim, which)
        h = made[(dim, which)]
        h.idx.set_rejection_test(2)
        h.idx.set_hnsw_dense_bounds(1)
        return h

    yield get
    for h in made.values():
        h.idx.close()


def _ids(cases):
    return ["dim%d-%s" % c for c in cases]


class _Launches:
    """Launch counters around one search: which of them rose."""
    NAMES = ("hnsw_wave", "hnsw_ordered", "hnsw_rejection", "hnsw_plain", "hnsw_helpers", "hnsw_solo")

    def __init__(self, eng, idx):
        self.eng, self.idx = eng, idx
        self.before = {c: eng.debug_counter(c) for c in self.NAMES}
        self.table = idx.hnsw_dense_bounds_state()[2]
        idx.rejection_stats(reset=True)

    def done(self):
        self.rose = {c for c in self.NAMES if self.eng.debug_counter(c) > self.before[c]}
        self.table = self.idx.hnsw_dense_bounds_state()[2] - self.table
        self.rows = self.idx.rejection_stats(reset=True)
        return self


def _dev_search(idx, Q, k, ef):
    """hnswgpu_hnsw_search_dev into sentinel-filled buffers: ids, distances, stats as numpy; no sentinel may be left."""
    import torch

    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(np.array(Q, np.float32)).to(dev)
    ids = torch.full((len(Q), k), SENT_ID, dtype=torch.int32, device=dev)
    d = torch.full((len(Q), k), SENT_D, dtype=torch.float32, device=dev)
    st = torch.full((len(Q), 2), SENT_ST, dtype=torch.int64, device=dev)
    idx.hnsw_search_dev(Qd, k, ef, out=(ids, d), stats=st)
    torch.cuda.synchronize()
    ids, d, st = ids.cpu().numpy(), d.cpu().numpy(), st.cpu().numpy()
    assert (ids != SENT_ID).all() and (d != SENT_D).all() and (st != SENT_ST).all(), "a query was not answered"
    return ids, d, st


def _assert_rows(rows, decides, tag):
    """(f32 rows, neighbours) of a launch; decides: the int8 loop must have decided something at this width, and not everything."""
    assert 0 < rows[0] <= rows[1] and (not decides or rows[0] < rows[1]), "%s: (f32 rows, neighbours) %s" % (tag, (rows,))


def _wave_launch(eng, idx, tune, Q, k, ef, mode, vis_global, ordered, dense, dev, decides=True):
    """One launch of the wave kernel as configured; asserts that it was that launch; returns (results, (f32 rows, neighbours),
    what it was)."""
    tune.set("HNSW_WAVE", 2)
    tune.set("PREFETCH", 0)          # no small-launch kernels: every batch size takes the wave kernel
    tune.unset("HNSW_NW")
    tune.set("VIS_GLOBAL", vis_global)
    tune.set("HNSW_ORDER", 2 if ordered else 0)
    idx.set_rejection_test(mode)
    idx.set_hnsw_dense_bounds(2 if dense else 0)
    L = _Launches(eng, idx)
    got = _dev_search(idx, Q, k, ef) if dev else idx.hnsw_search(Q, k, ef, want_stats=True)
    L.done()
    tag = "rejection %d, stamps %d, ordered %d, table %d, device buffers %d" % (mode, vis_global, ordered, dense, dev)
    assert "hnsw_wave" in L.rose and not L.rose & {"hnsw_helpers", "hnsw_solo"}, "%s: launch counters that rose: %s" % (tag, sorted(L.rose))
    assert ("hnsw_rejection" if mode == 2 else "hnsw_plain") in L.rose, "%s: %s" % (tag, sorted(L.rose))
    assert ("hnsw_ordered" in L.rose) == bool(ordered), "%s: %s" % (tag, sorted(L.rose))
    assert (L.table > 0) == bool(dense), "%s: %d launches read the table" % (tag, L.table)
    _assert_rows(L.rows, mode == 2 and decides, tag)
    return got, L.rows, tag


# ---- A, B, C: the wave kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim,which", HANDLES, ids=_ids(HANDLES))
def test_wave_kernel(eng, handles, tune, dim, which):
    """A: HNSW_WAVE = 2, rejection mode 2 and 0, the visited set in LDS and in HBM stamps; once through device buffers."""
    h = handles(dim, which)
    for ef in EFS:
        for mode in (2, 0):
            for vis_global in (0, 1):
                for dev in ((0, 1) if (mode, vis_global) == (2, 0) else (0,)):
                    got, _, tag = _wave_launch(eng, h.idx, tune, h.Q, K, ef, mode, vis_global, False, False, dev)
                    h.check(got, ef, 0, NQ, "wave kernel, " + tag)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,which", HANDLES, ids=_ids(HANDLES))
def test_wave_kernel_ordered(eng, handles, tune, dim, which):
    """B: HNSW_ORDER = 2 -- slots and queries differ."""
    h = handles(dim, which)
    for ef in EFS:
        got, _, tag = _wave_launch(eng, h.idx, tune, h.Q, K, ef, 2, 0, True, False, 0)
        h.check(got, ef, 0, NQ, "wave kernel, " + tag)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,which", HANDLES, ids=_ids(HANDLES))
def test_wave_kernel_with_the_dense_table(eng, handles, tune, dim, which):
    """C: the bounds from the table, plain and ordered, through device and host buffers: the results AND the handle's (f32 rows,
    neighbours) pair equal those of the launch that computes its bounds (family A's).  The table of a row-strided query block
    (qld > dim beside ld != dim: the only entry that takes one) equals the contiguous block's and, for the first queries, the
    traversal's own bounds."""
    h = handles(dim, which)
    for ef in EFS:
        for ordered in (False, True):
            for dev in (0, 1):
                got0, rows0, tag0 = _wave_launch(eng, h.idx, tune, h.Q, K, ef, 2, 0, ordered, False, dev)
                got2, rows2, tag2 = _wave_launch(eng, h.idx, tune, h.Q, K, ef, 2, 0, ordered, True, dev)
                h.check(got0, ef, 0, NQ, "wave kernel, " + tag0)
                h.check(got2, ef, 0, NQ, "wave kernel, " + tag2)
                assert rows2 == rows0, "%s ef %d: (f32 rows, neighbours) %s with the table, %s without" % (h.what, ef, rows2, rows0)
    wide = np.full((NQ, dim + 24), np.nan, np.float32)      # what lies between the queries is not read
    wide[:, :dim] = h.Q
    view = wide[:, :dim]
    assert view.strides[0] == 4 * (dim + 24)
    tab, flat = h.idx.hnsw_dense_bounds(view), h.idx.hnsw_dense_bounds(h.Q)
    assert tab.shape == (NQ, N) and not np.isnan(flat).any()
    np.testing.assert_array_equal(tab.view(np.uint32), flat.view(np.uint32), err_msg=h.what + ": the table of a strided block")
    every = np.arange(N, dtype=np.int32)
    for q in (0, NQ - 2, NQ - 1):
        np.testing.assert_array_equal(flat[q].view(np.uint32), h.idx.hnsw_rejection_bounds(h.Q[q], every).view(np.uint32),
                                      err_msg="%s: the table's row %d against the traversal's own bounds" % (h.what, q))


# ---- D: the single-workgroup kernel -----------------------------------------------------------------------------------------------
def _search_kernel_launch(eng, idx, tune, Q, k, ef, nw, mode, vis_global, decides=True):
    tune.set("HNSW_WAVE", 0)
    tune.set("PREFETCH", 0)
    tune.set("HNSW_NW", nw)
    tune.set("VIS_GLOBAL", vis_global)
    idx.set_rejection_test(mode)
    L = _Launches(eng, idx)
    got = idx.hnsw_search(Q, k, ef, want_stats=True)
    L.done()
    tag = "single-workgroup kernel, %d waves, rejection %d, stamps %d" % (nw, mode, vis_global)
    assert L.rose == {"hnsw_rejection" if mode == 2 else "hnsw_plain"}, "%s: launch counters that rose: %s" % (tag, sorted(L.rose))
    _assert_rows(L.rows, mode == 2 and decides, tag)
    return got, tag


@pytest.mark.gpu
@pytest.mark.parametrize("dim,which", HANDLES, ids=_ids(HANDLES))
def test_single_workgroup_kernel(eng, handles, tune, dim, which):
    """D: HNSW_WAVE = 0, 1 / 2 / 4 waves per query (HBM stamps at 4), rejection mode 2 and 0."""
    h = handles(dim, which)
    for ef in EFS:
        for nw in (1, 2, 4):
            for mode in (2, 0):
                got, tag = _search_kernel_launch(eng, h.idx, tune, h.Q, K, ef, nw, mode, 1 if nw == 4 else 0)
                h.check(got, ef, 0, NQ, tag)


# ---- E, F: the small launches -----------------------------------------------------------------------------------------------------
def _small_launches(eng, h, tune, counter, tag):
    for ef in EFS:
        for lo, hi in BATCHES:
            L = _Launches(eng, h.idx)
            got = h.idx.hnsw_search(h.Q[lo:hi], K, ef, want_stats=True)
            L.done()
            assert L.rose == {counter}, "%s: launch counters that rose: %s" % (tag, sorted(L.rose))
            _assert_rows(L.rows, False, tag)
            h.check(got, ef, lo, hi, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,which", HANDLES, ids=_ids(HANDLES))
def test_helper_kernel(eng, handles, tune, dim, which):
    """E: SOLO = 0 -- the round-2 helper kernel, batches of 1, 3 and 48; its helpers evaluate (PF_EVAL 1: the traversal's own int8
    test is off) or only warm the L2 (0: the instantiation that keeps the int8 test)."""
    h = handles(dim, which)
    tune.set("SOLO", 0)
    tune.unset("PREFETCH")
    tune.unset("HNSW_NW")
    tune.set("VIS_GLOBAL", 0)
    for pf_eval in (1, 0):
        tune.set("PF_EVAL", pf_eval)
        _small_launches(eng, h, tune, "hnsw_helpers", "helper kernel, PF_EVAL %d" % pf_eval)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,which", HANDLES, ids=_ids(HANDLES))
def test_several_cu_kernel(eng, handles, tune, dim, which):
    """F: SOLO = 2 -- one query over several CUs, batches of 1, 3 and 48."""
    h = handles(dim, which)
    tune.set("SOLO", 2)
    tune.unset("PREFETCH")
    tune.unset("HNSW_NW")
    tune.set("VIS_GLOBAL", 0)
    _small_launches(eng, h, tune, "hnsw_solo", "several-CU kernel")


# ---- G: the repeat pass -----------------------------------------------------------------------------------------------------------
TIE_MANY = next(c for c, _ in sg.scenarios() if c.name.startswith("S-tie-many"))
SCRIPTED_AT = (0, 3, 8, 9, 31, 47)      # places of the scripted query among the 48


def embed_wide(case, metric, dim):
    """scripted_graphs.embed with every component in use: rows (n, dim) f32 and the scripted query.  l2: row = value * u / 64 for one
    direction u without a zero, the query -u / 8: the distance grows with the value.  cosine, dot: r (cos t * u + sin t * w) for
    orthonormal u, w, t growing with the value, the query u.  Equal values give the same row, hence the same distance bits; that
    distinct values keep their strict order in the device's arithmetic is asserted by check_embedding on the distances."""
    assert (np.asarray(case.signs) == 1).all()
    rs = np.random.RandomState(1000 + dim)
    u = rs.uniform(0.5, 1.5, dim) * rs.choice([-1.0, 1.0], dim)
    u /= np.linalg.norm(u)
    v = np.asarray(case.values, np.float64)
    if metric == "l2":
        return (v[:, None] * u[None, :] / 64.0).astype(np.float32), (-u / 8.0).astype(np.float32)
    w = rs.uniform(0.5, 1.5, dim) * rs.choice([-1.0, 1.0], dim)
    if dim > 1:
        w -= (w @ u) * u
    w /= np.linalg.norm(w)
    t = (v + 200.0) * (2.4 / (sg.MAX_VALUE + 200))
    r = 1.0 + (v % 5) * 0.25 if metric == "cosine" else np.full(len(v), 2.0)
    return (r[:, None] * (np.cos(t)[:, None] * u[None, :] + np.sin(t)[:, None] * w[None, :])).astype(np.float32), u.astype(np.float32)


def scripted_launch(O, metric, dim):
    """(rows, graph, 48 queries, ef, k, the oracle's device-order answer): the scripted query at SCRIPTED_AT among rows of the graph;
    the CPU side of the repeat pass's precondition is asserted here."""
    case = TIE_MANY
    ef, = case.efs
    k = sg.result_k(ef)
    rows, q = embed_wide(case, metric, dim)
    g = sg.graph(O, case)
    pick = np.random.RandomState(dim).choice(len(rows), NQ, replace=False)
    Q = rows[pick].copy()
    Q[list(SCRIPTED_AT)] = q
    ref = O.hnsw_search(rows, g, Q, k, ef=ef, metric=O.METRICS[metric], mode=O.MODE_DEV)[:3]
    what = "S-tie-many %s dim %d" % (metric, dim)
    dist, traces = check_traces(O, g, rows, Q, metric, {ef: ref}, what)
    sg.check_embedding(case.values, dist[SCRIPTED_AT[0]])
    over = [overflows(tr, dist[i]) for i, tr in enumerate(traces[ef])]
    never = [cannot_overflow(tr) for tr in traces[ef]]
    assert all(over[i] for i in SCRIPTED_AT), what + ": the scripted query does not run out of room for its ties"
    assert sum(never) >= 8 and not any(over[i] and never[i] for i in range(NQ)), \
        "%s: %d queries of the launch provably need no repeat pass" % (what, sum(never))
    return rows, g, Q, ef, k, ref


def test_the_scripted_launch_reaches_the_repeat_pass(oracle):
    """The precondition itself, without a GPU, at the smallest and at a padded dim (the GPU test asserts it at every dim)."""
    for metric, dim in (("l2", 5), ("cosine", 257), ("dot", 1030)):
        scripted_launch(oracle, metric, dim)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,which", HANDLES, ids=_ids(HANDLES))
def test_repeat_pass(eng, oracle, tune, dim, which):
    """G: families A - D on a launch in which six queries overflow their first-pass lists and others provably do not."""
    metric = "l2" if which == "l2" else ALT_METRIC_OF[dim]
    rows, g, Q, ef, k, (oi, od, ost) = scripted_launch(oracle, metric, dim)

    def check(got, tag):
        tag = "S-tie-many %s dim %d, %s" % (metric, dim, tag)
        np.testing.assert_array_equal(got[2], ost, err_msg=tag + ": counters")
        assert_exact(got[0], got[1], oi, od, tag)

    with eng.Index(rows, metric) as idx:
        idx.set_rejection_test(2)
        idx.set_graph(g)
        idx.set_profiling(True)
        for mode in (2, 0):
            for vis_global in (0, 1):
                for dev in (0, 1):
                    got, _, tag = _wave_launch(eng, idx, tune, Q, k, ef, mode, vis_global, False, False, dev, decides=False)
                    check(got, tag)
        for dense in (False, True):
            got, _, tag = _wave_launch(eng, idx, tune, Q, k, ef, 2, 0, True, dense, 1, decides=False)
            check(got, tag)
        got, _, tag = _wave_launch(eng, idx, tune, Q, k, ef, 2, 0, False, True, 0, decides=False)
        check(got, tag)
        for nw in (1, 2, 4):
            for mode in (2, 0):
                got, tag = _search_kernel_launch(eng, idx, tune, Q, k, ef, nw, mode, 1 if nw == 4 else 0, decides=False)
                check(got, tag)
