"""Observers of what a live-index mutation leaves BESIDE the f32 rows (include/hnswgpu.h: hnswgpu_ivf_add / _remove / _update,
hnswgpu_lsh_add / _remove, hnswgpu_hnsw_add / _remove): the base-order int8 rows and their meta, the list-order int8 tiles, the
list-order half-precision copy.  The saved file does not carry these copies and a search at test size reads them only through
bounds that decide what is NOT computed, so a stale or wrongly remade copy that still bounds validly changes no result.  Every
function here takes (mutated, fresh, Q, ...) -- the handle that went through the mutation, a handle made from scratch over the same
rows as the header's equivalence says, float32 queries -- and asserts equality of BITS (uint32 views: NaN equals NaN) through the
diagnostic entries that read a copy directly, or through the counters of a search forced through it.  matches_f64 does not depend
on the fresh handle: it is the plain high-precision reference.

A helper module, not a conftest: the tests that use it are test_mutation_widths_gpu.py and test_mutation_scenarios_gpu.py."""
import numpy as np

from ivf_add_model import f64_distances
from util import assert_topk_parity, metric_scale

K = 10
HOME_QUERIES = 20          # more than one group of the home-list pass holds at wide rows (home_group: 16 queries and fewer)
# The forced passes of same_list_tiles.  IVF_CODES / STREAM_MID = 1: the int8 bounds pass and the half-precision pass from one
# query on (production: 48 pairs per list / 1.5 M candidates).  The bounds pass drops candidates against the threshold the routing
# step seeded and never lowers it, so WHICH candidates it appends to a query's survivor list is a function of the data; their
# order is not.  One slice per pass: the half-precision pass sees a query's whole list in one workgroup, takes ONE threshold from
# it -- the k-th smallest of its 256 threads' smallest upper bounds -- and compacts the list; the finish kernel's one workgroup
# walks what is left in one step per wave, against the threshold it was launched with.  With more than 256 entries a thread holds
# several and the threshold depends on the order of the list, so STREAM_CAP = 256: a longer list overflows (by its COUNT) and
# the query takes the fallback, which evaluates every candidate.  Under these four settings and the cap the (survivors,
# candidates) pair is a function of the codes, the half rows, the lists and the queries; same_list_tiles still asserts "the
# fresh handle read twice gives equal counters" as its precondition before it compares the handles.
FORCED_PASSES = {"IVF_CODES": 1, "STREAM_MID": 1, "MID_SLICES": 1, "FINISH_SLICES": 1, "STREAM_CAP": 256}
# The counted traversals of same_hnsw_searches.  A small launch spreads a query over several CUs whose fetchers evaluate
# neighbours AHEAD of the sequencer (solo_kernels.hpp; the round-2 helpers prefetch likewise): how many f32 rows they fetch
# depends on who got where first -- measured on one handle read twice: (1440, 1895) then (1416, 1895), the neighbours equal, the
# rows not.  PREFETCH = 0 takes both away, HNSW_WAVE = 2 gives every launch the one-wave-per-query kernel: a query's traversal
# then runs in program order and both counters are functions of the graph, the rows, the codes and the queries.
COUNTED_TRAVERSAL = {"PREFETCH": 0, "HNSW_WAVE": 2}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b, what):
    """(ids, distances[, stats]) of two searches: ids, distance bits and stats equal."""
    np.testing.assert_array_equal(a[0], b[0], err_msg=what + ": ids")
    np.testing.assert_array_equal(bits(a[1]), bits(b[1]), err_msg=what + ": distance bits")
    if len(a) > 2:
        np.testing.assert_array_equal(a[2], b[2], err_msg=what + ": stats")


def three_queries(Q, row):
    """A generated query, a base row of the handle (`row`: its own code meets itself; left out where the handle is empty), the
    zero query (no bound under cosine: NaN on both sides)."""
    qs = [np.ascontiguousarray(Q[0], np.float32), np.zeros(Q.shape[1], np.float32)]
    if row is not None:
        qs.insert(1, np.ascontiguousarray(row, np.float32))
    return qs


def _outcome(call):
    """("ok", arrays) or ("refused", error code) of a bounds entry."""
    from hnsw_clj_amd._native import HnswGpuError

    try:
        out = call()
    except HnswGpuError as e:
        return "refused", e.code
    return "ok", [bits(x) for x in (out if isinstance(out, tuple) else (out,))]


def _same_outcome(m, f, what):
    assert m[0] == f[0], "%s: the mutated handle %s, the fresh one %s" % (what, m, f)
    if m[0] == "refused":
        assert m[1] == f[1], "%s: refused with code %d, the fresh handle with %d" % (what, m[1], f[1])
        return False
    for side, (x, y) in enumerate(zip(m[1], f[1])):
        bad = np.flatnonzero(x.ravel() != y.ravel())
        assert bad.size == 0, "%s: %d of %d bounds differ (side %d), first at %d: %#x, fresh %#x" % (
            what, bad.size, x.size, side, bad[0], x.ravel()[bad[0]], y.ravel()[bad[0]])
    return True


def touch(ix, Q):
    """Make the copies a handle makes lazily exist BEFORE a mutation (the base-order int8 rows of a handle without a graph come
    with the first bounds call): a chain remakes only the copies the handle holds.  Returns nothing; a handle that makes no
    int8 rows (mode 0, mode 1 below dim 128) refuses, which is fine."""
    if ix.n > 0:
        _outcome(lambda: ix.distance_bounds(Q[0], np.arange(ix.n, dtype=np.int32)))


def same_base_codes(mutated, fresh, Q, row=None, expect=None):
    """Base-order int8 rows + meta: distance_bounds (both sides) and rejection_bounds of every row, three queries.  On a handle
    without int8 rows both refuse alike.  expect: True / False where the caller knows whether the rows exist."""
    n = mutated.n
    assert fresh.n == n
    every = np.arange(n, dtype=np.int32)
    for j, q in enumerate(three_queries(Q, row)):
        for name in ("distance_bounds", "rejection_bounds"):
            m = _outcome(lambda: getattr(mutated, name)(q, every))
            f = _outcome(lambda: getattr(fresh, name)(q, every))
            ok = _same_outcome(m, f, "%s, query %d" % (name, j))
            if expect is not None and n > 0:
                assert ok == expect, "%s: %s where int8 rows %s expected" % (name, m[0], "were" if expect else "were not")


def same_graph_codes(mutated, fresh, Q, row=None):
    """Graph handles: the traversals' own bounds (int8 rows against the 16-bit query code) of every row, three queries."""
    n = mutated.n
    every = np.arange(n, dtype=np.int32)
    for j, q in enumerate(three_queries(Q, row)):
        _same_outcome(_outcome(lambda: mutated.hnsw_rejection_bounds(q, every)), _outcome(lambda: fresh.hnsw_rejection_bounds(q, every)),
                      "hnsw_rejection_bounds, query %d" % j)


def same_list_half(mutated, fresh, Q, row=None, expect=None):
    """List-order half-precision copy + meta: ivf_half_bounds (both sides) of every list position, three queries."""
    n = mutated.n
    every = np.arange(n, dtype=np.int32)
    for j, q in enumerate(three_queries(Q, row)):
        ok = _same_outcome(_outcome(lambda: mutated.ivf_half_bounds(q, every)), _outcome(lambda: fresh.ivf_half_bounds(q, every)),
                           "ivf_half_bounds, query %d" % j)
        if expect is not None and n > 0:
            assert ok == expect, "ivf_half_bounds answered: %s, a half copy %s expected" % (ok, "was" if expect else "was not")


def home_ranges(off, changed_list):
    """The three ranges of same_home_pass from the lists' offsets: the whole index; the list `changed_list`; 37 rows that
    straddle a list boundary and end inside a 16-row block (counted from the range's start AND from position 0)."""
    off = np.asarray(off, np.int64)
    n = int(off[-1])
    out = [(0, n)]
    if off[changed_list + 1] > off[changed_list]:
        out.append((int(off[changed_list]), int(off[changed_list + 1])))
    for b in off[1:-1]:
        for before in range(20, 0, -1):                      # 37 is no multiple of 16: the range ends inside a block of its own
            r0, r1 = int(b) - before, int(b) - before + 37
            if 0 <= r0 < b < r1 <= n and r1 % 16 != 0:
                out.append((r0, r1))
                return out
    return out


def same_home_pass(mutated, fresh, Q, ranges, expect=None):
    """The matrix-core half-precision pass of large batches (rows of whole 128-element steps): ivf_home_bounds of HOME_QUERIES
    queries over each (row_begin, row_end) of `ranges`, both sides."""
    assert len(Q) >= HOME_QUERIES
    Qh = np.ascontiguousarray(Q[:HOME_QUERIES], np.float32)
    for r0, r1 in ranges:
        ok = _same_outcome(_outcome(lambda: mutated.ivf_home_bounds(Qh, r0, r1)), _outcome(lambda: fresh.ivf_home_bounds(Qh, r0, r1)),
                           "ivf_home_bounds rows [%d, %d)" % (r0, r1))
        if expect is not None:
            assert ok == expect, "ivf_home_bounds rows [%d, %d) answered: %s" % (r0, r1, ok)


def _forced(call, settings=None):
    """Run `call` with FORCED_PASSES (or `settings`) set; every key goes back to what it was."""
    from hnsw_clj_amd import _native

    settings = FORCED_PASSES if settings is None else settings
    saved = {name: _native.get_tuning(name) for name in settings}
    try:
        for name, v in settings.items():
            _native.set_tuning(name, v)
        return call()
    finally:
        for name, v in saved.items():
            _native.set_tuning(name, v)


def _counted(ix, search):
    ix.set_profiling(True)
    try:
        ix.rejection_stats(reset=True)
        res = search(ix)
        return res, ix.rejection_stats(reset=True)
    finally:
        ix.set_profiling(False)


def same_list_tiles(mutated, fresh, Q, nq=12, expect=None):
    """List-order int8 tiles + meta (no entry reads them directly): searches forced through the bounds pass and the
    half-precision pass at test size -- ids and distance bits equal, and so the (survivors, candidates) pair of rejection_stats:
    a looser-but-valid code changes no result, it lets more candidates through.  Precondition, asserted: the fresh handle read
    twice gives equal counters (FORCED_PASSES says when that holds).  expect: True where the passes must have run."""
    nlist = mutated.nlist
    assert fresh.nlist == nlist
    for k, nprobe in ((K, min(3, nlist)), (1, min(2, nlist))):
        def run():
            search = lambda ix: ix.ivf_search(Q[:nq], k, nprobe)   # noqa: E731
            return _counted(fresh, search), _counted(fresh, search), _counted(mutated, search)

        f1, f2, m = _forced(run)
        what = "forced passes, k %d nprobe %d" % (k, nprobe)
        print("%s: fresh %s, fresh again %s, mutated %s" % (what, f1[1], f2[1], m[1]))
        same(f1[0], f2[0], what + ", the fresh handle twice")
        assert f1[1] == f2[1], "%s: the counters of the fresh handle are no function of the data: %s then %s" % (what, f1[1], f2[1])
        same(m[0], f1[0], what)
        assert m[1] == f1[1], "%s: (survivors, candidates) %s, the fresh handle %s" % (what, m[1], f1[1])
        if expect and mutated.n > 0:
            surv, cand = m[1]
            assert 0 < surv <= cand, "%s: the bounds pass did not run: %s" % (what, m[1])
        if expect is False:
            assert m[1] == (0, 0), "%s: a handle without int8 tiles counted %s" % (what, m[1])


def same_hnsw_searches(mutated, fresh, Q):
    """Traversals at ef 10 and 64: ids, distance bits and the per-query stats pairs by the kernels the suite's settings choose,
    then the same under COUNTED_TRAVERSAL with the rejection_stats pair (f32 rows fetched, neighbours evaluated) while profiling
    is on -- what the int8 rows decide, which no result shows.  Precondition, asserted: the fresh handle read twice gives equal
    counters."""
    for ef in (10, 64):
        search = lambda ix: ix.hnsw_search(Q, K, ef, want_stats=True)   # noqa: E731
        same(search(mutated), search(fresh), "hnsw_search ef %d" % ef)
        f1, f2, m = _forced(lambda: (_counted(fresh, search), _counted(fresh, search), _counted(mutated, search)), COUNTED_TRAVERSAL)
        what = "counted hnsw_search ef %d" % ef
        print("%s: fresh %s, fresh again %s, mutated %s" % (what, f1[1], f2[1], m[1]))
        same(f1[0], f2[0], what + ", the fresh handle twice")
        assert f1[1] == f2[1], "%s: the counters of the fresh handle are no function of the data: %s then %s" % (what, f1[1], f2[1])
        same(m[0], f1[0], what)
        assert m[1] == f1[1], "%s: (f32 rows, neighbours) %s, the fresh handle %s" % (what, m[1], f1[1])


def matches_f64(mutated, rows, metric, Q, nq=8):
    """The plain high-precision reference, independent of any fresh handle: exact_knn(Q, 10) on the mutated handle against a
    float64 numpy brute force over `rows`, the rows it holds now by the caller's bookkeeping (util.assert_topk_parity: 1e-4
    relative + 1e-6 absolute, the bar of BASELINE.json's north star), and lb <= batch_distances <= ub from the int8 rows wherever
    neither side is NaN."""
    rows = np.ascontiguousarray(rows, np.float32)
    n = len(rows)
    assert mutated.n == n
    if n == 0:
        return
    Qn = np.ascontiguousarray(Q[:nq], np.float32)
    k = min(K, n)
    D = f64_distances(metric, Qn, rows)                      # [nq, n]: cosine 1 - cos, l2 rooted, dot negated
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    gi, gd = mutated.exact_knn(Qn, k)
    assert_topk_parity(gi, gd, order.astype(np.int32), np.take_along_axis(D, order, axis=1), "exact_knn against f64",
                       scale=metric_scale(metric, Qn, rows))
    every = np.arange(n, dtype=np.int32)
    for j, q in enumerate(three_queries(Q, rows[n // 2])):
        got = _outcome(lambda: mutated.distance_bounds(q, every))
        if got[0] == "refused":                              # no int8 rows on this handle
            continue
        d = mutated.batch_distances(q)
        lb, ub = (x.view(np.float32) for x in got[1])
        with np.errstate(invalid="ignore"):
            low, high = lb > d, d > ub                       # (False wherever a side is NaN)
        assert not low.any(), "query %d: a lower bound above the distance at rows %s" % (j, np.flatnonzero(low)[:5])
        assert not high.any(), "query %d: an upper bound below the distance at rows %s" % (j, np.flatnonzero(high)[:5])
