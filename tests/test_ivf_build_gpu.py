"""IVF construction on the device -- hnswgpu_kmeanspp, hnswgpu_ivf_build, hnswgpu_list_means / hnswgpu_list_sums and the
lightning mirror built on them -- against the CPU oracle on rows made for the purpose (tests/kmeans_inputs.py; their
premises are pinned without a GPU by tests/test_ivf_build_host.py).  Nothing here carries a tolerance except the float64
leg of the lightning searches, which uses the suite's own 1e-4.

  A  the seeding's bounds pass at every row-loader width, against the plain f32 pass and the oracle
  B  the two-level D^2 sampling walk: several blocks, block edges, zero total weight, nlist > n, n = 1
  C  the whole build: picks, assignments, centroid bits, lists; empty lists keep their centroid and stay searchable
  D  list sums / means: sequential float64 addition in list order, bit for bit
  E  lightning searches against the oracle over the index's own lists
  F  lightning's smart partition
"""
import functools
import random

import numpy as np
import pytest

import kmeans_inputs as ki
from util import assert_exact, assert_topk_parity

pytestmark = pytest.mark.gpu

METRIC = {"cosine": 0, "l2": 1, "dot": 2}
N, NLIST = 1100, 24          # three seed workgroups of 512 rows; the last one ends with a group of 8 that holds 4 rows
DIMS = [3, 100, 257, 300, 768, 1000, 1100, 1536, 2048, 2500, 3072]      # the seven widths, ld padding, half-empty last chunks


@pytest.fixture(scope="module")
def eng(native_lib):
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    return engine


# ---- inputs and oracle results, computed once and shared ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows(family, n, dim):
    from oracle import oracle as O

    if family == "clustered":
        base = ki.clustered(O, n, dim)
    elif family == "gaussian":
        base = ki.gaussian(O, n, dim)
    elif family == "lattice":
        base = ki.lattice(n, dim)
    elif family == "duplicates":
        base = ki.duplicates(dim)
    elif family == "all_equal":
        base = ki.all_equal(n, dim)
    else:
        raise KeyError(family)
    assert len(base) == n
    base.setflags(write=False)
    return base


@functools.lru_cache(maxsize=None)
def _built(family, n, dim, metric, nlist, iters, assign_mode=None):
    """oracle.ivf_build_dev: (picks, centroids, assignments) in the engine's arithmetic."""
    from oracle import oracle as O

    out = O.ivf_build_dev(_rows(family, n, dim), nlist, iters, METRIC[metric], 42, assign_mode=assign_mode)
    for a in out:
        a.setflags(write=False)
    return out


def _lists_of(idx, n, nlist):
    """get_ivf of a built handle -> (centroids, off, lids, assignment); ids ascend inside every list."""
    cen, off, lids = idx.get_ivf()
    assert len(off) == nlist + 1 and off[0] == 0 and off[-1] == n
    assign = np.full(n, -1, np.int32)
    for l in range(nlist):
        members = lids[off[l]:off[l + 1]]
        assert np.all(np.diff(members) > 0), "list %d is not in index order" % l
        assign[members] = l
    assert (assign >= 0).all()
    return cen, off, lids, assign


def _centroids_by_the_rule(base, picks, assigns):
    """The centroids of a build, restated from its rule alone: a list's centroid is the sequential float64 mean (rounded to
    float32) of its members in the LAST pass in which it had any, and its seeding row if it never had one."""
    cen = np.array(base[picks])
    for a in assigns:
        off, lids = np.concatenate(([0], np.cumsum(np.bincount(a, minlength=len(picks))))), np.argsort(a, kind="stable")
        means = ki.sequential_means(base, off, lids)
        live = np.diff(off) > 0
        cen[live] = means[live]
    return cen


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    np.testing.assert_array_equal(got.view(u), want.view(u), err_msg=what)


# ---- leg A / B: the seeding ----------------------------------------------------------------------------------------------------
def _picks_three_ways(eng, tune, base, metric, nlist, want, what, share=True):
    """hnswgpu_kmeanspp by the bounds pass (the suite's default: every handle has int8 rows), on a handle without int8
    rows, and with the bounds pass switched off: all three must make the oracle's picks.  Returns the share of
    (round >= 2, row) pairs the bounds pass may skip (kmeans_inputs.skip_share), from the index's own bounds."""
    from oracle import oracle as O

    n = len(base)
    got = {}
    skip = None
    with eng.Index(base, metric) as idx:
        got["bounds pass"] = idx.kmeanspp(nlist, 42)
        if share and nlist > 2:
            dist = ki.seeding_distances(O, base, METRIC[metric], want)
            rows = np.arange(n, dtype=np.int32)
            skip = ki.skip_share(dist, lambda r: idx.rejection_bounds(base[want[r]], rows))
            print("skip-share %-28s %.3f" % (what, skip))
        else:
            idx.rejection_bounds(base[0], np.zeros(1, np.int32))          # (raises on a handle without int8 rows)
    with eng.Index(base, metric) as idx:
        idx.set_rejection_test(0)
        got["handle without int8 rows"] = idx.kmeanspp(nlist, 42)
        with pytest.raises(Exception, match="no int8 rows"):
            idx.rejection_bounds(base[0], np.zeros(1, np.int32))
    tune.set("SEED_BOUNDS", 0)
    try:
        with eng.Index(base, metric) as idx:
            got["SEED_BOUNDS = 0"] = idx.kmeanspp(nlist, 42)
    finally:
        tune.restore()
    for name, picks in got.items():
        diff = ki.first_difference(picks, want)
        assert not diff, "%s, %s: %s" % (what, name, diff)
    return skip


LEG_A = ([("clustered", d, m) for d in DIMS for m in ("cosine", "l2", "dot")] +
         [("gaussian", d, m) for d in DIMS for m in ("cosine", "l2")] +
         [("duplicates", d, "cosine") for d in (300, 1536, 3072)] +
         [("lattice", d, m) for d in (24, 300, 1536, 3072) for m in ("l2", "dot")])


@pytest.mark.parametrize("family,dim,metric", LEG_A)
def test_seeding_at_every_row_width(eng, oracle, tune, family, dim, metric):
    """Leg A.  One bound that is too high leaves a stale minimum and moves every later D^2 pick; on `duplicates` the picks
    after the 7th are drawn from the last bits of the minima, on `lattice` they are the float64 reference's as well, and
    on `gaussian` rows -- all at nearly the same distance from one another -- most rows improve by a hair in every round,
    which is where a bound a little too high hides an improvement (clustered rows leave that band almost empty).
    The floor on the skip share is a coverage condition: it shows that the bounds pass had rows to reject."""
    O = oracle
    n, nlist = (420, 20) if family == "duplicates" else (N, NLIST)
    base = _rows(family, n, dim)
    want = _built(family, n, dim, metric, nlist, 0)[0]
    what = "%s %s dim=%d" % (family, metric, dim)
    if family == "lattice":
        np.testing.assert_array_equal(want, O.kmeanspp(base, nlist, METRIC[metric], 42), err_msg=what)
    skip = _picks_three_ways(eng, tune, base, metric, nlist, want, what)
    if family == "clustered" and metric in ("cosine", "l2"):
        assert skip >= 0.25, "%s: the bounds pass could skip only %.3f of the rows" % (what, skip)
    if family == "clustered" and metric == "dot" and dim <= 256:
        assert skip > 0, what


LEG_B = ([("lattice", 9001, 8, 40, m) for m in ("l2", "dot")] +                    # three blocks of 4096, the last with 809 rows
         [("clustered", 9001, 8, 40, m) for m in ("cosine", "l2", "dot")] +
         [("clustered", n, 8, 24, m) for n in (4096, 4097) for m in ("cosine", "l2")] +
         [("clustered", 3, 8, 5, m) for m in ("cosine", "l2")] +                   # nlist > n
         [("clustered", 1, 8, 1, "cosine"), ("clustered", 1, 8, 3, "cosine"), ("clustered", 1, 8, 3, "l2")])


@pytest.mark.parametrize("family,n,dim,nlist,metric", LEG_B)
def test_sampling_walk(eng, oracle, tune, family, n, dim, nlist, metric):
    """Leg B.  The D^2 sample is found by f64 block sums of 4096 entries and a walk through one block on the host."""
    O = oracle
    base = _rows(family, n, dim)
    want = _built(family, n, dim, metric, nlist, 0)[0]
    what = "%s %s n=%d nlist=%d" % (family, metric, n, nlist)
    if family == "lattice":
        np.testing.assert_array_equal(want, O.kmeanspp(base, nlist, METRIC[metric], 42), err_msg=what)
    if n > 4097:
        assert len(set((want // 4096).tolist())) == 3, "the picks should come from all three blocks"
    _picks_three_ways(eng, tune, base, metric, nlist, want, what, share=n > 4097)
    if nlist > n:
        _build_with_more_lists_than_rows(eng, base, family, n, dim, metric, nlist, what)


def _build_with_more_lists_than_rows(eng, base, family, n, dim, metric, nlist, what):
    """nlist exceeds the number of distinct rows: equal centroids send every row to the lowest index, the other lists come
    out empty and keep their centroid through the Lloyd passes."""
    picks = _built(family, n, dim, metric, nlist, 0)[0]
    with eng.Index(base, metric) as idx:
        idx.ivf_build(nlist, 0, 42)
        cen, off, lids, assign = _lists_of(idx, n, nlist)
        np.testing.assert_array_equal(assign, _built(family, n, dim, metric, nlist, 0)[2], err_msg=what)
        _same_bits(cen, base[picks], what + ": centroids of a build without Lloyd passes are the seeding rows")
        first = {}
        for l in range(nlist):                                                      # the lowest list of every distinct centroid
            first.setdefault(cen[l].tobytes(), l)
        lowest = np.array([first[cen[l].tobytes()] for l in range(nlist)])
        np.testing.assert_array_equal(assign, lowest[assign], err_msg=what + ": a row went to a later copy of its centroid")
        assert len(first) < nlist
        idx.ivf_build(nlist, 2, 42)
        cen2, off2, lids2, assign2 = _lists_of(idx, n, nlist)
        _, wcen, wassign = _built(family, n, dim, metric, nlist, 2)
        np.testing.assert_array_equal(assign2, wassign, err_msg=what)
        _same_bits(cen2, wcen, what + ": centroids after two passes")
        assert not np.isnan(cen2).any()
        assign1 = _built(family, n, dim, metric, nlist, 1)[2]                       # (what the second pass's means came from)
        never_used = np.setdiff1d(np.arange(nlist), np.unique(np.concatenate([assign, assign1, assign2])))
        assert len(never_used) > 0
        _same_bits(cen2[never_used], base[picks[never_used]], what + ": an empty list keeps its centroid")


@pytest.mark.parametrize("family,n,dim,nlist", [("all_equal", 5000, 8, 6), ("duplicates", 420, 300, 20)])
def test_sampling_walk_with_no_weight_left(eng, oracle, tune, family, n, dim, nlist):
    """Leg B.  Under L2 a self-distance is exactly 0: once every distinct row is a centre the total weight is 0 (two blocks
    of zeros for n = 5000) and every further pick is row 0; then nlist exceeds the number of distinct rows."""
    base = _rows(family, n, dim)
    want = _built(family, n, dim, "l2", nlist, 0)[0]
    distinct = len(np.unique(base, axis=0))
    assert len(np.unique(base[want[:distinct]], axis=0)) == distinct and (want[distinct:] == 0).all()
    what = "%s l2 n=%d" % (family, n)
    _picks_three_ways(eng, tune, base, "l2", nlist, want, what, share=False)
    _build_with_more_lists_than_rows(eng, base, family, n, dim, "l2", nlist, what)


# ---- leg C: the whole build ----------------------------------------------------------------------------------------------------
LEG_C = [("l2", 1536), ("l2", 3072), ("cosine", 300), ("cosine", 1100), ("cosine", 2500), ("dot", 300), ("dot", 1100), ("dot", 2500)]


@pytest.mark.parametrize("tile", ["default", "TILE=0"])
@pytest.mark.parametrize("metric,dim", LEG_C)
def test_whole_build(eng, oracle, tune, metric, dim, tile):
    """Leg C.  ivf_build(nlist, 2, 42) against the restatement of its arithmetic.  L2 above dim 1024 assigns by the GEMV
    scan instead of the register-row tiles; TILE = 0 sends cosine / dot there as well."""
    O = oracle
    base = _rows("clustered", N, dim)
    assign_mode = O.MODE_DEV if (tile == "TILE=0" or metric == "l2") else O.MODE_MFMA
    picks, wcen, wassign = _built("clustered", N, dim, metric, NLIST, 2, assign_mode)
    what = "%s dim=%d %s" % (metric, dim, tile)
    if tile == "TILE=0":
        tune.set("TILE", 0)
    with eng.Index(base, metric) as idx:
        diff = ki.first_difference(idx.kmeanspp(NLIST, 42), picks)
        assert not diff, what + ": " + diff
        idx.ivf_build(NLIST, 2, 42)
        cen, off, lids, assign = _lists_of(idx, N, NLIST)
    np.testing.assert_array_equal(assign, wassign, err_msg=what)
    woff, wlids = O.lists_from_assign(wassign, NLIST)
    np.testing.assert_array_equal(off, woff, err_msg=what)
    np.testing.assert_array_equal(lids, wlids, err_msg=what)
    _same_bits(cen, wcen, what + ": centroids")


@pytest.mark.parametrize("dim", [24, 300, 1536, 3072])
def test_whole_build_with_empty_lists(eng, oracle, dim):
    """Leg C.  Lattice rows under dot leave many lists empty: such a list keeps its centroid (its seeding row while it
    has never had a member), no 0 / 0 reaches a centroid, the assignments are the float64 reference's as well, and the
    handle is searchable."""
    O = oracle
    base = _rows("lattice", N, dim)
    picks, wcen, wassign = _built("lattice", N, dim, "dot", NLIST, 2)
    passes = [_built("lattice", N, dim, "dot", NLIST, it)[2] for it in (0, 1)]     # what the two mean updates came from
    empty = np.setdiff1d(np.arange(NLIST), wassign)
    never_used = np.setdiff1d(empty, np.concatenate(passes))
    assert len(empty) >= 9, "the case should have empty lists"
    assert len(never_used) > 0 or dim in (300, 1536), "at dims 24 and 3072 some lists are empty from the start"
    what = "lattice dot dim=%d" % dim
    Q = np.random.RandomState(dim).randn(5, dim).astype(np.float32)
    with eng.Index(base, "dot") as idx:
        idx.ivf_build(NLIST, 2, 42)
        cen, off, lids, assign = _lists_of(idx, N, NLIST)
        assert not np.isnan(cen).any(), what
        np.testing.assert_array_equal(assign, wassign, err_msg=what)
        np.testing.assert_array_equal(assign, O.ivf_build(base, NLIST, 2, O.DOT, 42)[1], err_msg=what + " (float64)")
        np.testing.assert_array_equal(np.flatnonzero(np.diff(off) == 0), empty)
        _same_bits(cen, wcen, what + ": centroids")
        _same_bits(cen[never_used], base[picks[never_used]], what + ": a list that never had a member keeps its seeding row")
        _same_bits(cen, _centroids_by_the_rule(base, picks, passes), what + ": an emptied list keeps its last mean")
        ids, d, probes = idx.ivf_search(Q, 10, 4, want_probes=True)                # 20 pairs over 24 lists: the GEMV order
        oi, od, opr = O.ivf_search(base, cen, off, lids, Q, 10, 4, metric=O.DOT, mode=O.MODE_DEV)
        np.testing.assert_array_equal(probes, opr, err_msg=what)
        assert_exact(ids, d, oi, od, what + ": search over lists with empty ones")
        # ... and one that probes every list, the empty ones included
        ids, d = idx.ivf_search(Q[:2], 10, NLIST)
        oi, od, _ = O.ivf_search(base, cen, off, lids, Q[:2], 10, NLIST, metric=O.DOT, mode=O.MODE_DEV)
        assert_exact(ids, d, oi, od, what + ": full probe")


# ---- leg D: list sums and means ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["gaussian", "cancellation"])
@pytest.mark.parametrize("dim", [1, 5, 255, 256, 257, 1000, 3072])
def test_list_sums_and_means_are_sequential_f64_in_list_order(eng, dim, family):
    """Leg D.  A thread owns columns t, t + 256, ...; the device rows have stride ld, the outputs stride dim.  Lists: empty
    first / middle / last, one row, most of the rows, descending and shuffled ids."""
    n = 600
    off, lids = ki.crafted_lists(n)
    if family == "gaussian":
        base = np.random.RandomState(dim).randn(n, dim).astype(np.float32)
    else:
        base = ki.cancellation(n, dim, off, lids)
    wsum = ki.sequential_sums(base, off, lids)
    wmean = ki.sequential_means(base, off, lids)
    what = "%s dim=%d" % (family, dim)
    with eng.Index(base, "l2") as idx:
        sums = idx.list_sums(off, lids)
        means = idx.list_means(off, lids)
    empty = np.flatnonzero(np.diff(off) == 0)
    assert len(empty) == 4
    assert not np.isnan(means).any() and not np.isnan(sums).any(), what
    _same_bits(sums[empty], np.zeros((4, dim), np.float64), what + ": sums of the empty lists")
    _same_bits(means[empty], np.zeros((4, dim), np.float32), what + ": means of the empty lists")
    _same_bits(sums, wsum, what + ": sums")
    _same_bits(means, wmean, what + ": means")


# ---- legs E / F: the lightning mirror ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lightning_index(eng):
    from hnsw_clj_amd import datagen, lightning

    vecs = datagen.generate_dataset(600, 40).astype(np.float32)
    li = lightning.build_index(datagen.indexed(vecs), num_partitions=24, show_progress=False, seed=1)
    yield li, vecs
    li.close()


def _lightning_queries(vecs):
    return [vecs[9], vecs[401], np.random.RandomState(8).randn(40).astype(np.float32)]


def _as_arrays(li, result, k):
    ids = np.full((1, k), -1, np.int32)
    d = np.full((1, k), np.inf, np.float32)
    for j, (name, x) in enumerate(result):
        ids[0, j], d[0, j] = li.ids.index(name), x
    return ids, d


@pytest.mark.parametrize("percent", [0.1, 0.5, 1.0])
def test_lightning_centroid_routing_against_oracle(lightning_index, oracle, percent):
    """Leg E.  search_lightning with centroid routing is an IVF search over the index's own lists and means."""
    from hnsw_clj_amd import lightning

    O = oracle
    li, vecs = lightning_index
    cen, off, lids = li.index.get_ivf()
    nprobe, k = max(1, int(24 * percent)), 10
    for qi, q in enumerate(_lightning_queries(vecs)):
        what = "lightning percent=%g query %d" % (percent, qi)
        ids, d = _as_arrays(li, lightning.search_lightning(li, q, k, search_percent=percent, use_centroids=True), k)
        oi, od, _ = O.ivf_search(vecs, cen, off, lids, q, k, nprobe, mode=O.MODE_DEV)   # nprobe pairs over 24 lists: GEMV order
        assert_exact(ids, d, oi, od, what)
        fi, fd, _ = O.ivf_search(vecs, cen, off, lids, q, k, nprobe)
        assert_topk_parity(ids, d, fi, fd, what + " (float64)")


@pytest.mark.parametrize("how", ["turbo", "percent 0.1"])
def test_lightning_random_probes_against_oracle(lightning_index, oracle, how):
    """Leg E.  Below 15 % (and in the turbo / fast modes) the partitions are drawn with random.sample: the same draw,
    replayed, and the stable top-k over exactly those lists in probe order."""
    from hnsw_clj_amd import lightning

    O = oracle
    li, vecs = lightning_index
    _, off, lids = li.index.get_ivf()
    k = 10
    for qi, q in enumerate(_lightning_queries(vecs)):
        random.seed(100 + qi)
        if how == "turbo":
            got, nsearch = lightning.search_knn(li, q, k, "turbo"), max(1, int(24 * 0.08))
        else:
            got, nsearch = lightning.search_lightning(li, q, k, search_percent=0.1, use_centroids=False), 2
        random.seed(100 + qi)
        probes = random.sample(range(24), nsearch)
        rows = np.concatenate([lids[off[l]:off[l + 1]] for l in probes]).astype(np.int64)
        assert len(rows) == 25 * nsearch
        oi, od, _ = O.exact_knn(vecs, q, 600, metric=O.COSINE, mode=O.MODE_DEV)
        dense = np.empty(600, np.float32)
        dense[oi[0]] = od[0].astype(np.float32)
        order = rows[np.argsort(dense[rows], kind="stable")][:k]
        ids, d = _as_arrays(li, got, k)
        assert_exact(ids, d, order[None, :].astype(np.int32), dense[order][None, :], "lightning %s query %d" % (how, qi))


def test_lightning_smart_partition(eng, oracle):
    """Leg F.  smart_partition: the lists are the k-means++ seeding plus ONE assignment, the centroids the list means."""
    from hnsw_clj_amd import datagen, lightning

    O = oracle
    vecs = datagen.generate_dataset(600, 40).astype(np.float32)
    li = lightning.build_index(datagen.indexed(vecs), num_partitions=24, show_progress=False, smart_partition=True)
    try:
        cen, off, lids = li.index.get_ivf()
        _, _, wassign = O.ivf_build_dev(vecs, 24, 0, O.COSINE, 42)
        woff, wlids = O.lists_from_assign(wassign, 24)
        np.testing.assert_array_equal(off, woff)
        np.testing.assert_array_equal(lids, wlids)
        _same_bits(cen, ki.sequential_means(vecs, off, lids), "smart partition: centroids")
        assert li.num_partitions == 24
    finally:
        li.close()
