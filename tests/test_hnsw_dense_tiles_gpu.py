"""The tile walk of hnsw_dense_bounds_kernel (dense_kernels.hpp): persistent workgroups, tiles of TQ = 128 queries x TR = 256
rows, two LDS images and one barrier per 128-byte K step, a tile's bounds stored between its last step and the next tile's first.

The table (hnswgpu_hnsw_dense_bounds) is held to hnswgpu_hnsw_rejection_bounds bit for bit at every edge of that walk: batches
and bases around one tile, a base one row past a whole super-panel and one whose row tiles do not divide by 8 super-panels, 2, 4,
6 and 8 K steps (dims 200, 300, 768, 1000: one to four turns of the two-step loop), a launch of exactly one tile, one of fewer
tiles than workgroups, and one in which a workgroup walks several tiles.  A search that reads the table (mode 2) is held to one
that computes its bounds (mode 0), as tests/test_hnsw_dense_bounds.py does, at TQ + 1 queries.

Data: finite gaussian rows and queries of mixed lengths, with the zero query, a query too small to be coded and the zero row among
them.  NaN and infinity are checked in the table only; they are never searched (HnswList::admit is not reproducible there)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from util import assert_exact  # noqa: E402

pytestmark = pytest.mark.gpu

TQ, TR, PANEL = 128, 256, 4      # kDenseTQ, kDenseTR, kDensePanel
METRICS = ("cosine", "dot", "l2")
NQS = (1, TQ - 1, TQ, TQ + 1, 2 * TQ + 1)
# 4097: 17 row tiles in super-panels of 2 -- one row past 8 whole super-panels; 8193: 33 row tiles in super-panels of 4 -- one row
# past 8 whole super-panels, and 33 does not divide by 8 x 4
NS = (1, TR - 1, TR, TR + 1, 4097, 8193)
DIMS = (200, 300, 768, 1000)     # 2, 4, 6, 8 K steps of 128 bytes
SENT_ID, SENT_D, SENT_ST = -7, -1.0, -3


def _tiling(nq, n):
    """dense_tiling and dense_walk_places: (query tiles, row tiles, row tiles per super-panel, super-panels, places, tiles)."""
    nqt, nrt = -(-nq // TQ), -(-n // TR)
    rp = max(1, min(PANEL, nrt // 8))
    nsp = -(-nrt // rp)
    return nqt, nrt, rp, nsp, 8 * (-(-nsp // 8)) * nqt * rp, nqt * nrt


def test_the_shapes_reach_the_edges_they_are_named_for():
    assert _tiling(1, 4097)[1:4] == (17, 2, 9) and 4097 == 8 * 2 * TR + 1
    assert _tiling(1, 8193)[1:4] == (33, 4, 9) and 8193 == 8 * 4 * TR + 1 and 33 % (8 * PANEL) != 0
    assert [-(-4 * 64 * ((d + 255) // 256) // 128) for d in DIMS] == [2, 4, 6, 8]


@pytest.fixture(scope="module")
def eng(native_lib):
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    return engine


@pytest.fixture(scope="module")
def workgroups():
    """The launch's persistent grid: one workgroup per CU, a multiple of 8."""
    import torch

    return max(8, torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8)


def _reference(idx, Q, n):
    ids = np.arange(n, dtype=np.int32)
    return np.stack([idx.hnsw_rejection_bounds(q, ids) for q in Q])


def _same_bits(tab, ref, tag):
    assert tab.shape == ref.shape, tag
    np.testing.assert_array_equal(np.isnan(tab), np.isnan(ref), err_msg=tag + ": NaNs in other places")
    ok = ~np.isnan(ref)
    np.testing.assert_array_equal(tab.view(np.uint32)[ok], ref.view(np.uint32)[ok], err_msg=tag + ": bound bits")


def _rows_and_queries(n, nq, dim, seed):
    """Gaussian rows and queries of lengths e^-2 .. e^2; the zero row, the zero query and a query below the coder's range in the
    places that exist."""
    rs = np.random.RandomState(seed)
    base = rs.randn(n, dim).astype(np.float32) * np.exp(rs.uniform(-2, 2, (n, 1))).astype(np.float32)
    Q = rs.randn(nq, dim).astype(np.float32) * np.exp(rs.uniform(-2, 2, (nq, 1))).astype(np.float32)
    if n > 5:
        base[5] = 0.0
    if nq > 6:
        Q[5] = 0.0
        Q[6] = (Q[6].astype(np.float64) * 1e-20).astype(np.float32)
    return base, Q


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", NS)
def test_table_at_every_tile_edge(eng, metric, dim, n):
    """The reference of all queries is computed once per index.  Every batch size takes queries of its own: the handle's table keeps
    what the call before wrote, in the same places, and a tile that a launch left out must not find its bounds there."""
    base, Q = _rows_and_queries(n, sum(NQS), dim, 7 * n + dim)
    with eng.Index(base, metric) as idx:
        idx.set_rejection_test(2)
        ref = _reference(idx, Q, n)
        at = 0
        for nq in NQS:
            _same_bits(idx.hnsw_dense_bounds(Q[at:at + nq]), ref[at:at + nq], "%s dim %d n %d nq %d" % (metric, dim, n, nq))
            at += nq


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", (200, 300, 768))
def test_one_tile_few_tiles_and_a_walk_of_several(eng, workgroups, metric, dim):
    """Exactly one tile; fewer tiles than workgroups, with empty places among them; more tiles than workgroups, so that a
    workgroup computes a tile's bounds with the next tile's operands in LDS -- at one turn of the two-step K loop (dim 200), where
    every turn is a tile's last, and at two and three turns (dims 300 and 768), where turns that are not come before it.  Each
    launch on a handle of its own: nothing is left in the table from a launch before."""
    n_many = 8193
    nq_many = TQ * (workgroups // _tiling(1, n_many)[1] + 1) + 1
    base, Q = _rows_and_queries(n_many, nq_many, dim, 4242 + dim)
    assert _tiling(TQ, TR)[4:] == (8, 1)
    nqt, nrt, rp, nsp, places, tiles = _tiling(2 * TQ + 1, 4097)
    assert tiles < workgroups and tiles < places
    nqt, nrt, rp, nsp, places, tiles = _tiling(nq_many, n_many)
    assert tiles > workgroups and places > workgroups, (tiles, places, workgroups)
    for n, nq in ((TR, TQ), (4097, 2 * TQ + 1), (n_many, nq_many)):
        with eng.Index(base[:n], metric) as idx:
            idx.set_rejection_test(2)
            _same_bits(idx.hnsw_dense_bounds(Q[:nq]), _reference(idx, Q[:nq], n), "%s dim %d n %d nq %d" % (metric, dim, n, nq))


@pytest.mark.parametrize("metric", METRICS)
def test_table_of_nan_and_infinity(eng, metric):
    """In the table only: a query holding NaN, one holding infinity and a row holding NaN abstain (NaN) where the traversal's own
    bounds do, in a batch and a base that end inside their last tiles."""
    base, Q = _rows_and_queries(TR + 1, TQ + 1, 300, 99)
    base[9, 17] = np.nan
    Q[3, 100] = np.nan
    Q[TQ, 0] = np.inf
    with eng.Index(base, metric) as idx:
        idx.set_rejection_test(2)
        tab = idx.hnsw_dense_bounds(Q)
        _same_bits(tab, _reference(idx, Q, len(base)), metric + " NaN and infinity")
        assert np.isnan(tab[[3, 6, TQ]]).all() and np.isnan(tab[:, 9]).all()


def _dev_search(idx, Q, k=10, ef=32):
    import torch

    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    ids = torch.full((len(Q), k), SENT_ID, dtype=torch.int32, device=dev)
    d = torch.full((len(Q), k), SENT_D, dtype=torch.float32, device=dev)
    st = torch.full((len(Q), 2), SENT_ST, dtype=torch.int64, device=dev)
    idx.hnsw_search_dev(Qd, k, ef, out=(ids, d), stats=st)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), d.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("metric", METRICS)
def test_search_with_the_table_equals_search_without(eng, tune, metric):
    """TQ + 1 queries on 2,000 rows (8 row tiles, the last one ragged), the wave kernel forced: ids, distance bits, both per-query
    counters and the handle's (f32 rows, neighbours) of mode 2 are mode 0's."""
    base, Q = _rows_and_queries(2000, TQ + 1, 128, 2000)
    tune.set("HNSW_WAVE", 2)
    tune.set("PREFETCH", 0)
    with eng.Index(base, metric) as idx:
        idx.set_rejection_test(2)
        idx.hnsw_build(8, 100, 42)
        idx.set_profiling(True)
        out, rej = {}, {}
        for mode in (0, 2):
            idx.set_hnsw_dense_bounds(mode)
            idx.rejection_stats(reset=True)
            w0, l0 = eng.debug_counter("hnsw_wave"), idx.hnsw_dense_bounds_state()[2]
            out[mode] = _dev_search(idx, Q)
            rej[mode] = idx.rejection_stats(reset=True)
            assert eng.debug_counter("hnsw_wave") > w0, "the wave kernel did not run (mode %d)" % mode
            assert (idx.hnsw_dense_bounds_state()[2] > l0) == (mode == 2), "launches with the table in mode %d" % mode
        idx.set_hnsw_dense_bounds(1)
        (i0, d0, s0), (i2, d2, s2) = out[0], out[2]
        np.testing.assert_array_equal(s2, s0, err_msg=metric + ": counters")
        assert_exact(i2, d2, i0, d0, metric)
        assert rej[2] == rej[0] and rej[0][1] > 0, "(f32 rows, neighbours) %s with the table, %s without" % (rej[2], rej[0])
        assert (i2 != SENT_ID).all() and (d2 != SENT_D).all() and (s2 != SENT_ST).all() and not np.isnan(d2).any()
