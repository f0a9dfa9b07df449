"""hnswgpu_range_search_filtered[_each] on the GPU: the rows an allow-mask lets pass within a radius, against float64 distances.

Shapes, data and radii are test_range_search_gpu's: the radii sit in the middle of float64 gaps that exceed 100 x the largest
|hnswgpu_batch_distances - float64| of their query (the EXISTING entry point's error, not the code under test's), so the expected
set is exactly {i : bit(i) and d64(q, i) <= radius[q]}."""
import ctypes as C
import functools

import numpy as np
import pytest
from test_range_search_gpu import ELIMIT, N, NQ, TIED, _d64, _data, _radii

pytestmark = pytest.mark.gpu

_bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
_same = lambda got, ref: all(np.array_equal(_bits(g), _bits(r)) for g, r in zip(got, ref))


def _mask(kind):
    """ones | zero | half (283 rows: a second tile of the pass list; the tied rows pass) | eighth (70 rows: two pass-list words
    and a partial one; no tied row passes) | tail (the last, partial mask word + row 0)."""
    m = np.zeros(N, bool)
    if kind == "ones":
        m[:] = True
    elif kind == "tail":
        m[512:] = m[0] = True
    elif kind != "zero":
        m = np.random.default_rng({"half": 1, "eighth": 2}[kind]).random(N) < {"half": 0.5, "eighth": 0.125}[kind]
        m[list(TIED)] = m[TIED[0]]
    return m


@functools.lru_cache(maxsize=None)
def _ref(metric, dim):
    """Once per (metric, dim): data, f64 distances, the bits of batch_distances, the guarded radii, the unfiltered result."""
    from hnsw_clj_amd import engine

    base, Q = _data(dim)
    d64 = _d64(metric, Q, base)
    rad, rad64, gap = _radii(d64)
    with engine.Index(base, metric, 0) as idx:
        bd = np.stack([idx.batch_distances(Q[q]) for q in range(NQ)])
        plain = idx.range_search(Q, rad)
    err = np.abs(bd.astype(np.float64) - d64).max(1)
    print("%s dim %d: smallest gap / error = %.1f" % (metric, dim, (gap / err).min()))
    assert (gap > 100 * err).all() and (np.abs(rad.astype(np.float64) - rad64) < gap / 4).all()
    within = d64 <= rad64[:, None]
    assert all(within[q, list(TIED)].sum() in (0, 3) for q in range(NQ)) and within[:, TIED[0]].any()
    return base, Q, rad, within, bd, plain


@pytest.mark.parametrize("kind", ["ones", "zero", "half", "eighth", "tail"])
@pytest.mark.parametrize("dim", [20, 260, 768, 1100, 2100])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_single_mask_matches_float64_and_the_unfiltered_result(native_lib, metric, dim, kind):
    from hnsw_clj_amd import engine

    base, Q, rad, within, bd, (pl, pi, pd) = _ref(metric, dim)
    m = _mask(kind)
    assert {"half": m.sum() == 283 and m[TIED[0]], "eighth": m.sum() == 70}.get(kind, True)
    with engine.Index(base, metric, 0) as idx:
        lims, ids, d = idx.range_search_filtered(Q, rad, engine.pack_mask(m, N))
        lims2, ids2, d2 = idx.range_search_filtered(Q, rad, engine.pack_mask(m, N), by_distance=True)
    want = [np.flatnonzero(m & within[q]) for q in range(NQ)]
    assert lims[0] == 0 and np.array_equal(np.diff(lims), [len(w) for w in want]) and np.array_equal(lims2, lims)
    for q in range(NQ):
        a, b = lims[q], lims[q + 1]
        assert np.array_equal(ids[a:b], want[q]), q                       # the expected set, ascending
        assert np.array_equal(_bits(d[a:b]), _bits(bd[q, want[q]])), q
        ui, ud = pi[pl[q]:pl[q + 1]], pd[pl[q]:pl[q + 1]]                 # the unfiltered result with the failing rows dropped
        assert np.array_equal(ids[a:b], ui[m[ui]]) and np.array_equal(_bits(d[a:b]), _bits(ud[m[ui]])), q
        o = np.lexsort((ids[a:b], d[a:b]))
        assert np.array_equal(ids2[a:b], ids[a:b][o]) and np.array_equal(_bits(d2[a:b]), _bits(d[a:b][o])), q
        if set(TIED) <= set(want[q]):
            at = int(np.flatnonzero(ids2[a:b] == TIED[0])[0])
            assert tuple(ids2[a:b][at:at + 3]) == TIED, q                 # adjacent, ascending id
    if kind == "ones":
        assert _same((lims, ids, d), (pl, pi, pd))                        # hnswgpu_range_search, bit for bit


def _masks_each():
    """One mask per query; the first group (8 queries at dim 2100) holds an all-zero and an all-ones mask, two equal masks and
    two disjoint ones."""
    rng = np.random.default_rng(11)
    M = rng.random((NQ, N)) < rng.choice([0.02, 0.125, 0.5, 0.9], NQ)[:, None]
    M[0], M[1], M[3], M[5] = False, True, M[2], ~M[4]
    return M


@pytest.mark.parametrize("dim", [20, 768, 2100])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_each_mask_row_equals_the_single_mask_call(native_lib, metric, dim):
    from hnsw_clj_amd import engine

    base, Q, rad, within, _, _ = _ref(metric, dim)
    M = _masks_each()
    packed = engine.pack_masks(M, N)
    with engine.Index(base, metric, 0) as idx:
        for by in (False, True):
            lims, ids, d = idx.range_search_filtered_each(Q, rad, packed, by_distance=by)
            assert lims[0] == 0 and np.array_equal(np.diff(lims), (M & within).sum(1))
            for q in range(NQ):
                a, b = lims[q], lims[q + 1]
                l1, i1, d1 = idx.range_search_filtered(Q[q:q + 1], rad[q], packed[q], by_distance=by)
                assert l1[1] == b - a and np.array_equal(ids[a:b], i1) and np.array_equal(_bits(d[a:b]), _bits(d1)), (q, by)
                assert M[q, ids[a:b]].all(), q                            # never a row whose bit is clear for q


def test_edges_cap_slices_and_degenerate_calls(native_lib, tune):
    import torch

    from hnsw_clj_amd import engine

    base, Q, rad, within, _, _ = _ref("cosine", 260)
    rad = rad.copy()
    rad[3] = np.nan
    M = _masks_each()
    M[3] = True
    L = native_lib.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dq, dr = torch.from_numpy(Q).cuda(), torch.from_numpy(rad).cuda()
    with engine.Index(base, "cosine", 0) as idx:
        forms = ((L.hnswgpu_range_search_filtered, idx.range_search_filtered, idx.range_search_filtered_dev, engine.pack_mask(_mask("half"), N)),
                 (L.hnswgpu_range_search_filtered_each, idx.range_search_filtered_each, idx.range_search_filtered_each_dev, engine.pack_masks(M, N)))
        for fn, host, dev, mask in forms:
            lims, ids, d = ref = host(Q, rad, mask)
            ref_d = host(Q, rad, mask, by_distance=True)
            total = int(lims[-1])
            assert lims[4] == lims[3] and total > N                       # NaN: no hits, whatever the mask
            lims_c = np.full(NQ + 1, -1, np.int64)                        # count only
            assert fn(idx._h, p(Q), NQ, p(rad), 0, p(mask), p(lims_c), None, None, 0) == 0 and np.array_equal(lims_c, lims)
            lims_c[:] = -1                                                # cap = total - 1
            small_i, small_d = np.empty(total - 1, np.int32), np.empty(total - 1, np.float32)
            assert fn(idx._h, p(Q), NQ, p(rad), 0, p(mask), p(lims_c), p(small_i), p(small_d), total - 1) == ELIMIT
            assert np.array_equal(lims_c, lims)
            out = (torch.full((NQ + 1,), -1, dtype=torch.int64, device="cuda"), torch.full((total + 8,), -7, dtype=torch.int32, device="cuda"),
                   torch.full((total + 8,), -7.0, dtype=torch.float32, device="cuda"))
            dev(dq, dr, torch.from_numpy(mask.view(np.int32)).cuda(), total - 1, out=out)   # returns 0 (check() raises otherwise)
            torch.cuda.synchronize()
            got = [t.cpu().numpy() for t in out]
            assert _same((got[0], got[1][:total - 1], got[2][:total - 1]), (lims, ids[:total - 1], d[:total - 1]))
            assert (got[1][total - 1:] == -7).all() and (got[2][total - 1:] == -7.0).all()
            tune.set("FILTER_EACH_MB", 0)                                 # one query group per slice: 35 queries, 2 slices
            assert _same(host(Q, rad, mask), ref) and _same(host(Q, rad, mask, by_distance=True), ref_d)
            tune.unset("FILTER_EACH_MB")
            assert fn(idx._h, p(Q), NQ, p(rad), 0, None, p(lims_c), None, None, 0) == -1          # a null mask
            assert fn(idx._h, None, 0, None, 0, p(mask), None, None, None, 0) == 0                 # no queries
    with engine.Index(np.zeros((0, 16), np.float32), "l2", 0) as empty:
        for got in (empty.range_search_filtered(np.ones((3, 16), np.float32), 1.0, np.zeros(0, np.uint32)),
                    empty.range_search_filtered_each(np.ones((3, 16), np.float32), 1.0, np.zeros((3, 0), np.uint32))):
            assert np.array_equal(got[0], np.zeros(4, np.int64)) and len(got[1]) == 0 and len(got[2]) == 0
