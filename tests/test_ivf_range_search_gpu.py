"""hnswgpu_ivf_range_search on the GPU: the rows of each query's probed lists within a radius, in candidate-stream order,
against float64 distances in numpy.

Seven lists of 0, 1, 31, 32, 33, 290 and 162 rows (empty; one row; one short of a hit word, a full word, one past it; a list that
crosses a 256-row tile and ends in a partial word) over a fixed permutation of the row ids, so list order is not id order.  The
rows of a list lie around the list's own centre, so the centroids (the lists' means) are well separated.  Radii as in
test_range_search_gpu.py: midpoints of float64 gaps that exceed 100 x the error of hnswgpu_batch_distances (the EXISTING entry
point's, measured here), so the expected segment of a query is exactly the rows of its stream with d64 <= radius."""
import functools

import numpy as np
import pytest
from test_range_search_gpu import N, NQ, _d64, _radii

pytestmark = pytest.mark.gpu

LENS = (0, 1, 31, 32, 33, 290, 162)
NLIST, OFF = len(LENS), np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
LIST_IDS = np.random.default_rng(11).permutation(N).astype(np.int32)
EVERY = np.tile(np.arange(NLIST, dtype=np.int32), (NQ, 1))


def _crafted():
    """[35][4]: list 5 in every row that probes at all (34 queries: two or more query blocks for one list -- the row of all -1
    cannot probe it), the empty list 0, -1 in the first, a middle and the last column, a row of all -1, a list twice in a row,
    and list 1 probed by query 7 alone."""
    q = np.arange(NQ)
    T = np.stack([np.full(NQ, 5), 2 + q % 5, np.where(q % 3 == 0, 0, 3), 6 - 2 * (q % 2)], 1).astype(np.int32)
    T[1], T[2], T[3], T[4], T[6] = [-1, 5, 3, 4], [5, -1, 2, 6], [5, 4, 2, -1], [-1] * 4, [5, 3, 3, 2]
    T[7, 1] = 1
    return T


@functools.lru_cache(maxsize=None)
def _case(metric, dim):
    rng = np.random.default_rng(1000 + dim)
    centre = rng.standard_normal((NLIST, dim))
    base = np.empty((N, dim), np.float32)
    for l in range(NLIST):
        rows = LIST_IDS[OFF[l]:OFF[l + 1]]
        base[rows] = centre[l] + rng.standard_normal((len(rows), dim))
    cent = np.stack([base[LIST_IDS[OFF[l]:OFF[l + 1]]].mean(0) if LENS[l] else -8.0 * centre[1:].mean(0) for l in range(NLIST)])
    cent = cent.astype(np.float32)
    # the 35 of 280 candidate queries whose float64 centroid ranking has the widest gap at rank 3, under every metric
    cand = (centre[rng.integers(1, NLIST, 8 * NQ)] + 2.0 * rng.standard_normal((8 * NQ, dim))).astype(np.float32)
    ranked = [np.sort(_d64(m, cand, cent), 1) for m in ("cosine", "l2", "dot")]
    score = np.min([(s[:, 3] - s[:, 2]) / np.abs(s).max(1) for s in ranked], 0)
    Q = cand[np.sort(np.argsort(-score, kind="stable")[:NQ])]
    d64 = _d64(metric, Q, base)
    rad, rad64, gap = _radii(d64)
    return base, cent, Q, d64, rad, rad64, gap


def _expected(d64, rad64, table):
    return [np.array([r for j in table[q] if j >= 0 for r in LIST_IDS[OFF[j]:OFF[j + 1]] if d64[q, r] <= rad64[q]], np.int64)
            for q in range(NQ)]


def _open(engine, metric, dim):
    base, cent, Q, d64, rad, rad64, gap = _case(metric, dim)
    idx = engine.Index(base, metric, 0)
    idx.set_ivf(cent, OFF, LIST_IDS)
    bd = np.stack([idx.batch_distances(Q[q]) for q in range(NQ)])         # the existing entry point: the bits to match
    err = np.abs(bd.astype(np.float64) - d64).max(1)
    print("%s dim %d: smallest gap / error = %.1f" % (metric, dim, (gap / err).min()))
    assert (gap > 100 * err).all() and (np.abs(rad.astype(np.float64) - rad64) < gap / 4).all()
    return idx, Q, rad, bd


def _check(res, want, bd, by_id=False):
    lims, ids, d = res[:3]
    assert lims[0] == 0 and np.array_equal(np.diff(lims), [len(w) for w in want])
    for q in range(NQ):
        got, w = ids[lims[q]:lims[q + 1]], want[q]
        o = np.argsort(got, kind="stable") if by_id else slice(None)
        assert np.array_equal(got[o], np.sort(w) if by_id else w), q
        assert np.array_equal(d[lims[q]:lims[q + 1]][o].view(np.uint32), bd[q, got[o]].view(np.uint32)), q


@pytest.mark.parametrize("dim", [20, 260, 768, 1100, 2100])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_given_probes_stream_order_and_distance_order(native_lib, metric, dim):
    from hnsw_clj_amd import engine

    d64, rad64, T = _case(metric, dim)[3], _case(metric, dim)[5], _crafted()
    idx, Q, rad, bd = _open(engine, metric, dim)
    with idx:
        want = _expected(d64, rad64, T)
        assert sum(len(w) for w in want) > N
        res = idx.ivf_range_search(Q, rad, 4, probes=T, want_probes=True)
        _check(res, want, bd)                                             # stream order
        assert np.array_equal(res[3], T)
        lims, ids, d = idx.ivf_range_search(Q, rad, 4, probes=T, by_distance=True)
        assert np.array_equal(lims, res[0])
        for q in range(NQ):
            w = want[q][np.lexsort((want[q], bd[q, want[q]]))]            # a duplicated list: equal keys, adjacent
            assert np.array_equal(ids[lims[q]:lims[q + 1]], w), q
            assert np.array_equal(d[lims[q]:lims[q + 1]].view(np.uint32), bd[q, w].view(np.uint32)), q


@pytest.mark.parametrize("dim", [20, 260, 768, 1100, 2100])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_every_list_probed_is_the_exact_range_search(native_lib, metric, dim):
    from hnsw_clj_amd import engine

    idx, Q, rad, bd = _open(engine, metric, dim)
    with idx:
        lims, ids, d = idx.ivf_range_search(Q, rad, NLIST, probes=EVERY)
        el, ei, ed = idx.range_search(Q, rad)
        assert np.array_equal(lims, el)
        for q in range(NQ):
            o = lims[q] + np.argsort(ids[lims[q]:lims[q + 1]], kind="stable")
            assert np.array_equal(ids[o], ei[el[q]:el[q + 1]]), q
            assert np.array_equal(d[o].view(np.uint32), ed[el[q]:el[q + 1]].view(np.uint32)), q


@pytest.mark.parametrize("dim", [20, 260, 768, 1100, 2100])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_routed_probes(native_lib, metric, dim):
    from hnsw_clj_amd import engine

    base, cent, _, d64, _, rad64, _ = _case(metric, dim)
    idx, Q, rad, bd = _open(engine, metric, dim)
    with idx, engine.Index(cent, metric, 0) as cidx:
        c64 = _d64(metric, Q, cent)
        cerr = np.abs(np.stack([cidx.batch_distances(Q[q]) for q in range(NQ)]).astype(np.float64) - c64).max(1)
        s = np.sort(c64, 1)
        assert (s[:, 3] - s[:, 2] > 100 * cerr).all()                     # the ranking has a gap at rank 3: f32 cannot move it
        res = idx.ivf_range_search(Q, rad, 3, want_probes=True)
        assert np.array_equal(res[3], idx.ivf_search(Q, 1, 3, want_probes=True)[2])
        assert np.array_equal(np.sort(res[3], 1), np.sort(np.argsort(c64, 1, kind="stable")[:, :3], 1))
        _check(res, _expected(d64, rad64, res[3]), bd)
        res = idx.ivf_range_search(Q, rad, 100, want_probes=True)         # clamps to the 7 lists
        assert (res[3][:, NLIST:] == -1).all() and np.array_equal(np.sort(res[3][:, :NLIST], 1), EVERY)
        _check(res, _expected(d64, rad64, EVERY), bd, by_id=True)


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_slices_cap_device_entry_and_refusals(native_lib, tune, metric):
    import torch

    from hnsw_clj_amd import engine

    T = _crafted()
    idx, Q, rad, bd = _open(engine, metric, 260)
    with idx:
        ref = idx.ivf_range_search(Q, rad, 4, probes=T)
        ref_d = idx.ivf_range_search(Q, rad, 4, probes=T, by_distance=True)
        total = int(ref[0][-1])
        p = engine._p
        fn = native_lib.lib().hnswgpu_ivf_range_search
        lims_c = np.full(NQ + 1, -1, np.int64)                            # count only
        assert fn(idx._h, p(Q), NQ, p(rad), 4, p(T), 0, p(lims_c), None, None, 0, None) == 0
        assert np.array_equal(lims_c, ref[0])
        lims_c[:] = -1                                                    # cap = total - 1
        small_i, small_d = np.empty(total - 1, np.int32), np.empty(total - 1, np.float32)
        assert fn(idx._h, p(Q), NQ, p(rad), 4, p(T), 0, p(lims_c), p(small_i), p(small_d), total - 1, None) == -5
        assert np.array_equal(lims_c, ref[0])
        dq, dr, dt = torch.from_numpy(Q).cuda(), torch.from_numpy(rad).cuda(), torch.from_numpy(T).cuda()
        with torch.cuda.stream(torch.cuda.Stream()):
            dev = idx.ivf_range_search_dev(dq, dr, 4, total, probes=dt, want_probes=True)
            cnt = idx.ivf_range_search_dev(dq, dr, 4, 0, probes=dt)
        torch.cuda.synchronize()
        assert np.array_equal(dev[0].cpu().numpy(), ref[0]) and np.array_equal(dev[1].cpu().numpy(), ref[1])
        assert np.array_equal(dev[2].cpu().numpy().view(np.uint32), ref[2].view(np.uint32)) and np.array_equal(dev[3].cpu().numpy(), T)
        assert np.array_equal(cnt[0].cpu().numpy(), ref[0]) and cnt[1] is None and cnt[2] is None
        for kw, code in (({"nprobe": 0}, -1), ({"nprobe": 4, "probes": np.where(T == 6, 7, T)}, -1)):
            with pytest.raises(native_lib.HnswGpuError) as e:
                idx.ivf_range_search(Q, rad, **kw)
            assert e.value.code == code
        tune.set("FILTER_EACH_MB", 0)                                     # one query group per slice: 35 queries, 2 slices
        for by, r in ((False, ref), (True, ref_d)):
            got = idx.ivf_range_search(Q, rad, 4, probes=T, by_distance=by)
            assert all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else np.array_equal(g, w)
                       for g, w in zip(got, r))
    with engine.Index(_case(metric, 260)[0], metric, 0) as bare, pytest.raises(native_lib.HnswGpuError) as e:
        bare.ivf_range_search(Q, rad, 4)
    assert e.value.code == -3
