"""hnswgpu_range_search on the GPU: every row within a radius, CSR results, against float64 distances in numpy.

The radii sit in the middle of float64 gaps that exceed 100 x the largest |hnswgpu_batch_distances - float64| of their query (the
EXISTING entry point's error, not the code under test's): f32 rounding cannot move a row across a radius, so the expected set is
exactly {i : d64(q, i) <= radius[q]}."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NQ = 549, 35             # two full 256-row tiles + 37 rows (last hit word partial); a full query group + a partial one
TIED = (5, 300, 548)        # row 5 copied: exact ties inside a segment, one of them in the partial word
ELIMIT = -5


def _d64(metric, Q, base):
    Q, base = Q.astype(np.float64), base.astype(np.float64)
    dot = Q @ base.T
    if metric == "dot":
        return -dot
    if metric == "l2":
        return np.stack([np.sqrt(((q - base) ** 2).sum(1)) for q in Q])
    return 1.0 - dot / (np.linalg.norm(Q, axis=1)[:, None] * np.linalg.norm(base, axis=1)[None, :])


def _data(dim, seed=7):
    rng = np.random.default_rng(seed + dim)
    base = rng.standard_normal((N, dim)).astype(np.float32)
    base[TIED[1]] = base[TIED[2]] = base[TIED[0]]
    return base, rng.standard_normal((NQ, dim)).astype(np.float32)


def _radii(d64):
    """Per query: the radius for its target count, at the midpoint of the largest gap within +-3 of the target; and that gap."""
    targets = [0, 1, 7, 33, 300, N - 1, N]
    rad, gap = np.empty(NQ), np.empty(NQ)
    for q in range(NQ):
        s, t = np.sort(d64[q]), targets[q % len(targets)]
        if t == 0:
            rad[q], gap[q] = s[0] - 1.0, np.inf
        elif t == N:
            rad[q], gap[q] = s[-1] + 1.0, np.inf
        else:
            cs = np.arange(max(1, t - 3), min(N - 1, t + 3) + 1)          # counts: s[c - 1] <= radius < s[c]
            c = cs[np.argmax(s[cs] - s[cs - 1])]
            rad[q], gap[q] = 0.5 * (s[c - 1] + s[c]), s[c] - s[c - 1]
    return rad.astype(np.float32), rad, gap


@pytest.mark.parametrize("dim", [20, 260, 768, 1100, 2100])
@pytest.mark.parametrize("metric", ["cosine", "l2", "dot"])
def test_range_search_matches_float64(native_lib, metric, dim):
    from hnsw_clj_amd import engine

    base, Q = _data(dim)
    d64 = _d64(metric, Q, base)
    with engine.Index(base, metric, 0) as idx:
        bd = np.stack([idx.batch_distances(Q[q]) for q in range(NQ)])     # the existing entry point: the bits to match
        rad, rad64, gap = _radii(d64)
        err = np.abs(bd.astype(np.float64) - d64).max(1)
        print("%s dim %d: smallest gap / error = %.1f" % (metric, dim, (gap / err).min()))
        assert (gap > 100 * err).all() and (np.abs(rad.astype(np.float64) - rad64) < gap / 4).all()
        want = [np.flatnonzero(d64[q] <= rad64[q]) for q in range(NQ)]
        assert all(len(set(TIED) & set(w)) in (0, 3) for w in want)      # the window never splits the tied copies
        assert any(TIED[0] in w for w in want)
        lims, ids, d = idx.range_search(Q, rad)
        assert lims[0] == 0 and (np.diff(lims) >= 0).all()
        assert np.array_equal(np.diff(lims), [len(w) for w in want])
        for q in range(NQ):
            a, b = lims[q], lims[q + 1]
            assert np.array_equal(ids[a:b], want[q]), q                   # the expected set, ascending
            assert np.array_equal(d[a:b].view(np.uint32), bd[q, want[q]].view(np.uint32)), q
            assert (d[a:b] <= rad[q]).all()
        lims2, ids2, d2 = idx.range_search(Q, rad, by_distance=True)
        assert np.array_equal(lims2, lims)
        for q in range(NQ):
            a, b = lims[q], lims[q + 1]
            o = np.lexsort((ids[a:b], d[a:b]))
            assert np.array_equal(ids2[a:b], ids[a:b][o]), q
            assert np.array_equal(d2[a:b].view(np.uint32), d[a:b][o].view(np.uint32)), q
            if TIED[0] in want[q]:
                at = int(np.flatnonzero(ids2[a:b] == TIED[0])[0])
                assert tuple(ids2[a:b][at:at + 3]) == TIED, q             # adjacent, ascending id


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_range_search_edges_cap_and_slices(native_lib, tune, metric):
    import torch

    from hnsw_clj_amd import engine

    dim = 260
    base, Q = _data(dim)
    L = native_lib.lib()
    with engine.Index(base, metric, 0) as idx:
        assert not idx.range_search(Q, -np.inf)[0].any()
        assert np.array_equal(idx.range_search(Q, np.inf)[0], np.arange(NQ + 1) * N)
        rad = _radii(_d64(metric, Q, base))[0]
        rad[3] = np.nan
        lims, ids, d = idx.range_search(Q, rad)
        total = int(lims[-1])
        assert lims[4] == lims[3] and total > N                           # NaN: no hits
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        lims_c = np.full(NQ + 1, -1, np.int64)                            # count only
        assert L.hnswgpu_range_search(idx._h, p(Q), NQ, p(rad), 0, p(lims_c), None, None, 0) == 0
        assert np.array_equal(lims_c, lims)
        lims_c[:] = -1                                                    # cap = total - 1
        small_i, small_d = np.empty(total - 1, np.int32), np.empty(total - 1, np.float32)
        assert L.hnswgpu_range_search(idx._h, p(Q), NQ, p(rad), 0, p(lims_c), p(small_i), p(small_d), total - 1) == ELIMIT
        assert np.array_equal(lims_c, lims)
        dq, dr = torch.from_numpy(Q).cuda(), torch.from_numpy(rad).cuda()
        out = (torch.full((NQ + 1,), -1, dtype=torch.int64, device="cuda"), torch.full((total + 8,), -7, dtype=torch.int32, device="cuda"),
               torch.full((total + 8,), -7.0, dtype=torch.float32, device="cuda"))
        idx.range_search_dev(dq, dr, total - 1, out=out)                  # returns 0 (check() raises otherwise)
        torch.cuda.synchronize()
        assert np.array_equal(out[0].cpu().numpy(), lims)
        assert np.array_equal(out[1].cpu().numpy()[:total - 1], ids[:total - 1])
        assert np.array_equal(out[2].cpu().numpy()[:total - 1].view(np.uint32), d[:total - 1].view(np.uint32))
        assert (out[1][total - 1:] == -7).all() and (out[2][total - 1:] == -7.0).all()
        lims_d, ids_d, d_d = idx.range_search(Q, rad, by_distance=True)
        tune.set("FILTER_EACH_MB", 0)                                     # one query group per slice: 35 queries, 2 slices
        for by, ref in ((False, (lims, ids, d)), (True, (lims_d, ids_d, d_d))):
            got = idx.range_search(Q, rad, by_distance=by)
            assert all(np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, r.view(np.uint32) if r.dtype == np.float32 else r)
                       for g, r in zip(got, ref))


@pytest.mark.parametrize("n", [4097, 9001])
def test_range_sort_of_segments_beyond_one_lds_tile(native_lib, n):
    """Segments of more than 4096 entries: the bitonic network's wide strides through global memory (4097: one key in the
    second tile; 9001: three tiles, two wide merges, a padded power of two)."""
    from hnsw_clj_amd import engine

    rng = np.random.default_rng(n)
    base = rng.standard_normal((n, 20)).astype(np.float32)
    base[n - 1] = base[4095] = base[17]                                   # ties across tiles
    Q = rng.standard_normal((2, 20)).astype(np.float32)
    with engine.Index(base, "l2", 0) as idx:
        lims, ids, d = idx.range_search(Q, [np.inf, 5.0], by_distance=True)
        for q in range(2):
            bd = idx.batch_distances(Q[q])
            keep = np.flatnonzero(bd <= (np.inf, np.float32(5.0))[q])
            o = keep[np.lexsort((keep, bd[keep]))]
            assert np.array_equal(ids[lims[q]:lims[q + 1]], o), q
            assert np.array_equal(d[lims[q]:lims[q + 1]].view(np.uint32), bd[o].view(np.uint32)), q
        assert lims[1] == n and lims[2] - lims[1] > 0


def test_range_search_empty_index_and_no_queries(native_lib):
    from hnsw_clj_amd import engine

    with engine.Index(np.zeros((0, 16), np.float32), "l2", 0) as empty:
        lims, ids, d = empty.range_search(np.ones((3, 16), np.float32), 1.0)
        assert np.array_equal(lims, np.zeros(4, np.int64)) and len(ids) == 0 and len(d) == 0
    with engine.Index(np.ones((4, 16), np.float32), "l2", 0) as idx:
        assert native_lib.lib().hnswgpu_range_search(idx._h, None, 0, None, 0, None, None, None, 0) == 0
        lims, ids, d = idx.range_search(np.ones((2, 16), np.float32), 0.5)
        assert np.array_equal(lims, [0, 4, 8]) and np.array_equal(ids, [0, 1, 2, 3] * 2) and not d.any()
