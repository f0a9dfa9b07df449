"""The premises of tests/test_ivf_build_gpu.py, pinned with the CPU oracle alone (tests/kmeans_inputs.py has the
constructions): lattice rows make the float64 reference the oracle of the device's float32 build; duplicated rows make
every later pick depend on the last bit of every minimum; the cancellation family tells three orders of addition apart."""
import numpy as np
import pytest

import kmeans_inputs as ki

# (n, dim, nlist): every lattice shape the GPU file uses
LATTICE_SHAPES = [(1100, 24, 24), (1100, 300, 24), (1100, 1536, 24), (1100, 3072, 24), (9001, 8, 40)]


@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("n,dim,nlist", LATTICE_SHAPES)
def test_lattice_rows_make_the_f64_reference_the_oracle(oracle, n, dim, nlist, metric):
    O = oracle
    m = O.METRICS[metric]
    base = ki.lattice(n, dim)
    assert np.array_equal(base, np.round(base)) and np.abs(base).max() <= ki.LATTICE_AMP[dim] + 1
    want = O.kmeanspp(base, nlist, m, 42)
    for iters in ((0,) if n > 2000 else (0, 2)):
        picks, cen, assign = O.ivf_build_dev(base, nlist, iters, m, 42)
        assert not ki.first_difference(picks, want), ki.first_difference(picks, want)
        fcen, fassign = O.ivf_build(base, nlist, iters, m, 42)
        np.testing.assert_array_equal(assign, fassign)                              # hence the same lists
        np.testing.assert_array_equal(O.lists_from_assign(assign, nlist)[1], O.lists_from_assign(fassign, nlist)[1])
        np.testing.assert_allclose(cen, fcen, rtol=1e-6, atol=0)
        if m != O.L2 and iters == 2:                                                # the GEMV-order assignment as well
            p2, c2, a2 = O.ivf_build_dev(base, nlist, iters, m, 42, assign_mode=O.MODE_DEV)
            np.testing.assert_array_equal(a2, fassign)
            np.testing.assert_array_equal(c2.view(np.uint32), cen.view(np.uint32))


@pytest.mark.parametrize("dim", [300, 1536, 3072])
def test_duplicates_under_cosine_amplify_the_last_bit(oracle, dim):
    O = oracle
    base = ki.duplicates(dim)
    assert len(base) == 420 and len(np.unique(base, axis=0)) == 7
    picks = O.ivf_build_dev(base, 20, 0, O.COSINE, 42)[0]
    f64 = O.kmeanspp(base, 20, O.COSINE, 42)
    distinct = [tuple(base[i][:4]) for i in picks[:7]]
    assert len(set(distinct)) == 7, "a duplicate of a chosen row was picked before all 7 distinct rows were"
    assert np.array_equal(picks[:7], f64[:7])
    assert not np.array_equal(picks[7:], f64[7:]), "the picks drawn from the rounding residue should differ from float64's"
    # what they are drawn from: minima of ~1e-8, not zeros
    minima = ki.running_minima(ki.seeding_distances(O, base, O.COSINE, picks))
    assert 0 < np.abs(minima[8]).max() < 1e-6


def test_duplicates_under_l2_have_no_weight_left(oracle):
    O = oracle
    base = ki.duplicates(300)
    for picks in (O.ivf_build_dev(base, 20, 0, O.L2, 42)[0], O.kmeanspp(base, 20, O.L2, 42)):
        assert len(np.unique(base[picks[:7]], axis=0)) == 7
        assert (picks[7:] == 0).all()
    same = ki.all_equal(5000, 8)
    assert (O.ivf_build_dev(same, 6, 0, O.L2, 42)[0][1:] == 0).all()


@pytest.mark.parametrize("dim", [1, 5, 257])
def test_cancellation_family_tells_three_orders_apart(dim):
    n = 600
    off, lids = ki.crafted_lists(n)
    sizes = np.diff(off)
    assert sizes[0] == sizes[3] == sizes[-1] == 0 and sizes[1] == 1 and sizes[2] > n // 2
    assert (np.diff(lids[off[4]:off[5]]) < 0).all()                                # the descending list
    assert sorted(lids.tolist()) == list(range(n))
    base = ki.cancellation(n, dim, off, lids)
    a, b, c = ki.sequential_sums(base, off, lids), ki.index_order_sums(base, off, lids), ki.pairwise_sums(base, off, lids)
    for l in np.flatnonzero(sizes >= 8):
        assert (a[l] != b[l]).any() and (a[l] != c[l]).any() and (b[l] != c[l]).any(), "list %d" % l
        if dim >= 5:                                                                # ... in most columns, not in one
            assert np.mean((a[l] != b[l]) & (a[l] != c[l])) > 0.5
    assert (a[sizes == 0] == 0).all()
    np.testing.assert_array_equal(a[1], base[lids[off[1]]].astype(np.float64))
    # a float accumulator would not survive gaussian rows either
    g = np.random.RandomState(5).randn(n, dim).astype(np.float32)
    f32 = np.zeros((len(off) - 1, dim), np.float32)
    for l in range(len(off) - 1):
        for i in lids[off[l]:off[l + 1]]:
            f32[l] = f32[l] + g[i]
    means = ki.sequential_means(g, off, lids)
    big = np.flatnonzero(sizes >= 8)
    assert ((f32[big] / sizes[big, None].astype(np.float32)) != means[big]).any()


def test_seeding_replay_is_the_oracles_arithmetic(oracle):
    """seeding_distances takes its rows from one exact-kNN call: the same bits as oracle.distance_dev pair by pair, and the
    replayed minima reproduce the picks' own history (a centre's minimum is its self-distance from its round on)."""
    O = oracle
    base = ki.clustered(O, 300, 100)
    for m in (O.COSINE, O.L2, O.DOT):
        picks = O.ivf_build_dev(base, 12, 0, m, 42)[0]
        dist = ki.seeding_distances(O, base, m, picks)
        rs = np.random.RandomState(3)
        for r, i in zip(rs.randint(0, 11, 40), rs.randint(0, 300, 40)):
            assert np.float32(O.distance_dev(m, base[picks[r]], base[i])) == dist[r, i]
        # a bound equal to the distance itself skips exactly the rows the new centre does not improve
        share = ki.skip_share(dist, lambda r: dist[r])
        minima = ki.running_minima(dist)
        assert share == np.mean(dist[1:] >= minima[1:])
        assert ki.skip_share(dist, lambda r: np.full(300, np.nan, np.float32)) == 0.0
