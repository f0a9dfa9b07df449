"""Crafted rows for the IVF construction kernels (k-means++ seeding, list means / sums, the Lloyd loop) and what they must
return: the role tests/topk_streams.py plays for the selection kernels.

Two constructions replace a tolerance:

  lattice     integer cluster centres in [-amp, amp]^dim, every row one centre with +-1 on ~15 % of its components.  While
              (2 amp + 2)^2 * dim stays far below 2^24 every dot product and squared L2 distance is an exact integer in
              float32 IN ANY SUMMATION ORDER, so the device-order restatement (oracle.ivf_build_dev) and the float64
              reference (oracle.kmeanspp / oracle.ivf_build) make the same picks and assignments: the device is compared
              with the reference arithmetic itself (tests/test_ivf_build_host.py pins that premise).
  duplicates  m distinct gaussian rows, each repeated, shuffled.  Under cosine, once all m are centres every running
              minimum is the float32 rounding residue of a self-distance (~1e-8) and the remaining picks are D^2 samples of
              that noise: ANY deviation in ANY minimum moves a pick.  Only the device-order oracle is the reference there.
              Under L2 a self-distance is exactly 0: the total weight is 0 after coverage and every further pick is row 0.

The list means / sums have their own family (`cancellation`): columns whose float64 sum depends on the order of addition,
and a plain restatement of the contract (sequential_sums: one float64 add at a time, in LIST order).
"""
import numpy as np

FLT_MAX = np.float32(3.402823466e+38)
# amp per dim: (2 amp + 2)^2 * dim is the largest squared L2 distance between two rows; all of them far below 2^24
LATTICE_AMP = {8: 6, 24: 6, 300: 2, 1536: 1, 3072: 1}
# The picks and the first assignment are exact for any draw.  After a Lloyd pass the centroids are means, stored in float32
# by the engine and in float64 by the reference: a row whose two best means are closer than that rounding may go either way
# (seen for 1 to 9 of 1100 rows under dot in about one draw in three).  The draws used are those without such a row;
# tests/test_ivf_build_host.py holds them to it.
LATTICE_SEED = {300: 1}


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- families --------------------------------------------------------------------------------------------------
def clustered(O, n, dim, seed=42, num_clusters=9, noise_level=0.5):
    """The oracle's generator (test/data_generator.clj), as the other build tests use it."""
    return _f32(O.generate_dataset(n, dim, "clustered", num_clusters=num_clusters, noise_level=noise_level, seed=seed))


def gaussian(O, n, dim, seed=42):
    """Independent gaussian rows: at dims of a few hundred all pairwise distances are nearly equal, so a seeding round
    improves most running minima by a small fraction -- the rows a bound that is a little too high would skip."""
    return _f32(O.generate_dataset(n, dim, "gaussian", seed=seed))


def lattice(n, dim, amp=None, seed=None, centres=9, share=0.15):
    amp = LATTICE_AMP[dim] if amp is None else amp
    seed = LATTICE_SEED.get(dim, 0) if seed is None else seed
    assert (2 * amp + 2) ** 2 * dim < 2 ** 24 // 64, "sums would not stay exact"
    rs = np.random.RandomState(1000 + seed + dim)
    c = rs.randint(-amp, amp + 1, size=(centres, dim))
    rows = c[rs.randint(0, centres, n)]
    step = rs.choice([-1, 1], size=(n, dim)) * (rs.rand(n, dim) < share)
    return _f32(rows + step)


def duplicates(dim, m=7, reps=60, seed=0):
    rs = np.random.RandomState(2000 + seed + dim)
    distinct = _f32(rs.randn(m, dim))
    return _f32(distinct[rs.permutation(np.repeat(np.arange(m), reps))])


def all_equal(n, dim, seed=0):
    rs = np.random.RandomState(3000 + seed + dim)
    return _f32(np.tile(_f32(rs.randn(1, dim)), (n, 1)))


BIG = np.float32(2.0 ** 60)


def cancellation(n, dim, off, lids, seed=0):
    """Rows for the lists (off, lids): in every list of >= 8 rows every column holds +2^60 at one member, -2^60 at a later
    one (positions in LIST order, drawn per column) and integers 1..50 elsewhere.  A float64 sum keeps only what the
    rounding at 2^60 (steps of 256) lets through, so it depends on where the two large terms fall in the order of
    addition."""
    rs = np.random.RandomState(4000 + seed + dim)
    base = rs.randint(1, 51, size=(n, dim)).astype(np.float32)
    cols = np.arange(dim)
    for l in range(len(off) - 1):
        members = np.asarray(lids[off[l]:off[l + 1]], np.int64)
        m = len(members)
        if m < 8:
            continue
        plus = rs.randint(0, m // 2, dim)                    # somewhere in the first half of the list ...
        minus = rs.randint(m // 2, m - 1, dim)               # ... and cancelled in the second, with rows left behind it
        base[members[plus], cols] = BIG
        base[members[minus], cols] = -BIG
    return _f32(base)


def crafted_lists(n, seed=0):
    """(off, lids) over rows 0..n-1, n >= 300: empty first / middle / last lists, a one-row list, one list holding most of
    the rows (shuffled), one in DESCENDING id order, two more shuffled ones."""
    rs = np.random.RandomState(5000 + seed + n)
    perm = rs.permutation(n).astype(np.int32)
    sizes = [0, 1, n - 1 - 60 - 47 - 90, 0, 60, 47, 0, 90, 0]
    assert sum(sizes) == n and sizes[2] > n // 2
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    lids = perm.copy()
    lids[off[4]:off[5]] = np.sort(perm[off[4]:off[5]])[::-1]
    return off, lids


# ---- the contract of hnswgpu_list_sums / hnswgpu_list_means, restated ------------------------------------------------------
def sequential_sums(base, off, lids):
    """float64 column sums of every list, ONE add at a time in list order (ivf_flat.clj:70-75); not np.sum, which adds
    pairwise."""
    base = np.asarray(base)
    out = np.zeros((len(off) - 1, base.shape[1]), np.float64)
    for l in range(len(off) - 1):
        for i in lids[off[l]:off[l + 1]]:
            out[l] = out[l] + base[i].astype(np.float64)
    return out


def sequential_means(base, off, lids):
    """float32(sum / count) of sequential_sums; an empty list gives the zero vector."""
    s = sequential_sums(base, off, lids)
    cnt = np.diff(off).astype(np.float64)
    out = np.zeros(s.shape, np.float32)
    for l in np.flatnonzero(cnt > 0):
        out[l] = (s[l] / cnt[l]).astype(np.float32)
    return out


def index_order_sums(base, off, lids):
    """The same with every list's members in ascending id order: NOT the contract."""
    lids = np.array(lids)
    for l in range(len(off) - 1):
        lids[off[l]:off[l + 1]] = np.sort(lids[off[l]:off[l + 1]])
    return sequential_sums(base, off, lids)


def _pairwise(rows):
    if len(rows) == 0:
        return 0.0
    if len(rows) == 1:
        return rows[0]
    h = len(rows) // 2
    return _pairwise(rows[:h]) + _pairwise(rows[h:])


def pairwise_sums(base, off, lids):
    """The same in list order but added as a balanced tree: NOT the contract."""
    base = np.asarray(base, np.float64)
    out = np.zeros((len(off) - 1, base.shape[1]), np.float64)
    for l in range(len(off) - 1):
        out[l] = _pairwise(base[np.asarray(lids[off[l]:off[l + 1]], np.int64)])
    return out


# ---- replay of a seeding ---------------------------------------------------------------------------------------------------
def seeding_distances(O, base, metric, picks):
    """dist[r][i]: the device-order distance (oracle.distance_dev's arithmetic, one call for all rows) of row i to the
    centre of round r + 1, base[picks[r]], for the nlist - 1 rounds of a seeding."""
    base = _f32(base)
    centres = base[np.asarray(picks[:-1], np.int64)]
    ids, d, _ = O.exact_knn(base, centres, len(base), metric=metric, mode=O.MODE_DEV)
    out = np.empty((len(centres), len(base)), np.float32)
    np.put_along_axis(out, ids.astype(np.int64), d.astype(np.float32), axis=1)
    return out


def running_minima(dist):
    """minima[r][i]: row i's running minimum BEFORE round r + 1 (FLT_MAX before the first)."""
    out = np.empty(dist.shape, np.float32)
    cur = np.full(dist.shape[1], FLT_MAX, np.float32)
    for r in range(len(dist)):
        out[r] = cur
        cur = np.minimum(cur, dist[r])
    return out


def skip_share(dist, bounds):
    """The share of (round >= 2, row) pairs a bounds pass may skip: bounds(r) -> the lower bounds of every row against the
    centre of round r + 1 (r counts from 0; NaN = no bound), compared with the replayed running minima."""
    minima = running_minima(dist)
    skipped = total = 0
    for r in range(1, len(dist)):
        lb = np.asarray(bounds(r), np.float32)
        with np.errstate(invalid="ignore"):
            skipped += int((lb >= minima[r]).sum())
        total += dist.shape[1]
    return skipped / max(total, 1)


def first_difference(got, want):
    """'' or a message naming the first differing pick: the round whose minima were stale."""
    got, want = np.asarray(got), np.asarray(want)
    bad = np.flatnonzero(got != want)
    if len(bad) == 0:
        return ""
    r = int(bad[0])
    return "pick %d differs: row %d, expected row %d (the minima after round %d are suspect)" % (r, got[r], want[r], r)
