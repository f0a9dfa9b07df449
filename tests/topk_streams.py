"""Crafted distance streams for the top-k selection and merge kernels, and what a selection over them must return.

Any float32 stream v[0..n) can be made the exact distance stream of a search over rows v[i] * e0 (every other component
zero), in the GEMV and in the MFMA summation order alike:

  dot     query -s * e0   distance s * v[i]                     (dot_rows_query)
  l2      zero query      distance |v[i]| when v[i]^2 is exact  (the `grid` family)
  cosine  query e0        distance 0 / 1 (zero row) / 2         (cosine_rows)

so the reference needs no distance arithmetic at all: `expected` is numpy's stable argsort of the float64 stream -- ties
go to the lower position --, `expected_mapped` the same through a candidate list (re-rank), `expected_merge` the same over
several lists with a tie rule (the merge entry points).  Nothing here carries a tolerance.  The sign of a zero distance
differs between the summation orders (the kernels' keys canonicalise -0 to +0): compare distances as values, not as bits.

NaN distances are out of scope: no entry point's contract names them, and no family produces one.  +inf with a valid id
appears in the merge streams only (merge_case).
"""
import numpy as np

PLATEAU_SIZES = (2, 32, 33, 256, 257, 400)
MODERATE = ("equal", "two_values", "plateau")      # the families the cosine legs use


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def plateau(n, k, t, where, rs):
    """Distinct gaussian values with a group of t equal ones whose ranks hold the k-th smallest: as the group's first
    element (where = 0), its last (where = 2) or in between (1).  None when n or k leave no room for it."""
    kk = min(k, n)
    j = min((0, t // 2, t - 1)[where], kk - 1)
    start = kk - 1 - j
    if t > n or start + t > n:
        return None
    s = np.sort(rs.randn(n)).astype(np.float32)
    s = np.unique(s)
    if len(s) < n:                                   # (float32 collisions of a gaussian sample: practically never)
        return None
    s[start:start + t] = s[start]
    return _f32(s[rs.permutation(n)])


FAMILIES = ("equal", "two_values", "low_bits", "plateau", "descending", "ascending", "straddle", "grid", "gaussian")
VARIANTS = {
    "two_values": ["two_values_km1", "two_values_k", "two_values_kp1"],
    "low_bits": ["low_bits_256", "low_bits_65536"],
    "plateau": ["plateau_%d_%s" % (t, w) for t in PLATEAU_SIZES for w in ("first", "inside", "last")],
}


def variants(base):
    return VARIANTS.get(base, [base])


def make(name, n, k, rs):
    """The stream of one family variant, or None when (n, k) leave no room for it; k places the boundaries of two_values
    and plateau."""
    if name == "equal":                                  # everything is tie-breaking by position
        return np.full(n, 1.5, np.float32)
    if name.startswith("two_values"):                    # the lower value on k - 1, k, k + 1 positions
        m = max(0, min(n, k + {"km1": -1, "k": 0, "kp1": 1}[name.split("_")[2]]))
        v = np.full(n, 2.0, np.float32)
        v[rs.permutation(n)[:m]] = 1.0
        return v
    if name.startswith("low_bits"):                      # every histogram pass down to sh == 0
        bits = int(name.split("_")[2])
        return (np.uint32(0x3f800000) + rs.randint(0, bits, n).astype(np.uint32)).view(np.float32)
    if name.startswith("plateau"):
        _, t, w = name.split("_")
        where = ("first", "inside", "last").index(w)
        t = int(t)
        if where and min((0, t // 2, t - 1)[where], min(k, n) - 1) == (0, t // 2)[where - 1]:
            return None                                  # (k too small to tell this placement from the one before)
        return plateau(n, k, t, where, rs)
    if name == "descending":                             # every key goes to position 0: the list shifts in full
        return _f32(np.arange(n, 0, -1) * 0.25)
    if name == "ascending":                              # only the first k are ever accepted
        return _f32(np.arange(n) * 0.25 - 3.0)
    if name == "straddle":                               # make_key's orderable transform; a range of nearly all 32 bits
        v = (rs.randn(n) * 10.0 ** rs.randint(-30, 31, n)).astype(np.float32)
        plant = np.array([1e-45, -1e-45, 1.1e-38, -1.1e-38, 5e-39, 3e38, -3e38, 0.0, -0.0, 0.0], np.float32)
        at = rs.permutation(n)[:len(plant)]
        v[at] = plant[:len(at)]
        return v
    if name == "grid":                                   # squares exact in float32: the L2 legs
        return _f32(rs.randint(-2048, 2048, n) / 16.0)
    if name == "gaussian":                               # the control
        return rs.randn(n).astype(np.float32)
    raise KeyError(name)


def families(n, k, rs, names=FAMILIES):
    """(name, float32 stream of length n) for every variant of every family that fits (n, k)."""
    for base in names:
        for name in variants(base):
            v = make(name, n, k, rs)
            if v is not None:
                yield name, v


def sample(n_edges, k_edges, seed, names=FAMILIES, per_pair=3):
    """A sampled cross product, (name, n, k, stream): every family meets every n edge and every k edge at least once
    (26 (n, k) pairs for the edge sets of the GPU legs), each pair with up to `per_pair` of the family's variants in
    rotation; a variant that does not fit a pair (a plateau of 400 among 63 keys) gives way to the next that does."""
    rs = np.random.RandomState(seed)
    N, K = list(n_edges), list(k_edges)
    for gi, base in enumerate(names):
        var = variants(base)
        pairs = [(n, K[(gi + i) % len(K)]) for i, n in enumerate(N)] + [(N[(gi + 3 + i) % len(N)], k) for i, k in enumerate(K)]
        for j, (n, k) in enumerate(pairs):
            got = 0
            for m in range(len(var)):
                name = var[(j * per_pair + m) % len(var)]
                v = make(name, n, k, rs)
                if v is not None:
                    yield name, n, k, v
                    got += 1
                    if got == min(per_pair, len(var)):
                        break


# ---- a stream as the rows and the query of a search ------------------------------------------------------------------
def rows_of(v, dim):
    base = np.zeros((len(v), dim), np.float32)
    base[:, 0] = v
    return base


def unit_query(scale, dim):
    q = np.zeros(dim, np.float32)
    q[0] = scale
    return q


def dot_stream(v, s):
    """The distances of the rows v[i] * e0 from the query -s * e0 under the dot metric: s * v[i] in float32 (s a power
    of two: exact unless it overflows, and a product this large would be a valid +inf, which only the merge legs hold --
    callers halve such a stream first, see fit_scale)."""
    with np.errstate(over="ignore"):
        return (np.float32(s) * _f32(v)).astype(np.float32)


def fit_scale(v, s):
    """v, or v / 4 when s * v would leave the finite float32 range (the stream is whatever the rows give: the expectation
    is computed from the scaled rows, so rounding of a denormal in the division changes nothing)."""
    v = _f32(v)
    if abs(s) > 1 and float(np.abs(v).max(initial=0.0)) * abs(s) > 3.0e38:
        v = (v * np.float32(0.25)).astype(np.float32)
    return v


def cosine_rows(v, k):
    """Row scalars whose cosine distances from e0 keep the stream's boundary: rows below the k-th smallest value point
    along the query (distance 0), rows equal to it are zero rows (1, the zero-norm guard), rows above point away (2).
    Magnitudes 1 + |v| stay moderate (the norm of 1e+-30 under- or overflows).  Returns (row scalars, distance stream)."""
    v = _f32(v).astype(np.float64)
    kth = np.sort(v)[min(k, len(v)) - 1]
    r = np.where(v < kth, 1.0 + np.abs(v), np.where(v > kth, -(1.0 + np.abs(v)), 0.0)).astype(np.float32)
    return r, np.where(r > 0, 0.0, np.where(r < 0, 2.0, 1.0)).astype(np.float32)


# ---- expectations -----------------------------------------------------------------------------------------------------
def expected(stream, k):
    """The k smallest of the stream, ties to the lower position: (positions int32 [k], distances float32 [k]), padded
    with -1 / +inf."""
    s64 = np.asarray(stream, np.float64)
    order = np.argsort(s64, kind="stable")[:k]
    ids = np.full(k, -1, np.int32)
    d = np.full(k, np.inf, np.float32)
    ids[:len(order)] = order
    d[:len(order)] = s64[order]
    return ids, d


def expected_mapped(stream, cand, k):
    """Re-rank: the candidates cand[j] that name a row (0 <= id < len(stream)), stable by (distance, position j in the
    list); the ids are the list's entries (repeats stay)."""
    cand = np.asarray(cand, np.int64)
    pos = np.flatnonzero((cand >= 0) & (cand < len(stream)))
    s64 = np.asarray(stream, np.float64)[cand[pos]]
    order = np.argsort(s64, kind="stable")[:k]
    ids = np.full(k, -1, np.int32)
    d = np.full(k, np.inf, np.float32)
    ids[:len(order)] = cand[pos[order]]
    d[:len(order)] = s64[order]
    return ids, d


def expected_merge(ids, dist, k, order=None):
    """Several lists of one query, ids [nlists][k_in] (-1 = no entry) and distances: the k best, ties to the lower
    list then the lower rank (order None: a stable sort of the concatenation), or to the lower `order` word whatever the
    list (order: uint32 [nlists][k_in])."""
    ids = np.asarray(ids).reshape(-1)
    d64 = np.asarray(dist, np.float64).reshape(-1)
    valid = np.flatnonzero(ids >= 0)
    second = valid if order is None else np.asarray(order).reshape(-1).astype(np.uint32).astype(np.int64)[valid]
    pick = valid[np.lexsort((second, d64[valid]))][:k]
    oi = np.full(k, -1, np.int32)
    od = np.full(k, np.inf, np.float32)
    oi[:len(pick)] = ids[pick]
    od[:len(pick)] = d64[pick]
    return oi, od


def merge_case(v, nlists, k_in, rs, with_inf=True):
    """Per-list ascending lists cut from a stream for one query: list s holds a random number of the stream's values
    (sorted, so equal values meet inside and across lists), a -1 tail, valid +inf entries at the end of some lists, and
    one list is wholly empty when there are more than two.  Ids are unique.  Returns (ids [nlists][k_in], dist)."""
    ids = np.full((nlists, k_in), -1, np.int32)
    dist = np.full((nlists, k_in), np.inf, np.float32)
    empty = rs.randint(0, nlists) if nlists > 2 else -1
    v = _f32(v)
    for s in range(nlists):
        if s == empty:
            continue
        m = k_in if rs.rand() < 0.5 else rs.randint(0, k_in + 1)
        vals = np.sort(v[rs.randint(0, len(v), m)].astype(np.float64), kind="stable").astype(np.float32)
        if with_inf and m >= 2 and rs.rand() < 0.5:
            vals[-(1 + rs.randint(0, min(m, 3))):] = np.inf        # valid entries at +inf: they beat the -1 padding
        dist[s, :m] = vals
        ids[s, :m] = s * k_in + np.arange(m)
    # (dist behind a list's last valid entry stays +inf, the ids there -1)
    return ids, dist


def assert_same(ids, d, want_ids, want_d, what):
    """Exact ids, exact float32 values (values, not bits: -0 == +0)."""
    ids, want_ids = np.asarray(ids), np.asarray(want_ids)
    d, want_d = np.asarray(d, np.float32), np.asarray(want_d, np.float32)
    assert ids.shape == want_ids.shape and d.shape == want_d.shape, (what, ids.shape, want_ids.shape)
    bad = np.argwhere(ids != want_ids)
    assert bad.size == 0, "%s: ids differ first at %s: got %s want %s (distances %s / %s)" % (
        what, bad[0], ids[tuple(bad[0])], want_ids[tuple(bad[0])], d[tuple(bad[0])], want_d[tuple(bad[0])])
    bad = np.argwhere(~(d == want_d))
    assert bad.size == 0, "%s: distances differ first at %s: got %r want %r" % (
        what, bad[0], d[tuple(bad[0])], want_d[tuple(bad[0])])
