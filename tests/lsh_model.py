"""numpy restatement of src/hnsw/ann/hash/hybrid_lsh.clj, independent of the library: the hash (:33-55), the buckets in
insertion order (:105-129), the probe order (:307-327), the per-probe truncation (:147-193), the dedup by first occurrence and
the stable sort (:330-342).  Distances come in as a dense row per query, so the model says nothing about arithmetic."""
import numpy as np

# hybrid_lsh.clj:350-364
MODES = {"turbo": (2, 1), "fast": (4, 1), "balanced": (6, 2), "accurate": (8, 3), "precise": (8, 4)}


def codes_from_dots(dots):
    """dots (n, T, B) -> codes (n, T): bit i of table t = dots[:, t, i] >= 0.0 (-0.0 counts as >= 0, as in the JVM)."""
    dots = np.asarray(dots)
    w = (1 << np.arange(dots.shape[2], dtype=np.uint32))
    return ((dots >= 0.0).astype(np.uint32) * w).sum(axis=2).astype(np.uint16)


def dots_f64(X, planes):
    return np.einsum("nd,tbd->ntb", np.asarray(X, np.float64), np.asarray(planes, np.float64))


def hash_codes(X, planes):
    """Codes under f64 dots: what the device gives wherever no dot is within f32 rounding of zero."""
    return codes_from_dots(dots_f64(X, planes))


def buckets(codes, bits):
    """Stable counting sort per table: off (T, 2^bits + 1), ids (T, n); rows ascending inside a bucket."""
    codes = np.asarray(codes)
    n, T = codes.shape
    off = np.zeros((T, (1 << bits) + 1), np.int64)
    ids = np.zeros((T, n), np.int32)
    for t in range(T):
        off[t, 1:] = np.cumsum(np.bincount(codes[:, t], minlength=1 << bits))
        ids[t] = np.argsort(codes[:, t], kind="stable")
    return off, ids


def probe_sequence(qcode, bits, num_probes, probe_radius):
    """[(table, bucket, is_own_bucket)] in the order search-hybrid-multiprobe's sequential branch visits them."""
    seq = []
    for t in range(min(num_probes, len(qcode))):
        c = int(qcode[t])
        seq.append((t, c, True))
        for j in range(min(probe_radius, bits)):
            seq.append((t, c ^ (1 << j), False))
    return seq


def search(drow, qcode, off, ids, bits, k, num_probes, probe_radius, take_main, take_flip):
    """One query: drow[r] = its distance to row r.  Returns the row ids, at most k."""
    cands = []
    for t, b, own in probe_sequence(qcode, bits, num_probes, probe_radius):
        rows = ids[t, off[t, b]:off[t, b + 1]]
        take = take_main if own else take_flip
        if len(rows) > take:  # (:153: a bucket of no more than `take` rows is returned whole, unsorted)
            rows = rows[np.argsort(drow[rows], kind="stable")][:take]
        cands.extend(int(r) for r in rows)
    seen, unique = set(), []
    for r in cands:
        if r not in seen:
            seen.add(r)
            unique.append(r)
    unique.sort(key=lambda r: drow[r])  # stable, as Collections/sort
    return unique[:k]


def search_batch(D, qcodes, off, ids, bits, k, num_probes, probe_radius, take_main, take_flip):
    """-> ids (nq, k) padded with -1, distances (nq, k) padded with +inf, of D's dtype"""
    nq = len(qcodes)
    oi = np.full((nq, k), -1, np.int32)
    od = np.full((nq, k), np.inf, D.dtype)
    for q in range(nq):
        r = search(D[q], qcodes[q], off, ids, bits, k, num_probes, probe_radius, take_main, take_flip)
        oi[q, :len(r)] = r
        od[q, :len(r)] = D[q, r]
    return oi, od


# ---- examples worked by hand: dim 4, 2 tables x 2 bits, axis-aligned planes, Euclidean distance --------------------------------
# table 0: bit 0 = x0 >= 0, bit 1 = x1 >= 0; table 1: bit 0 = x2 >= 0, bit 1 = x3 >= 0
HAND_PLANES = np.eye(4, dtype=np.float32).reshape(2, 2, 4)
HAND_ROWS = np.array([
    [1, 1, 1, 1],    # 0: codes (3, 3), distance 0
    [1, 1, 1, 2],    # 1: codes (3, 3), distance 1
    [1, 3, -1, 1],   # 2: codes (3, 2), distance sqrt(8)
    [-1, 1, 1, 4],   # 3: codes (2, 3), distance sqrt(13)
    [-1, 1, 1, 1],   # 4: codes (2, 3), distance 2
    [1, -1, 1, 1],   # 5: codes (1, 3), distance 2
    [-1, 1, 1, 1],   # 6: row 4 again
], np.float32)
HAND_QUERY = np.array([1, 1, 1, 1], np.float32)   # codes (3, 3)
HAND_CODES = np.array([[3, 3], [3, 3], [3, 2], [2, 3], [2, 3], [1, 3], [2, 3]], np.uint16)
# table 0: bucket 1 = [5], 2 = [3, 4, 6], 3 = [0, 1, 2]; table 1: bucket 2 = [2], 3 = [0, 1, 3, 4, 5, 6]
# (k, num_probes, probe_radius, take_main, take_flip) -> ids
HAND_CASES = [
    # Both own buckets are cut to their 2 nearest rows, [0, 1] each, BEFORE the dedup: two results.  Deduplicating first
    # (the 3 nearest distinct rows of the probed buckets) would give [0, 1, 4].
    ((3, 2, 0, 2, 1), [0, 1]),
    # One table, both flips: own [0, 1, 2] -> 0, 1; bit 0 flipped: bucket 2 = [3, 4, 6] -> 4 (ties with its twin 6, earlier in the
    # bucket); bit 1 flipped: bucket 1 = [5].  4 and 5 tie at distance 2: 4 was met first.
    ((4, 1, 2, 2, 1), [0, 1, 4, 5]),
    ((3, 1, 2, 2, 1), [0, 1, 4]),
    # Two tables, one flip: stream 0 1 | 4 | 0 1 | 2 -> rows 0 and 1 found through both tables count once; four results for k = 5.
    ((5, 2, 1, 2, 1), [0, 1, 4, 2]),
    # takes larger than every bucket: whole buckets in bucket order, 0 1 2 | 3 4 6 | 5, then the stable sort: 4, 6, 5 tie at 2
    ((7, 1, 2, 8, 8), [0, 1, 4, 6, 5, 2, 3]),
]


def hand_distances():
    return np.sqrt(((HAND_ROWS.astype(np.float64) - HAND_QUERY.astype(np.float64)) ** 2).sum(axis=1))
