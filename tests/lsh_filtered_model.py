"""The filtered hybrid LSH search (include/hnswgpu.h: hnswgpu_lsh_search_filtered) as a numpy model: lsh_model.search with one
added line -- a probed bucket lists only its passing rows, in bucket order, BEFORE the take.  Everything else (probe order,
truncation before the dedup, first occurrence, stable sort) is lsh_model's, restated here because the line sits in its middle."""
import numpy as np

import lsh_model as M


def search(drow, qcode, off, ids, bits, k, num_probes, probe_radius, take_main, take_flip, allow):
    """One query: drow[r] = its distance to row r, allow[r] = row r passes.  Returns the row ids, at most k."""
    cands = []
    for t, b, own in M.probe_sequence(qcode, bits, num_probes, probe_radius):
        rows = ids[t, off[t, b]:off[t, b + 1]]
        rows = rows[allow[rows]]   # the one added line: filter first, then take
        take = take_main if own else take_flip
        if len(rows) > take:
            rows = rows[np.argsort(drow[rows], kind="stable")][:take]
        cands.extend(int(r) for r in rows)
    seen, unique = set(), []
    for r in cands:
        if r not in seen:
            seen.add(r)
            unique.append(r)
    unique.sort(key=lambda r: drow[r])  # stable, as Collections/sort
    return unique[:k]


def post_filter(drow, qcode, off, ids, bits, k, num_probes, probe_radius, take_main, take_flip, allow):
    """The other rule, for the record: the unfiltered search with the same takes, then drop what fails, keep k."""
    return [r for r in M.search(drow, qcode, off, ids, bits, len(drow), num_probes, probe_radius, take_main, take_flip) if allow[r]][:k]


def search_batch(D, qcodes, off, ids, bits, k, num_probes, probe_radius, take_main, take_flip, allow):
    """allow: bool (n,) -- one mask for the batch -- or bool (nq, n), row q for query q.
    -> ids (nq, k) padded with -1, distances (nq, k) padded with +inf, of D's dtype"""
    allow = np.asarray(allow, np.bool_)
    nq = len(qcodes)
    oi = np.full((nq, k), -1, np.int32)
    od = np.full((nq, k), np.inf, D.dtype)
    for q in range(nq):
        a = allow if allow.ndim == 1 else allow[q]
        r = search(D[q], qcodes[q], off, ids, bits, k, num_probes, probe_radius, take_main, take_flip, a)
        oi[q, :len(r)] = r
        od[q, :len(r)] = D[q, r]
    return oi, od


def passing_per_probe(qcode, off, ids, bits, num_probes, probe_radius, take_main, take_flip, allow):
    """[(passing rows in the probed bucket, its take)] in probe order"""
    out = []
    for t, b, own in M.probe_sequence(qcode, bits, num_probes, probe_radius):
        rows = ids[t, off[t, b]:off[t, b + 1]]
        out.append((int(allow[rows].sum()), take_main if own else take_flip))
    return out


# ---- examples worked by hand on lsh_model's HAND_ROWS / HAND_PLANES / HAND_QUERY (query codes (3, 3)) --------------------------
# table 0: bucket 1 = [5], 2 = [3, 4, 6], 3 = [0, 1, 2]; table 1: bucket 2 = [2], 3 = [0, 1, 3, 4, 5, 6]
# distances: 0: 0, 1: 1, 2: sqrt(8), 3: sqrt(13), 4: 2, 5: 2, 6: 2
def _mask(clear=(), only=None):
    m = np.ones(len(M.HAND_ROWS), np.bool_) if only is None else np.zeros(len(M.HAND_ROWS), np.bool_)
    m[list(clear)] = False
    if only is not None:
        m[list(only)] = True
    return m


# (name, mask, (k, num_probes, probe_radius, take_main, take_flip), filter-then-take ids, take-then-filter ids)
HAND_FILTERED = [
    # (a) row 0 cleared.  Table 0, own bucket 3: [0, 1, 2] -> passing [1, 2], no more than take 2: kept whole.  Table 1, own
    # bucket 3: [0, 1, 3, 4, 5, 6] -> passing [1, 3, 4, 5, 6], the 2 nearest: 1 (1), 4 (2; ties with 5 and 6, earlier in the
    # bucket).  Stream 1 2 | 1 4 -> distinct 1 2 4 -> sorted by distance 1 (1), 4 (2), 2 (sqrt 8).
    # Take-then-filter: both own buckets are cut to [0, 1] (HAND_CASES[0]) -> [0, 1] -> drop 0 -> [1].
    ("a_row0_cleared", _mask(clear=[0]), (3, 2, 0, 2, 1), [1, 4, 2], [1]),
    # (b) the twins 4 / 6 (one vector at two ids): 4 cleared.  One table, both flips: own [0, 1, 2] -> 0, 1; bit 0 flipped: bucket
    # 2 = [3, 4, 6] -> passing [3, 6] -> take 1: 6 (2 < sqrt 13); bit 1 flipped: bucket 1 = [5].  6 and 5 tie at 2: 6 was met first.
    # Take-then-filter: bucket 2 gives 4 (HAND_CASES[1]), which fails: [0, 1, 5].
    ("b_twin4_cleared", _mask(clear=[4]), (4, 1, 2, 2, 1), [0, 1, 6, 5], [0, 1, 5]),
    # ... and 6 cleared instead: nothing changes against the unfiltered case, 4 stood before its twin anyway
    ("b_twin6_cleared", _mask(clear=[6]), (4, 1, 2, 2, 1), [0, 1, 4, 5], [0, 1, 4, 5]),
    # only far rows pass: own bucket [0, 1, 2] -> [2]; bucket 2 -> [3]; bucket 1 -> none.  Take-then-filter finds neither:
    # 0 1 | 4 | 5 all fail.
    ("far_rows_only", _mask(only=[2, 3]), (4, 1, 2, 2, 1), [2, 3], []),
    # (c) nothing passes
    ("c_all_zeros", _mask(only=[]), (5, 2, 1, 2, 1), [], []),
]
# (d) an all-ones mask: lsh_model.HAND_CASES unchanged
HAND_ALL_ONES = [(cfg, want) for cfg, want in M.HAND_CASES]
