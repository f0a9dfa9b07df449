"""Input builders and float64 references for test_range_search_shapes_gpu.py: large bases, large batches built from a few
distinct query vectors, guarded radii, packed masks and expected CSR results.  Nothing here touches the GPU:
the callers' hnswgpu_batch_distances (the EXISTING entry point, once per distinct vector) for the distance bits."""
import numpy as np

NVEC = 40                           # distinct query vectors of a batch: query q is vector q % NVEC with its own radius
N_BIG = 32 * 1024 + 37              # W = 1026 hit words: two fill blocks of 1024 words, the last word partial
TIED_BIG = (5, 32767, 32768, 32770)  # row 5 copied: exact ties on both sides of the fill blocks' border
ANCHOR = (5, 32790, 10000, 20000, 30000, N_BIG - 1)   # vector j < 6 sits on row ANCHOR[j]: its nearest row, whatever the metric
FAR = 12345                         # the one row farthest from every vector (the radius target "n-1")
NEAR = 1003                         # rows of the nearest population (radius targets up to 65 stay inside it)
# the cycle of radius targets (27: coprime with NVEC, so 1080 queries pair every vector with every target)
TARGETS = (0, 1, 1, 2, 1, 33, "near", 5, 31, "half", 32, 64, 3, "n-1", 65, 7, "nan", 17, "n", 4, 0, 33, 6, 1, 48, 2, 8)


def d64(metric, V, base, block=8192):
    """float64 distances [len(V)][len(base)], the base taken in row blocks."""
    V = V.astype(np.float64)
    out = np.empty((len(V), len(base)))
    vn = np.linalg.norm(V, axis=1)
    for r0 in range(0, len(base), block):
        b = base[r0:r0 + block].astype(np.float64)
        dot = V @ b.T
        if metric == "dot":
            out[:, r0:r0 + block] = -dot
        elif metric == "l2":
            for j, v in enumerate(V):
                out[j, r0:r0 + block] = np.sqrt(((v - b) ** 2).sum(1))
        else:
            out[:, r0:r0 + block] = 1.0 - dot / (vn[:, None] * np.linalg.norm(b, axis=1)[None, :])
    return out


def d32(metric, V, base):
    """The same distances restated in float32 numpy: what float32 arithmetic costs, known before any GPU run."""
    one = np.float32(1.0)
    dot = V @ base.T
    if metric == "dot":
        return -dot
    if metric == "l2":
        return np.stack([np.sqrt(((v - base) ** 2).sum(1, dtype=np.float32)) for v in V])
    return one - dot / (np.linalg.norm(V, axis=1)[:, None] * np.linalg.norm(base, axis=1)[None, :])


def big_data(dim, seed=3):
    """(base [N_BIG][dim], V [NVEC][dim]).  Rows and vectors share one unit direction u: vectors carry alpha u, rows c beta u
    with c = 2 for NEAR rows at random places, 1 for about half of the rest, -1 for the others and -2.5 for row FAR, and noise
    orthogonal to u.
    Under all three metrics the populations are then nearest, middle and far from every vector, with wide gaps between them
    (the radius targets "near" and "half"), while the noise spreads the distances inside a population."""
    rng = np.random.default_rng(seed + dim)
    u = rng.standard_normal(dim)
    u /= np.linalg.norm(u)
    beta = np.sqrt(max(4.0 * np.sqrt(dim), 42.0))
    alpha = 3.0 * beta
    noise = rng.standard_normal((N_BIG + NVEC, dim))
    noise -= (noise @ u)[:, None] * u[None, :]
    c = np.where(rng.random(N_BIG) < 0.5, 1.0, -1.0)
    near = rng.choice(N_BIG, NEAR, replace=False)
    c[near] = 2.0
    c[list(ANCHOR)] = 2.0
    c[FAR] = -2.5
    eta, eps = noise[:N_BIG], noise[N_BIG:]
    eps[:len(ANCHOR)] = eta[list(ANCHOR)]
    base = (c[:, None] * beta * u[None, :] + eta).astype(np.float32)
    for r in TIED_BIG[1:]:
        base[r] = base[TIED_BIG[0]]
    return base, (alpha * u[None, :] + eps).astype(np.float32)


def small_data(n, dim, seed=5):
    rng = np.random.default_rng(seed + n + dim)
    return rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((NVEC, dim)).astype(np.float32)


def _count_radius(s, t, window):
    """The radius for about t hits among the sorted float64 distances s: the midpoint of the largest gap whose count lies within
    `window` of t.  Returns (radius, gap)."""
    n = len(s)
    if t <= 0:
        return s[0] - 1.0, np.inf
    if t >= n:
        return s[-1] + 1.0, np.inf
    cs = np.arange(max(1, t - window), min(n - 1, t + window) + 1)        # counts: s[c - 1] <= radius < s[c]
    c = cs[np.argmax(s[cs] - s[cs - 1])]
    return 0.5 * (s[c - 1] + s[c]), s[c] - s[c - 1]


def radii(dv, nq, targets, tied_row=None, zero_at=()):
    """Per query q of a batch (vector q % NVEC; dv: the vectors' float64 distances): a float64 radius at the middle of a gap
    and that gap.  Targets cycle through `targets`: a count t (the widest gap within +-(3 + t // 8); exact up to 2 for the
    anchored vectors), "near" / "half" (the widest gap within +-128 of NEAR + 128, +-512 of n / 2), "n-1" (exact), "n", "nan";
    with tied_row, the queries of vector 0 alternate between a radius just below the tied distance, one just above it and the
    cycle; the queries in zero_at match nothing."""
    n = dv.shape[1]
    srt = np.sort(dv, axis=1)
    rad, gap = np.empty(nq), np.empty(nq)
    for q in range(nq):
        s, t = srt[q % NVEC], targets[q % len(targets)]
        if q in zero_at:
            t = 0
        elif tied_row is not None and q % NVEC == 0 and (q // NVEC) % 3 < 2:
            dt = dv[0, tied_row]
            lo, hi = s[s < dt], s[s > dt]
            if (q // NVEC) % 3 == 0:
                rad[q], gap[q] = (0.5 * (lo[-1] + dt), dt - lo[-1]) if len(lo) else (dt - 1.0, np.inf)
            else:
                rad[q], gap[q] = (0.5 * (hi[0] + dt), hi[0] - dt) if len(hi) else (dt + 1.0, np.inf)
            continue
        if t == "nan":
            rad[q], gap[q] = np.nan, np.inf
            continue
        window = {"near": 128, "half": 512, "n-1": 0}.get(t, 3 + t // 8 if isinstance(t, int) else 0)
        t = {"near": NEAR + 128, "half": n // 2, "n-1": n - 1, "n": n}.get(t, t)
        if t <= 2 and 0 < q % NVEC < len(ANCHOR) and tied_row is not None:  # an anchored vector: its own row stands apart
            window = 0
        rad[q], gap[q] = _count_radius(s, t, window)
    return rad, gap


def guard(gap, err_v, nq, rad64):
    """Every query's gap exceeds 100 x the largest error of its vector's distances, and the float32 radius stays well inside the
    gap: rounding cannot move a row across a radius.  Returns the smallest gap / error."""
    err = err_v[np.arange(nq) % len(err_v)]
    ok = np.isnan(rad64) | (np.abs(np.float32(rad64).astype(np.float64) - rad64) < gap / 4)
    assert ok.all(), np.flatnonzero(~ok)
    assert (gap > 100 * err).all(), (np.flatnonzero(gap <= 100 * err), (gap / err).min())
    return float((gap / np.maximum(err, 1e-300)).min())


def csr(within, bd, mask=None):
    """The expected CSR result in id order: (lims, ids, distance bits) from within[q][row] (and mask [row] or [q][row]); the
    bits are those of bd[q % len(bd)] (hnswgpu_batch_distances, one row per distinct vector)."""
    if mask is not None:
        within = within & mask
    qi, ids = np.nonzero(within)
    lims = np.zeros(len(within) + 1, np.int64)
    np.cumsum(within.sum(1), out=lims[1:])
    return lims, ids.astype(np.int32), bd.view(np.uint32)[qi % len(bd), ids]


def by_distance(res):
    """The id-order result (lims, ids, bits) in (distance, row id) order, -0 as +0: what HNSWGPU_RANGE_BY_DISTANCE returns."""
    lims, ids, bits = res
    d = bits.view(np.float32) + np.float32(0.0)
    seg = np.repeat(np.arange(len(lims) - 1), np.diff(lims))
    o = np.lexsort((ids, d, seg))
    return lims, ids[o], d[o].view(np.uint32)


def same(got, want, what=""):
    """got: (lims, ids, dist) of a call; want: (lims, ids, bits).  Exact, with the first difference in the message."""
    assert np.array_equal(got[0], want[0]), (what, "lims", np.flatnonzero(got[0] != want[0])[:8])
    assert np.array_equal(got[1], want[1]), (what, "ids", np.flatnonzero(got[1] != want[1])[:8])
    gb = got[2].view(np.uint32)
    assert np.array_equal(gb, want[2]), (what, "distance bits", np.flatnonzero(gb != want[2])[:8])


def bits_of(res):
    return res[0], res[1], res[2].view(np.uint32)


def pack_rows(M):
    """engine.pack_masks for a bool array [nq][n], without a Python loop over the queries."""
    nq, n = M.shape
    W = (n + 31) // 32
    P = np.zeros((nq, W * 32), bool)
    P[:, :n] = M
    return np.ascontiguousarray(np.packbits(P, axis=1, bitorder="little")).view("<u4").reshape(nq, W).astype(np.uint32)


def tq_of(dim):
    """Queries per group (filtered_group_queries of the padded row length)."""
    ld = (dim + 3) // 4 * 4
    return 32 if ld <= 1024 else (16 if ld <= 2048 else 8)


def slicing(n, dim, nq, budget_mb=2048, each=False):
    """range_enqueue's two formulas restated: (G, groups per slice, chunk_rows of the first slice)."""
    tq, W = tq_of(dim), (n + 31) // 32
    G = (nq + tq - 1) // tq
    group_bytes = tq * W * 4 + ((8 * n + 4 * W) if each else 0)
    gps = max(1, min((budget_mb << 20) // group_bytes, 65535 // tq))
    ng = min(gps, G)
    tiles = (n + 255) // 256
    want = max(1, min(tiles, (2048 + ng - 1) // ng))
    return G, gps, (tiles + want - 1) // want * 256


SORT_LENGTHS = (2, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12288, 16384, 16385, 16500)


def tied_data(metric, dim=20, seed=9):
    """(base [16500][dim], q [dim]), small integers: the distances are exact in float32 and tie heavily.  The rows are picked
    from a pool, level by level of the distance to q (17 consecutive levels around the pool's median), so that the counts at
    or below each level are exactly SORT_LENGTHS: every one of those segment lengths is reachable by a radius between two
    levels.  Single rows stand between the large tied groups; for dot, level 0 (distance -0 on the device) is among them."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-1, 3, dim)
    pool = rng.integers(-2, 3, (400000, dim))
    key = -(pool @ q) if metric == "dot" else ((pool - q) ** 2).sum(1)
    sizes = np.diff((0,) + SORT_LENGTHS)
    k0 = int(np.median(key)) - 11
    rows = []
    for j, size in enumerate(sizes):
        have = np.flatnonzero(key == k0 + j)
        assert len(have) >= size, (metric, j, len(have), size)
        rows.append(have[:size])
    rows = rng.permutation(np.concatenate(rows))                          # row id and distance rank: unrelated
    return pool[rows].astype(np.float32), q.astype(np.float32)
