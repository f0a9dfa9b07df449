"""What hnswgpu_ivf_search_filtered_each must return, and how its scan walks a list -- restated here, independent of the library.

The expectation.  For ONE mask (bits over row ids) the rule is that of test_ivf_filtered_search.py: with pid = flatnonzero(bits),
every list restricted to its passing rows, renumbered into base[pid], the centroids kept --
O.ivf_search(base[pid], cen, off', lids', Q, k, nprobe, metric, MODE_DEV), ids mapped back through pid: the unmodified oracle's
candidate stream with the failing rows dropped, first k.  For one mask per query the queries are grouped by DISTINCT mask and the
oracle runs once per mask over that mask's queries (a query's oracle result does not depend on the other queries of its call).

The walk.  The device scan serves a (query, list) pair in chunks of chunk_rows list positions (plan_chunks, restated from
engine.hip); the four waves of a chunk's workgroup take its 64-position blocks w, w + 4, ...; a wave queues the passing positions
of a block and evaluates RB of them whenever it holds that many (RB = 8 / 4 / 2 by row width), the leftovers carry into the next
block, the rest is flushed after the last.  wave_walks gives the per-block passing counts of every wave, which is what the crafted
masks of the edge test are chosen by."""
import numpy as np

WAVE, NWAVE = 64, 4


def om(O, metric):
    return {"cosine": O.COSINE, "l2": O.L2, "dot": O.DOT}[metric]


def lists(O, base, nlist, o_metric):
    _, cen, assign = O.ivf_build_dev(base, nlist, max_iterations=3, metric=o_metric)
    off, lids = O.lists_from_assign(assign, nlist)
    return cen, off, lids


def garbage_past_n(mask, n, seed):
    """Random bits at the positions >= n of the last word of every mask row: the library must ignore them."""
    m = np.array(mask, np.uint32, copy=True)
    if n & 31:
        g = np.random.default_rng(seed).integers(0, 1 << 32, size=m.shape[:-1] or None, dtype=np.uint64)
        m[..., -1] |= ((np.asarray(g, np.uint64) >> np.uint64(n & 31)) << np.uint64(n & 31)).astype(np.uint64).astype(np.uint32)
    return m


def expect_single(O, base, cen, off, lids, Q, bits, nprobe, o_metric, k):
    """-> ids, distances, probes (None when nothing passes: the oracle is not asked about an empty base)"""
    nq = len(Q)
    pid = np.flatnonzero(bits)
    if len(pid) == 0:
        return np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf, np.float64), None
    keep = bits[lids]                                                # per list position
    lids2 = np.searchsorted(pid, lids[keep]).astype(np.int32)       # passing rows renumbered into base[pid], list order kept
    off2 = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)[off]   # passing positions below every list's first
    oi, od, pr = O.ivf_search(base[pid], cen, off2, lids2, Q, k, nprobe, metric=o_metric, mode=O.MODE_DEV)
    ids = np.where(oi >= 0, pid[np.maximum(oi, 0)], -1).astype(np.int32)
    return ids, od, pr


def expect_each(O, base, cen, off, lids, Q, masks_bits, which, nprobe, o_metric, k):
    """Query q under mask masks_bits[which[q]]: the oracle once per distinct mask -> ids [nq][k], distances [nq][k] (float64)."""
    which = np.asarray(which)
    ids = np.full((len(Q), k), -1, np.int32)
    d = np.full((len(Q), k), np.inf, np.float64)
    for m, bits in enumerate(masks_bits):
        qs = np.flatnonzero(which == m)
        if len(qs):
            ids[qs], d[qs], _ = expect_single(O, base, cen, off, lids, np.ascontiguousarray(Q[qs]), bits, nprobe, o_metric, k)
    return ids, d


def deal(nq, nmasks):
    """Masks dealt to the queries round-robin."""
    return np.arange(nq) % nmasks


# ---- the walk ----------------------------------------------------------------------------------------------------------------
def nch_of(dim):
    need = -(-((dim + 3) // 4) // WAVE)
    return next(o for o in (1, 2, 3, 4, 6, 8, 12) if o >= need)


def rb_of(dim):
    """Rows a wave evaluates per step: the register rows launch_ivf_filtered_scan's dispatch gives the row width."""
    nch = nch_of(dim)
    return 8 if nch <= 3 else (4 if nch <= 6 else 2)


def plan_chunks(dim, max_rows, mean_rows, npairs, scan_blocks=0):
    """engine.hip plan_chunks for (query, list) pairs -> chunk_rows, nchunks.  scan_blocks: the SCAN_BLOCKS tuning key (0: unset)."""
    per_iter = NWAVE * rb_of(dim)
    max_rows, mean_rows = max(max_rows, 1), max(mean_rows, 1)
    mean_rows = min(mean_rows, max_rows)
    small = min(4096, max(512, 8 * npairs))
    target = scan_blocks if scan_blocks > 0 else (small if npairs <= 4096 else 16384)
    want = max(1, -(-target // max(npairs, 1)))
    if want == 1:
        mean_rows = max_rows
    want = min(want, -(-mean_rows // per_iter))
    cr = -(-mean_rows // want)
    cr = -(-cr // per_iter) * per_iter
    return cr, -(-max_rows // cr)


def wave_walks(keep, chunk_rows):
    """keep: bool per position of ONE list.  -> for every (chunk, wave) with at least one block, the passing counts of its blocks."""
    out = []
    n = len(keep)
    for c0 in range(0, n, chunk_rows):
        c1 = min(c0 + chunk_rows, n)
        for w in range(NWAVE):
            counts = [int(np.sum(keep[b:min(b + WAVE, c1)])) for b in range(c0 + w * WAVE, c1, NWAVE * WAVE)]
            if counts:
                out.append(counts)
    return out


def walk_events(counts, rb):
    """What one wave's walk over blocks with these passing counts does: (full steps inside a block that started with leftovers,
    blocks left with leftovers to carry, size of the final flush)."""
    have = carried_steps = carries = 0
    for i, c in enumerate(counts):
        start = have
        have += c
        steps, have = divmod(have, rb)
        if start and steps:
            carried_steps += 1
        if have and i + 1 < len(counts):
            carries += 1
    return carried_steps, carries, have


# ---- the inputs of the GPU test ----------------------------------------------------------------------------------------------
# ones / zeros and half / not_half are neighbours in the round-robin deal: complementary masks side by side
PARITY_MASKS = ["ones", "zeros", "half", "not_half", "sparse", "one_list"]


def parity_bits(n, seed, off, lids, probes0):
    """The six masks of the parity test over n rows; one_list: exactly the rows of the list query 0 probes first."""
    rng = np.random.default_rng(seed)
    half = rng.random(n) < 0.5
    sparse = rng.random(n) < 0.03
    one = np.zeros(n, np.bool_)
    l = int(probes0[0])
    one[lids[off[l]:off[l + 1]]] = True
    return [np.ones(n, np.bool_), np.zeros(n, np.bool_), half, ~half, sparse, one]


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _by_position(n, off, lids, passing):
    """passing: {list: positions inside the list} -> bits over ROW ids"""
    bits = np.zeros(n, np.bool_)
    for l, pos in passing.items():
        pos = np.asarray(list(pos), np.int64)
        assert len(pos) == 0 or (pos.min() >= 0 and pos.max() < off[l + 1] - off[l])
        bits[lids[off[l] + pos]] = True
    return bits


def _crafted(n, dim, lens, seed):
    from hnsw_clj_amd import datagen

    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert off[-1] == n
    lids = rng.permutation(n).astype(np.int32)                      # a list position is not its row id
    cen = rng.standard_normal((len(lens), dim)).astype(np.float32)
    return datagen.generate_dataset(n, dim), cen, off, lids


def edge_case():
    """300 x 32 in the lists [1, 63, 64, 65, 0, 107], every list probed.  RB = 8 at this row length.  With one chunk per pair
    (SCAN_BLOCKS = 1: 128 positions) wave 0 takes a list's positions 0 .. 63 and wave 1 the rest; the masks, placed by list
    POSITION, give the blocks of the 65-row list (3) and the 107-row list (5) the passing counts
        A:     list 5: 64, 0     list 3: 7, 1      (RB - 1, 1; every other list emptied; 72 rows pass: more than a register list)
        not A: list 5: 0, 43     list 3: 57, 0
        B:     list 5: 8, 9      list 3: 9, 0      (RB, RB + 1), and 1 / 8 / 17 rows of the lists 0 / 1 / 2."""
    from hnsw_clj_amd import datagen

    n, dim, lens = 300, 32, [1, 63, 64, 65, 0, 107]
    base, cen, off, lids = _crafted(n, dim, lens, 11)
    a = _by_position(n, off, lids, {5: range(64), 3: list(range(7)) + [64]})
    b = _by_position(n, off, lids, {5: [0, 9, 18, 27, 36, 45, 54, 63, 64, 65, 70, 80, 90, 100, 104, 105, 106],
                                    3: [1, 2, 3, 5, 8, 13, 21, 34, 55], 0: [0], 1: range(0, 63, 8), 2: range(0, 64, 4)})
    which = deal(6, 3)
    return Case(n=n, dim=dim, nlist=6, nprobe=6, k=100, base=base, cen=cen, off=off, lids=lids, masks=[a, ~a, b], which=which,
                Q=datagen.generate_dataset(len(which), dim, seed=43))


def long_walk_case():
    """900 x 32 in the lists [808, 92], both probed: the 300-row lists above are too short for a wave to walk four blocks.  With one
    chunk per pair (SCAN_BLOCKS = 1: 832 positions) wave w takes the blocks w, w + 4, w + 8 (and wave 0 block 12, 40 positions) of
    the long list.  Mask 0 passes 3, 0, 7 and 2 positions of wave 0's blocks: 3 carried over an empty block, a full step of 8 inside
    the third block with 2 left, a flush of 4 at the end.  Waves 1 .. 3: 5, 64, 10 / 0, 9, 0 / 8, 8, 1.  Mask 1 is its complement."""
    from hnsw_clj_amd import datagen

    n, dim, lens = 900, 32, [808, 92]
    base, cen, off, lids = _crafted(n, dim, lens, 12)
    blk = lambda b, pos: [b * WAVE + p for p in pos]  # noqa: E731
    long_list = (blk(0, [5, 20, 63]) + blk(8, [0, 1, 8, 18, 28, 48, 63]) + blk(12, [0, 39])
                 + blk(1, [0, 7, 31, 32, 63]) + blk(5, range(64)) + blk(9, range(3, 63, 6))
                 + blk(6, [0, 1, 2, 3, 4, 5, 6, 7, 63])
                 + blk(3, range(0, 64, 8)) + blk(7, range(56, 64)) + blk(11, [17]))
    a = _by_position(n, off, lids, {0: long_list, 1: range(92)})
    which = deal(4, 2)
    return Case(n=n, dim=dim, nlist=2, nprobe=2, k=256, base=base, cen=cen, off=off, lids=lids, masks=[a, ~a], which=which,
                Q=datagen.generate_dataset(len(which), dim, seed=43))
