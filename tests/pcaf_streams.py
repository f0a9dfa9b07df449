"""Crafted inputs for the P-HNSW kernels (pcaf_kernels.hpp, pcaf.hip): a Python restatement of the launch plan, builders whose
phase-1 candidate sets are known without a tolerance, and what the searches must return for them.  Shared by
test_pcaf_streams_host.py (the preconditions, no GPU) and test_pcaf_streams_gpu.py (the kernels)."""
import collections
import functools

import numpy as np

import util
from test_pcaf_one_handle_gpu import clustered, reference

# ---- the plan, restated from pcaf.hip / pcaf_kernels.hpp ----------------------------------------------------------------
LDS_MAX = 160 * 1024  # kPcafLdsMax
SLICE = 65536         # kPcafSlice
CUS = 256             # compute units of an MI355X (idx->cus)
MAX_KF = 128          # kPcafMaxKf


def pcaf_tp(T):
    return (T + 7) & ~7


def filter_lds(Tp, kf, nw):
    return 8 * 32 * (2 * kf + 1) + 4 * 32 * (Tp + 4) * (1 + nw) + 4 * 36


def filter_masked_lds(Tp, kf, nw):
    return filter_lds(Tp, kf, nw) + 4 * 64 * nw


def project_nt(T):
    """the NT of pcaf_project_kernel<NT, MAP> that launch_pcaf_project picks"""
    nt = (pcaf_tp(T) + 31) // 32
    return 1 if nt <= 1 else 2 if nt <= 2 else 4 if nt <= 4 else 8


def filter_nv(T):
    """the NV of pcaf_filter_kernel<NV> / pcaf_filter_masked_kernel<NV, EACH> that launch_pcaf_filter[_masked] picks"""
    nv = pcaf_tp(T) // 8
    return next(v for v in (4, 8, 13, 16, 24, 32) if nv <= v)


Plan = collections.namedtuple("Plan", "nw lds slab_rows nslabs")


def filter_plan(n, T, nq, kf, masked, cus=CUS):
    """pcaf_filter_plan as pcaf_search_enqueue calls it: nq is the call's batch (planned at its first slice), kf the
    effective min(k_filter, 3 k, n)"""
    lds = lambda nw: (filter_masked_lds if masked else filter_lds)(pcaf_tp(T), kf, nw)  # noqa: E731
    nw = 8
    while nw > 1 and lds(nw) > LDS_MAX:
        nw >>= 1
    step = nw * 32
    steps, qblocks = (n + step - 1) // step, (min(nq, SLICE) + 31) // 32
    want = max(1, (cus + qblocks - 1) // qblocks)
    slab_rows = max(1, (steps + want - 1) // want) * step
    return Plan(nw, lds(nw), slab_rows, (n + slab_rows - 1) // slab_rows)


def effective_kf(k, k_filter, n):
    return min(k_filter or 32, 3 * k, n)


# ---- helpers ------------------------------------------------------------------------------------------------------------
def cosine64(q, rows):
    q, rows = np.float64(q), np.float64(rows)
    return 1.0 - rows @ q / (np.linalg.norm(rows, axis=1) * np.linalg.norm(q))


def check_bound_distances(ids, d, Q, base):
    """Every returned distance is the f64 cosine distance of the returned id on the original rows; -1 / +inf behind them."""
    for q in range(len(ids)):
        m = int((ids[q] >= 0).sum())
        assert (ids[q][:m] >= 0).all() and (ids[q][m:] == -1).all() and np.isinf(d[q][m:]).all(), q
        assert len(set(ids[q][:m].tolist())) == m, (q, "an id came back twice")
        if m:
            assert util.close(d[q][:m], cosine64(Q[q], base[ids[q][:m]])).all(), q
            assert (np.diff(d[q][:m]) >= 0).all(), (q, "distances are not ascending")


def check_candidate_sets(ids, want_sets, what):
    """k = kf: every candidate of phase 1 comes back, so the returned id set IS phase 1's selection -- no tolerance."""
    for q, want in enumerate(want_sets):
        got = ids[q][ids[q] >= 0].tolist()
        lost, extra = sorted(set(want) - set(got)), sorted(set(got) - set(want))
        assert not lost and not extra and len(got) == len(want), "%s q%d: lost %s, extra %s" % (what, q, lost[:8], extra[:8])


def exact_phase2(Q, base, cand_sets, k):
    """f64 refine of known candidate sets -> ids [nq][k] (-1 padded), distances (+inf padded)"""
    ids, dist = np.full((len(Q), k), -1, np.int32), np.full((len(Q), k), np.inf)
    for q, cand in enumerate(cand_sets):
        cand = np.asarray(cand, np.int64)
        if len(cand) == 0:
            continue
        d2 = cosine64(Q[q], base[cand])
        top = np.lexsort((cand, d2))[:k]
        ids[q, :len(top)], dist[q, :len(top)] = cand[top], d2[top]
    return ids, dist


# ---- 1. exact needles ---------------------------------------------------------------------------------------------------
# name: (T, dim, n, kf).  dim > T, never a multiple of 32, and odd / not a multiple of 4 in several shapes (the projection
# kernel's scalar chunk tail); n is odd, so the last needle sits on a ragged last row.
NEEDLES = {
    "T40": (40, 77, 601, 24),
    "T64": (64, 100, 701, 24),
    "T112": (112, 150, 811, 24),
    "T128_nw4": (128, 200, 901, 32),
    "T136": (136, 301, 907, 24),
    "T192_nw2": (192, 260, 1103, 128),
    "T250_padded": (250, 333, 1301, 24),
    "T256_nw2": (256, 300, 1499, 32),
    "T256_nw1": (256, 300, 1499, 128),
    "T120_split": (120, 131, 777, 37),
}
# what the issue's table says each shape reaches: name -> (NT, NV, plain nw, masked nw); None: not pinned by the table
NEEDLE_REACH = {
    "T40": (2, 8, None, None), "T64": (2, 8, None, None), "T112": (4, 16, None, None), "T128_nw4": (4, 16, 4, 4),
    "T136": (8, 24, None, None), "T192_nw2": (8, 24, 2, 2), "T250_padded": (8, 32, None, None), "T256_nw2": (8, 32, 2, 2),
    "T256_nw1": (8, 32, 1, 1), "T120_split": (4, 16, 8, 4),
}
NEEDLE_NQ = 33  # two query blocks, the second ragged

Needles = collections.namedtuple("Needles", "T dim n kf pi P base Q comp sign member needle_id")


def component_sets(T, nq=NEEDLE_NQ):
    """member [nq][T]: query m asks for the components c = m (mod nq) and, for three queries in four, a few strided extras.
    Every component is in a set; no set is larger than 12, so with kf >= 24 every needle of a set is a candidate."""
    member = np.zeros((nq, T), bool)
    for m in range(nq):
        member[m, m::nq] = True
        member[m, [(5 * m + 11 * i) % T for i in range(m % 4)]] = True
    return member


@functools.lru_cache(maxsize=None)
def needle_inputs(name):
    T, dim, n, kf = NEEDLES[name]
    rng = np.random.RandomState(1000 * T + kf)
    pi = rng.permutation(dim)[:T]
    if dim - 1 not in pi:
        pi[T // 2] = dim - 1  # the last float of the last chunk is selected
    rest = np.setdiff1d(np.arange(dim), pi)
    P = np.zeros((T, dim), np.float32)
    P[np.arange(T), pi] = 1.0
    slots = np.linspace(1, n - 1, T).astype(np.int64)  # distinct (n >= 2 T), interleaved with fillers, the last is row n - 1
    needle_id = slots[(37 * np.arange(T)) % T]         # (37 is coprime to every T of the table: needle order != id order)
    base = np.zeros((n, dim), np.float32)
    base[:, rest] = 0.3 * rng.randn(n, len(rest))
    comp, sign = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    comp[needle_id], sign[needle_id] = np.arange(T), 1
    fillers = np.flatnonzero(sign == 0)
    neg = fillers[1::2]                                # every other filler: a negated one-hot; the others project to zero
    comp[neg], sign[neg] = (5 * np.arange(len(neg))) % T, -1
    live = np.flatnonzero(sign != 0)
    base[live, pi[comp[live]]] = sign[live]
    member = component_sets(T)
    Q = np.zeros((NEEDLE_NQ, dim), np.float32)
    Q[:, rest] = 0.3 * rng.randn(NEEDLE_NQ, len(rest))
    for m in range(NEEDLE_NQ):
        Q[m, pi[member[m]]] = 1.0
    for a in (P, base, Q):
        a.setflags(write=False)
    return Needles(T, dim, n, kf, pi, P, base, Q, comp, sign, member, needle_id)


def needle_dots(inp):
    """int [nq][n]: the projected dot of every (query, row) pair -- 1, 0 or -1, exact in any arithmetic"""
    hit = np.where(inp.comp >= 0, inp.member[:, np.maximum(inp.comp, 0)], False)
    return hit * inp.sign[None, :]


def needle_candidates(inp, allow=None):
    """Phase 1 by the rule alone.  Projected norms are 1 (0 for the zero fillers) and sqrtf(|S_m|), dots are 1, 0, -1: a needle
    of S_m is at 1 - 1 / sqrtf(|S_m|) < 1, a negated filler of S_m at 1 + 1 / sqrtf(|S_m|) > 1, everything else at exactly 1
    (the zero fillers by finish_dist's rn == 0 branch).  Equal distances order by row id (make_key).  allow: None, bool [n]
    or bool [nq][n] -> the passing rows only."""
    dots, sets = needle_dots(inp), []
    for q in range(len(inp.Q)):
        rows = np.arange(inp.n) if allow is None else np.flatnonzero(allow if np.ndim(allow) == 1 else allow[q])
        sets.append(rows[np.lexsort((rows, -dots[q, rows]))][:inp.kf])
    return sets


@functools.lru_cache(maxsize=None)
def needle_masks(name):
    """form -> bool mask(s): all rows; one mask that clears every third needle and every fifth row; one mask per query."""
    inp = needle_inputs(name)
    rng = np.random.RandomState(77 + inp.T)
    some = np.ones(inp.n, bool)
    some[inp.needle_id[::3]] = False
    some[4::5] = False
    each = rng.rand(NEEDLE_NQ, inp.n) < 0.7
    each[1] = True
    each[2] = False
    each[2, inp.needle_id[:5]] = True  # fewer rows than kf pass: padding
    each[3] = False                    # nothing passes
    each[32] = some                    # (the ragged block's only query)
    return {"plain": None, "ones": np.ones(inp.n, bool), "some": some, "each": each}


@functools.lru_cache(maxsize=None)
def needle_expected(name, form):
    """-> (candidate sets, ids [nq][kf], f64 distances) of a search with k = k_filter = kf"""
    inp = needle_inputs(name)
    sets = needle_candidates(inp, needle_masks(name)[form])
    return (sets,) + exact_phase2(inp.Q, inp.base, sets, inp.kf)


# ---- 2. stream orders ---------------------------------------------------------------------------------------------------
STREAM_KF = (1, 2, 64, 127, 128)
STREAM_ORDERS = ("monotone", "sawtooth", "identical", "planted")
STREAM_N, STREAM_T, STREAM_NQ = 1500, 16, 33  # 1500 % 32 = 28: a ragged last step; two query blocks
# the refine merge: name -> (T, n, nq) at kf = 128, order "monotone"
MERGE = {"T16_17_slabs": (16, 4100, 5), "T256_47_slabs": (256, 1500, 5)}

Stream = collections.namedtuple("Stream", "T dim n kf P base Q rank")


def planted_rows(n, plan):
    """Row ids on the edges of the plan, most exposed first: the last row, the first and last row of every slab, the last row
    of every wave's step in the first step of every slab."""
    ids = [n - 1]
    for s in range(plan.nslabs):
        lo, hi = s * plan.slab_rows, min(n, (s + 1) * plan.slab_rows)
        ids += [hi - 1, lo]
    for s in range(plan.nslabs):
        lo, hi = s * plan.slab_rows, min(n, (s + 1) * plan.slab_rows)
        ids += [r for r in range(lo + 31, min(hi, lo + plan.nw * 32), 32)]
    return list(dict.fromkeys(ids))


def stream_ranks(order, n, kf, plan):
    """rank[id]: 0 is the row nearest to the even queries (and farthest from the odd ones)"""
    ids = np.arange(n)
    if order == "monotone":   # even queries: strictly descending distance by id; odd queries: strictly ascending
        return n - 1 - ids
    step = plan.nw * 32
    if order == "sawtooth":   # descending inside every step, the steps interleaved: each step brings rows of every level
        return np.argsort(np.argsort((step - 1 - ids % step) * ((n + step - 1) // step) + ids // step))
    if order == "planted":
        first = planted_rows(n, plan)[:kf]
        others = np.random.RandomState(5).permutation(np.setdiff1d(ids, first))
        rank = np.empty(n, np.int64)
        rank[np.concatenate([first, others]).astype(np.int64)] = ids
        return rank
    assert order == "identical"
    return np.zeros(n, np.int64)


def stream_distance(rank, n, kf):
    """The designed projected cosine distance to the even queries: 0.85 / n a rank, and 0.02 more behind rank kf - 1 and behind
    rank n - kf - 1 (the boundary the odd queries see from the other side)."""
    return 0.05 + 0.85 * rank / n + 0.02 * (rank >= kf) + 0.02 * (rank >= n - kf)


@functools.lru_cache(maxsize=None)
def stream_inputs(order, kf, T=STREAM_T, n=STREAM_N, nq=STREAM_NQ):
    """P keeps the first T coordinates.  A row's projection is s (cos t, 0, ..., 0, sin t) with 1 - cos t its designed distance;
    even queries point along coordinate 0, odd ones along coordinate T - 1, so one input is a descending AND an ascending
    stream.  Everything behind coordinate T is noise that only phase 2 sees."""
    dim = T + 8
    rng = np.random.RandomState(100 * kf + T)
    rank = stream_ranks(order, n, kf, filter_plan(n, T, nq, kf, False))
    c = 1.0 - stream_distance(rank, n, kf)
    scale = np.ones(n) if order == "identical" else 0.5 + 1.5 * rng.rand(n)
    base = rng.randn(n, dim)
    base[:, :T] = 0.0
    base[:, 0], base[:, T - 1] = scale * c, scale * np.sqrt(1.0 - c * c)
    Q = rng.randn(nq, dim)
    Q[:, :T] = 0.0
    Q[0::2, 0] = 1.0 + np.arange(0, nq, 2) / 8.0
    Q[1::2, T - 1] = 1.0 + np.arange(1, nq, 2) / 8.0
    P = np.eye(T, dim, dtype=np.float32)
    base, Q = np.float32(base), np.float32(Q)
    for a in (P, base, Q):
        a.setflags(write=False)
    return Stream(T, dim, n, kf, P, base, Q, rank)


@functools.lru_cache(maxsize=None)
def stream_masks(n, nq):
    """form -> bool mask(s); the per-query form cycles through three masks"""
    rng = np.random.RandomState(9)
    one = rng.rand(n) < 0.6
    three = [rng.rand(n) < 0.7, rng.rand(n) < 0.2, np.ones(n, bool)]
    return {"plain": None, "one": one, "each": np.stack([three[q % 3] for q in range(nq)])}


def reference_under(base, P, Q, k, k_filter, allow):
    """reference() over the passing rows, ids mapped back; allow: None, bool [n], or bool [nq][n] (equal masks share a call)
    -> ids, f64 distances, decided"""
    nq = len(Q)
    if allow is None:
        return reference(base, P, Q, k, k_filter)[:3]
    allow = np.asarray(allow)
    if allow.ndim == 1:
        allow = np.broadcast_to(allow, (nq, len(base)))
    ids, dist, decided = np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf), np.ones(nq, bool)
    groups = collections.defaultdict(list)
    for q in range(nq):
        groups[allow[q].tobytes()].append(q)
    for qs in groups.values():
        rows = np.flatnonzero(allow[qs[0]])
        if len(rows) == 0:
            continue
        wi, wd, dec, _, _ = reference(base[rows], P, Q[qs], k, k_filter)
        ids[qs], dist[qs], decided[qs] = np.where(wi >= 0, rows[np.maximum(wi, 0)], -1), wd, dec
    return ids, dist, decided


@functools.lru_cache(maxsize=None)
def stream_expected(order, kf, k, form, T=STREAM_T, n=STREAM_N, nq=STREAM_NQ):
    inp = stream_inputs(order, kf, T, n, nq)
    return reference_under(inp.base, inp.P, inp.Q, k, kf, stream_masks(n, nq)[form])


def boundary_margin(inp, allow=None):
    """min over the queries of (gap between the kf-th and the (kf + 1)-th f64 projected distance) / util's tolerance there"""
    low, qlow = np.float64(inp.base[:, :inp.T]), np.float64(inp.Q[:, :inp.T])
    worst = np.inf
    for q in range(len(qlow)):
        rows = np.arange(inp.n) if allow is None else np.flatnonzero(allow if np.ndim(allow) == 1 else allow[q])
        if len(rows) <= inp.kf:
            continue
        d = np.sort(cosine64(qlow[q], low[rows]))
        a, b = d[inp.kf - 1], d[inp.kf]
        worst = min(worst, (b - a) / (util.RTOL * abs(b) + util.ATOL))
    return worst


# ---- 3. the second slice of queries -------------------------------------------------------------------------------------
# (seed: the f64 reference alone leaves none of the sampled queries undecided, with and without the mask)
SLICED = dict(n=300, dim=32, T=8, nq=SLICE + 33, k=10, kf=32, seed=12)
Sliced = collections.namedtuple("Sliced", "base Q allow sample")


@functools.lru_cache(maxsize=None)
def sliced_inputs():
    s = SLICED
    rng = np.random.RandomState(s["seed"])
    base = clustered(s["n"], s["dim"])
    Q = np.float32(rng.randn(s["nq"], s["dim"]))
    allow = rng.rand(s["n"]) < 0.5
    sample = np.unique(np.r_[np.arange(16) * (s["nq"] // 16), SLICE - 1, SLICE, SLICE + 1, s["nq"] - 1])
    for a in (base, Q, allow):
        a.setflags(write=False)
    return Sliced(base, Q, allow, sample)


def sliced_each_words():
    """The per-query masks of the sliced batch as engine.pack_masks lays them out, drawn as words (every query its own; about
    half the rows pass; the bits behind row n - 1 are clear)."""
    s = SLICED
    words = np.random.RandomState(s["seed"] + 1).randint(0, 2**32, size=(s["nq"], (s["n"] + 31) // 32), dtype=np.uint32)
    if s["n"] & 31:
        words[:, -1] &= np.uint32((1 << (s["n"] & 31)) - 1)
    return words


# ---- 4. mutated handles at the projection widths the mutation tests leave out ---------------------------------------------
MUTATION_SHAPES = [(72, 40), (300, 256)]  # (dim, T): NT = 2 and NT = 8
MUTATION_SCRIPTS = ["interleaved", "update_129", "add_129_onto_700", "remove_all_then_add"]
