"""TEST INFRASTRUCTURE: scripted layer-0 graphs that drive the HNSW traversal's candidate list into its edge states, and a
plain restatement of search-layer-ultra that says which states a graph reaches.

The parity tests search graphs a builder made from clustered or gaussian rows: an expansion finds a few fresh neighbours, one
or two are admitted, the list moves a step at a time.  The wave and several-CU kernels keep that list as a main list in LDS, an
admission buffer in registers and a 64-entry tail window (hnsw_list.hpp: HnswList); its hard states -- 64 fresh neighbours
all admitted, evictions that empty the tail window, evictions split between the two tails on a tie, a forced merge followed
by a multi-admit, a fan-out wider than the list -- are reached here on purpose.

A graph is SCRIPTED: every node has an integer `value` in [1, 4096), its intended distance rank from the scripted query, and
64 layer-0 slots (M = 32).  `embed` turns values into rows whose device-order distance (oracle.distance_dev) has exactly the
order and the ties of the values, for each metric; `check_embedding` asserts that on the distances themselves.

    l2             row (+-value, 0, ...), query the origin: the distance IS the value, exactly
    cosine, dot    row r (cos t, +-sin t, 0, ...), t growing with the value, query (1, 0, ...)

`trace` is NOT a model of the kernels' list: two sorted Python lists, the reference's loop (ultra_fast.clj:151-212) one
neighbour at a time, and a log of what every expansion did.  tests/test_scripted_graph_traces.py checks it against the oracle
and asserts from the log that every scenario reaches the state it is named after; tests/test_hnsw_scripted_graphs.py runs the
same cases through every traversal kernel on the GPU.
"""
import bisect
import collections

import numpy as np

M, M0 = 32, 64
METRICS = ("l2", "cosine", "dot")
DIMS = (8, 768)          # 768: another NCH instantiation, zero-padded (the scripted distances keep their bits' order)
MAX_VALUE = 4096

Case = collections.namedtuple("Case", "name values signs l0 entry efs roles")
# What ONE expansion did.  list_full: `nearest` held ef entries when it began; n_survivors: fresh neighbours below the worst
# the expansion found (all of them while the list is not full); n_evicted_old: entries of `nearest` as the expansion found it
# that left; n_admitted_then_evicted: neighbours admitted by this expansion and pushed out again by a later one of its own;
# on_tie: the expanded candidate had LEFT `nearest` and ties its worst (the reference's <=, :175-178); boundary_tie: two or more
# were admitted and the nearest entry that left ties the worst entry that stayed; worst: the worst of `nearest` AFTER the expansion
# (None while it is not full); n_tied_out: the entries that have left `nearest` by then and tie that worst, expanded or not -- what a
# kernel's list has to keep behind its ef entries (the ghosts of kernels.hpp, the run behind `nearest` of hnsw_list.hpp: compact)
Event = collections.namedtuple(
    "Event", "node list_full n_fresh n_survivors n_admitted n_evicted_old n_admitted_then_evicted on_tie boundary_tie worst n_tied_out")
# stop: (node, its distance, the worst) or None; visited: every node whose distance the search evaluated
Trace = collections.namedtuple("Trace", "ids evals hops events stop visited")


# ---- embeddings ----------------------------------------------------------------------------------------------------------
def embed(values, signs, metric, dim):
    """Rows (n, dim) f32 and the scripted query (dim,) f32.  Equal values give bit-identical distances from the query: the
    sign lands in a component the query has a zero in."""
    v = np.asarray(values, np.int64)
    s = np.asarray(signs, np.int64)
    assert v.min() >= 1 and v.max() < MAX_VALUE and set(np.unique(s)) <= {-1, 1}
    rows = np.zeros((len(v), dim), np.float32)
    q = np.zeros(dim, np.float32)
    if metric == "l2":
        rows[:, 0] = (v * s).astype(np.float32)
    else:
        t = (v + 200).astype(np.float64) * (2.4 / (MAX_VALUE + 200))      # (0.1, 2.4] rad: 1 - cos t and -cos t both grow
        r = 1.0 + (v % 5) * 0.25 if metric == "cosine" else np.full(len(v), 2.0)
        rows[:, 0] = (r * np.cos(t)).astype(np.float32)
        rows[:, 1] = (r * np.sin(t) * s).astype(np.float32)
        q[0] = 1.0
    return rows, q


def dev_distances(O, metric, q, rows):
    code = {"l2": O.L2, "cosine": O.COSINE, "dot": O.DOT}[metric]
    return np.array([O.distance_dev(code, q, r) for r in rows], np.float64)


def check_embedding(values, dist):
    """The device-order distances have the order AND the ties of the values (asserted on the distances, not on angles)."""
    v = np.asarray(values)
    order = np.argsort(v, kind="stable")
    vs, ds = v[order], np.asarray(dist)[order]
    same = vs[1:] == vs[:-1]
    assert np.all(ds[1:][same] == ds[:-1][same]), "equal values must tie bit for bit"
    assert np.all(ds[1:][~same] > ds[:-1][~same]), "distinct values must keep their strict order"


def graph(O, case):
    """Layer 0 only, the layout hnswgpu_set_graph takes: levels 0, no upper blocks, max_level 0."""
    n = len(case.values)
    return O.Graph(np.zeros(n, np.int32), case.l0, np.zeros(n + 1, np.int64), np.zeros(0, np.int32), M, case.entry, 0)


def queries(case, metric, dim, nq=130):
    """The scripted query nq - 3 times, then three rows of the graph as queries (seeded by the graph's size)."""
    rows, q = embed(case.values, case.signs, metric, dim)
    pick = np.random.RandomState(len(rows)).choice(len(rows), 3, replace=False)
    return rows, np.ascontiguousarray(np.vstack([np.tile(q, (nq - 3, 1)), rows[pick]]), np.float32)


# ---- scenario S: the full fan-out, with a consequence -------------------------------------------------------------------
V_N, V_H, V_Y, V_HUB, V_A, V_G, V_F, V_E = 100, 500, 700, 800, 1000, 2000, 2100, 3900


def scenario_s(ef=80, kind="plain"):
    """Nodes by distance from the query: N0..N63 (nearest), H, Y, [hubs], A0.., G, F0..F62, E (the entry).

    ef < 128 (the base layout):  E -> F0..F62, G;  G -> A0..A[a-1], H;  H -> N0..N63;  A[a-1] -> Y, with
    a = ef - 64.  The reference expands E, then G -- the list is now full: H, the A's, G and the nearest F's --, then H: its 64
    neighbours are all admitted and push out the 64 worst, A[a-1] among them.  It then expands the N's and A0..A[a-2] and STOPS
    at A[a-1], which is strictly beyond the worst: Y is never evaluated.  ef 80: 146 evaluations, 82 expansions.

    ef >= 128: G's 64 slots cannot hold ef - 64 A's, so a chain of m = ceil((ef - 64) / 64) hubs C1..Cm NEARER than the A's
    (each is expanded as soon as it is found) hands out a = ef - 64 - m A's and the 63 F's, 63 to a node, and the last hub
    holds H: again the list is exactly full when H is expanded, 64 entries leave, A[a-1] is the nearest of them.

    kind "tie": A[a-1] ties A[a-2] bit for bit -- the reference's <= DOES expand it, and Y is found.
    kind "tie-many": every A and every F has one value: 64 entries leave `nearest` and every one of them ties its worst (more
    than the ghost slots of any kernel hold: the repeat pass), the reference expands them all.
    kind "split": (ef 80) H's neighbours in slot order: 10 between the F's (admitted, they push out F61..F52), 10 that tie the
    worst the list has by then and 20 beyond it but below the worst the expansion found (survivors that are refused), then 24
    near ones that push out, among others, the first 10 again (admitted, then evicted).
    kind "small": the graph of ef 80 for lists SHORTER than the fan-out (ef 1, 10, 64); H holds the N's farthest first, so each
    of the 64 is nearer than everything before it and is admitted, whatever the list's length."""
    names, values = [], []

    def node(name, value):
        names.append(name)
        values.append(value)
        return len(names) - 1

    assert ef >= 65 and kind in ("plain", "tie", "tie-many", "split", "small") and (kind not in ("split", "small") or ef == 80)
    m = 0 if ef < 128 else -(-(ef - 64) // 64)
    a = ef - 64 - m
    fstep = 2 if kind == "split" else 1
    E = node("E", V_E)
    hubs = [node("C%d" % (i + 1), V_HUB - i) for i in range(m)] if m else [node("G", V_G)]
    one = kind == "tie-many"
    A = [node("A%d" % i, V_A if one else V_A + i) for i in range(a)]
    F = [node("F%d" % i, V_A if one else V_F + fstep * i) for i in range(63)]
    if kind == "tie" and a >= 2:
        values[A[-1]] = values[A[-2]]
    H = node("H", V_H)
    Y = node("Y", V_Y)
    if kind == "split":
        worst_then = V_F + fstep * 51                       # F51: the worst once the first ten have pushed out F61..F52
        nv = [V_F + fstep * (41 + i) + 1 for i in range(10)]            # between F41 and F51, one between each pair
        nv += [worst_then] * 10
        nv += [worst_then + 1 + i % 18 for i in range(20)]              # < F61, the worst the expansion finds
        nv += [V_N + i for i in range(24)]
    else:
        nv = [V_N + i for i in range(64)][::-1 if kind == "small" else 1]
    N = [node("N%d" % i, v) for i, v in enumerate(nv)]
    l0 = np.full((len(names), M0), -1, np.int32)
    if m == 0:
        l0[E, :64] = F + hubs
        l0[hubs[0], :a + 1] = A + [H]
    else:
        pool = A + F
        owners = [E] + hubs
        for i, o in enumerate(owners):
            part = pool[63 * i:63 * (i + 1)]
            l0[o, :len(part)] = part
            l0[o, 63] = hubs[i] if i < m else H
    l0[H, :64] = N
    l0[A[-1], 0] = Y
    roles = {"E": E, "H": H, "Y": Y, "last_A": A[-1], "A": A, "F": F, "N": N, "hubs": hubs}
    name = "S-%s-ef%d" % (kind, ef)
    efs = (1, 10, 64) if kind == "small" else (ef,)
    return Case(name, np.array(values, np.int64), np.ones(len(values), np.int64), l0, E, efs, roles)


def scenarios():
    """Every scripted scenario: (case, what its event log must show) -- see test_scripted_graph_traces.py."""
    out = [(scenario_s(ef), "full") for ef in (65, 80, 128, 640)]
    out += [(scenario_s(80, "tie"), "tie"), (scenario_s(128, "tie"), "tie"), (scenario_s(128, "tie-many"), "tie-many")]
    out += [(scenario_s(80, "split"), "split")]
    out += [(scenario_s(80, "small"), "small")]
    return out


# ---- funnel graphs --------------------------------------------------------------------------------------------------------
def funnel(seed, n=640, rewire=0.0, tie=0.0):
    """Shells of 64 nodes, farthest first; every node's 64 slots hold the NEXT shell in shuffled order, so the first expansion
    into a shell finds 64 fresh neighbours that are all nearer than the whole list; each slot is re-pointed at a random node
    with probability `rewire`; a fraction `tie` of the nodes duplicates another node's value; the last shell has 8 random
    edges per node; the entry is the farthest node; row signs and node numbers are random."""
    rs = np.random.RandomState(seed)
    values = rs.choice(np.arange(1, 4000), n, replace=False)
    ntie = int(tie * n)
    if ntie:
        dup = rs.choice(n, ntie, replace=False)
        keep = np.setdiff1d(np.arange(n), dup)
        values[dup] = values[rs.choice(keep, ntie)]
    perm = rs.permutation(n)                                # position in the farthest-first order -> node number
    order = np.argsort(-values, kind="stable")
    values = values[order]                                  # farthest first
    l0 = np.full((n, M0), -1, np.int32)
    nshell = (n + 63) // 64
    for s in range(nshell):
        lo, hi = 64 * s, min(64 * (s + 1), n)
        nxt = np.arange(64 * (s + 1), min(64 * (s + 2), n))
        for p in range(lo, hi):
            if len(nxt):
                row = rs.permutation(nxt)
                l0[perm[p], :len(row)] = perm[row]
                hit = np.flatnonzero(rs.random_sample(len(row)) < rewire)
                l0[perm[p], hit] = rs.randint(0, n, len(hit))
            else:
                l0[perm[p], :8] = rs.randint(0, n, 8)
    out_values = np.empty(n, np.int64)
    out_values[perm] = values
    signs = rs.choice([-1, 1], n)
    return Case("funnel-%d" % seed, out_values, signs, l0, int(perm[0]), FUNNEL_EFS, {})


FUNNEL_SEEDS = tuple(range(24))
FUNNEL_EFS = (10, 64, 65, 80, 128, 333)


def funnel_case(seed):
    """The funnel graphs of the GPU module: (case, metric, dim) -- both rewire rates, three tie rates, every metric, both dims."""
    case = funnel(seed, 640, (0.0, 0.02)[seed % 2], (0.0, 0.3, 0.6)[seed % 3])
    return case, METRICS[(seed // 6 + seed) % 3], DIMS[(seed // 3) % 2]


# ---- the reference, with a log -------------------------------------------------------------------------------------------
def trace(dist, l0, entry, ef, k=None):
    """search-layer-ultra (ultra_fast.clj:151-212) on layer 0 from `entry`, as oracle.c states it: candidates leave a queue
    nearest first (ties: admission order), a candidate is expanded iff `nearest` is not full or it is <= its worst (:175-178),
    a fresh neighbour is admitted iff `nearest` is not full or it is < its worst (:195-198), and then the worst leaves a
    `nearest` of ef + 1 (:203-204; ties: the latest admission).  dist: the query's distance to every node."""
    seq = 0
    nearest = [(float(dist[entry]), seq, int(entry))]      # ascending (distance, admission number)
    cand = list(nearest)
    visited = {int(entry)}
    evals, hops, events, stop = 1, 0, [], None
    left = collections.Counter()                            # distance -> entries that have left `nearest`
    while cand:
        d, _, node = cand.pop(0)
        full = len(nearest) >= ef
        worst0 = nearest[-1][0]
        if full and not d <= worst0:
            stop = (node, d, worst0)
            break
        hops += 1
        before = {e[2] for e in nearest}
        on_tie = full and d == worst0 and node not in before
        n_fresh = n_surv = n_adm = 0
        admitted, evicted = set(), []
        for nb in l0[node]:
            nb = int(nb)
            if nb < 0 or nb in visited:
                continue
            visited.add(nb)
            evals += 1
            n_fresh += 1
            dn = float(dist[nb])
            n_surv += 1 if (not full or dn < worst0) else 0
            if len(nearest) < ef or dn < nearest[-1][0]:
                seq += 1
                bisect.insort(nearest, (dn, seq, nb))
                bisect.insort(cand, (dn, seq, nb))
                admitted.add(nb)
                n_adm += 1
                if len(nearest) > ef:
                    evicted.append(nearest.pop())
        n_old = sum(1 for e in evicted if e[2] in before)
        btie = n_adm >= 2 and bool(evicted) and min(e[0] for e in evicted) == nearest[-1][0]
        left.update(e[0] for e in evicted)
        worst = nearest[-1][0] if len(nearest) >= ef else None
        events.append(Event(node, full, n_fresh, n_surv, n_adm, n_old, len(evicted) - n_old, on_tie, btie, worst,
                            left[worst] if worst is not None else 0))
    k = min(ef, len(nearest)) if k is None else k
    ids = [e[2] for e in nearest[:k]] + [-1] * max(0, k - len(nearest))
    return Trace(np.array(ids, np.int32), evals, hops, events, stop, frozenset(visited))


def is_full_fanout(e):
    """64 fresh neighbours on a full list, all admitted, 64 older entries pushed out."""
    return e.list_full and e.n_fresh == 64 and e.n_admitted == 64 and e.n_evicted_old == 64


def result_k(ef):
    return min(ef, 100)      # the list's CONTENT is compared, not just its ten nearest
