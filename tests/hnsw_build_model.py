"""What the batched-build tests share (test_hnsw_build_model_host.py, test_hnsw_build_batched_gpu.py,
test_hnsw_heuristic_paths_gpu.py): the engine's batch-size rule restated, the edge-for-edge comparison, and the data sets
with the conditions each must meet -- checked from the model's counters on the CPU, relied on by the GPU tests.

The model itself is oracle.c's orc_hnsw_build_batched (oracle.hnsw_build_batched)."""
import numpy as np

DEFAULT_MAX_BATCH = 16384        # hnsw.hip: insert_batches, the default (and the cap) of HNSWGPU_TUNE_BUILD_BATCH

# counters of oracle.hnsw_build_batched
TASKS, TASKS_2_PENDING, SYM_REMOVED, ABOVE_TOP, ENTRY_CHANGES, ENTRY_CHANGES_IN_BATCH, MOST_TASKS_IN_BATCH, \
    ADOPTED_FIRST, ADOPTED_UNSORTED = range(9)


def batch_schedule(n, start, max_batch=DEFAULT_MAX_BATCH):
    """Batch sizes of insert_batches over rows [start, n): with `done` rows in the graph the next batch holds
    min(max_batch, max(1, done // 8), 2048 + done // 64, n - done) rows.  A build starts at 1 (row 0 is the entry point),
    hnswgpu_hnsw_add at the rows the index holds."""
    max_batch = max(1, min(DEFAULT_MAX_BATCH, int(max_batch)))
    out, done = [], int(start)
    while done < n:
        b = min(max_batch, max(1, done // 8), 2048 + done // 64, n - done)
        out.append(b)
        done += b
    return out


def same_graph(g, og, what):
    """Edge for edge: levels, entry point, top, up_off and both adjacency arrays, every row in its order."""
    np.testing.assert_array_equal(g.levels, og.levels, err_msg=what + ": levels")
    assert (g.entry, g.max_level, g.M, g.M0) == (og.entry, og.max_level, og.M, og.M0), \
        "%s: entry / top / M / M0 %s, expected %s" % (what, (g.entry, g.max_level, g.M, g.M0), (og.entry, og.max_level, og.M, og.M0))
    np.testing.assert_array_equal(g.up_off, og.up_off, err_msg=what + ": up_off")
    n = len(og.levels)
    a, b = g.l0_adj.reshape(n, -1), og.l0_adj.reshape(n, -1)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert bad.size == 0, "%s: %d layer-0 rows differ, first at node %d: got %s expected %s" % (
        what, bad.size, bad[0], a[bad[0]], b[bad[0]])
    a, b = g.up_adj.reshape(-1, og.M), og.up_adj.reshape(-1, og.M)
    bad = np.nonzero((a != b).any(axis=1))[0]
    if bad.size:
        node = int(np.searchsorted(og.up_off, bad[0], side="right") - 1)
        raise AssertionError("%s: %d upper-layer lists differ, first at node %d layer %d: got %s expected %s" % (
            what, bad.size, node, bad[0] - og.up_off[node] + 1, a[bad[0]], b[bad[0]]))


def flag_bits(O, name):
    """'closest', 'heuristic', 'heuristic+symmetric', 'heuristic+extend' -> the oracle's BUILD_* bits."""
    return (O.BUILD_HEURISTIC if "heuristic" in name else 0) | (O.BUILD_SYMMETRIC if "symmetric" in name else 0) | \
           (O.BUILD_EXTEND if "extend" in name else 0)


def flag_kwargs(name):
    """... -> the keyword arguments of engine.Index.hnsw_build."""
    return dict(heuristic="heuristic" in name, symmetric="symmetric" in name, extend="extend" in name)


def clustered(O, n, dim, clusters, noise, seed, pairs=6, zero=True):
    """Clustered rows with `pairs` duplicated pairs and one zero row: at most 2 rows equal any one row, so a build search
    (which has no repeat pass) never runs out of ghost slots for candidates tied with its ef-th."""
    base = O.generate_dataset(n, dim, "clustered", num_clusters=clusters, noise_level=noise, seed=seed).astype(np.float32)
    for p in range(pairs):
        src = (37 + 101 * p) % (n // 2)
        dst = n // 2 + (53 + 211 * p) % (n - n // 2)
        base[dst] = base[src]
    if zero:
        base[(2 * n) // 3 + 1] = 0.0
    return base


# ---- the main sweep: n = 3000, dim 48, M 8, efc 40
MAIN = dict(n=3000, dim=48, M=8, efc=40, seed=42)
MAIN_FLAGS = ["closest", "heuristic", "heuristic+symmetric", "heuristic+extend"]
MAIN_BATCHES = [1, 7, 64, DEFAULT_MAX_BATCH]


def main_data(O):
    return clustered(O, MAIN["n"], MAIN["dim"], clusters=12, noise=0.4, seed=7)


# ---- the large case: n = 24,000, dim 16, M 8, efc 32
LARGE = dict(n=24000, dim=16, M=8, efc=32, seed=42)


def large_data(O):
    return clustered(O, LARGE["n"], LARGE["dim"], clusters=24, noise=1.0, seed=11)


# ---- hnsw_add: 2000 rows built, then calls of 1, 1, 5, 300 and 693 rows
# (M = 5: upper-layer lists of five fill without ever overflowing during 2000 sequential inserts -- full, in insertion order)
ADD = dict(n0=2000, calls=[1, 1, 5, 300, 693], M=5, efc=40, seed=42)
ADD_CASES = [(48, "cosine"), (48, "l2"), (1100, "cosine"), (1100, "l2")]


def add_data(O, dim):
    n = ADD["n0"] + sum(ADD["calls"])
    if dim <= 64:
        return clustered(O, n, dim, clusters=10, noise=0.4, seed=19)
    # long rows: a few informative dimensions in front, small noise behind, so that the searches of a dim-1100 model stay short
    base = np.zeros((n, dim), np.float32)
    base[:, :32] = clustered(O, n, 32, clusters=10, noise=0.4, seed=23)
    base[:, 32:] = 0.02 * O.generate_dataset(n, dim - 32, "gaussian", seed=29).astype(np.float32)
    base[n // 2 + 7] = base[11]
    return base


# ---- the selection kernel's paths: n = 600, efc 48, 20 duplicated pairs
PATHS = dict(n=600, efc=48, seed=42)
PATH_CASES = [(40, 16), (40, 20), (300, 8), (700, 8), (1000, 8), (1100, 8), (1536, 8), (1700, 8), (2500, 6)]   # (dim, M)
PATH_EXTEND = [(40, 16), (1100, 8)]


def paths_data(O, dim):
    """10 clusters of 60 rows, each cluster's centre itself a row (rows 30 .. 39).  Seen from its centre a cluster's rows
    are farther from each other than from the centre (noise * sqrt(2 dim) against noise * sqrt(dim)), so the heuristic
    keeps every one of them: the centres' lists fill to 2M -- the selection takes up to 2M rows -- and overflow, which the
    plain clustered rows of the other tests do not do at M >= 16."""
    n, k = PATHS["n"], 10
    rs = np.random.RandomState(100 + dim)
    centres = rs.randn(k, dim)
    base = centres[np.arange(n) % k] + 0.4 * rs.randn(n, dim)
    base[3 * k:4 * k] = centres
    base = base.astype(np.float32)
    base[300:320] = base[100:120]        # 20 duplicated pairs: runs of equal distances reach the selection in id order
    return base
