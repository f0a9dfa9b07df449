"""The numpy model of "merged lists" the ivf_add tests expect (include/hnswgpu.h: hnswgpu_ivf_add): every list keeps its old
members in their old order and receives its new members behind them, ascending by row id."""
import numpy as np


def merged_lists(list_off, list_ids, assign_new):
    """Old lists (list_off [nlist + 1], list_ids [n0]) + the list of every new row (assign_new[i]: row n0 + i) -> the grown
    (list_off int64 [nlist + 1], list_ids int32 [n0 + m])."""
    off = np.asarray(list_off, np.int64)
    ids = np.asarray(list_ids, np.int32)
    a = np.asarray(assign_new, np.int64)
    nlist, n0 = len(off) - 1, len(ids)
    assert off[0] == 0 and off[-1] == n0 and (len(a) == 0 or (a.min() >= 0 and a.max() < nlist))
    parts = []
    for l in range(nlist):
        parts.append(ids[off[l]:off[l + 1]])
        parts.append((n0 + np.flatnonzero(a == l)).astype(np.int32))     # flatnonzero ascends: row order
    new_off = np.zeros(nlist + 1, np.int64)
    new_off[1:] = np.cumsum(np.diff(off) + np.bincount(a, minlength=nlist))
    return new_off, (np.concatenate(parts) if parts else np.zeros(0, np.int32)).astype(np.int32)


def f64_distances(metric, rows, centroids):
    """[m, nlist] distances in f64: cosine 1 - cos, l2 rooted, dot negated."""
    x, c = np.asarray(rows, np.float64), np.asarray(centroids, np.float64)
    if metric == "l2":
        return np.sqrt(np.maximum(((x[:, None, :] - c[None, :, :]) ** 2).sum(-1), 0.0))
    dots = x @ c.T
    if metric == "dot":
        return -dots
    return 1.0 - dots / (np.linalg.norm(x, axis=1)[:, None] * np.linalg.norm(c, axis=1)[None, :])
