"""numpy statement of what hnswgpu_lsh_update leaves of the base and the tables, independent of the library.  A row whose code in a
table is unchanged keeps its bucket there; a row whose code changed leaves its bucket, which closes up, and joins the new one at
the place its row id gives it among the members.  An update changes no id and a bucket is ascending by row id, so the result is
the counting sort of the new codes -- `merge` states the rule one row at a time and the host tests hold it against `tables`."""
import numpy as np

import lsh_model as M


def apply(base, ids, rows):
    """The base with rows[i] in place of row ids[i] (a copy)."""
    out = np.array(base, np.float32, copy=True)
    ids = np.asarray(ids, np.int64).reshape(-1)
    rows = np.asarray(rows, np.float32).reshape(len(ids), -1)
    assert len(np.unique(ids)) == len(ids), "an id named twice has no winner"
    out[ids] = rows
    return out


def tables(codes, bits):
    """(off (T, 2^bits + 1), ids (T, n)) of the codes: lsh_model.buckets, the stable counting sort."""
    return M.buckets(codes, bits)


def merge(codes, off, ids, rows, new_codes):
    """(codes, off, ids) after rows[i] took the codes new_codes[i], one row and one table at a time: a stayer is not touched, a mover
    is cut out of its bucket and inserted into the new one before the first member with a larger id."""
    codes = np.array(codes, np.uint16, copy=True)
    T = codes.shape[1]
    lists = [[list(ids[t, off[t, b]:off[t, b + 1]]) for b in range(off.shape[1] - 1)] for t in range(T)]
    for r, now in zip(np.asarray(rows, np.int64).reshape(-1), np.asarray(new_codes, np.uint16).reshape(-1, T)):
        for t in range(T):
            was, to = int(codes[r, t]), int(now[t])
            if was == to:
                continue
            lists[t][was].remove(r)
            into = lists[t][to]
            into.insert(int(np.searchsorted(np.asarray(into, np.int64), r)), r)
            codes[r, t] = to
    new_off = np.zeros_like(off)
    new_ids = np.zeros_like(ids)
    for t in range(T):
        new_off[t, 1:] = np.cumsum([len(b) for b in lists[t]])
        flat = [r for b in lists[t] for r in b]
        new_ids[t] = flat
    return codes, new_off, new_ids
