"""numpy statement of what hnswgpu_lsh_remove leaves, independent of the library: which rows are kept, a kept row's new id, and
the lsh_get arrays after a removal -- computed by dropping entries and renumbering, never by sorting the codes again (that is
lsh_model.buckets, the other yardstick: the two have to agree)."""
import numpy as np


def kept(n, rows):
    """The old ids of the rows that remain, ascending (int64): the row numbered i afterwards was kept(n, rows)[i].  `rows` may
    repeat and come in any order."""
    keep = np.ones(n, np.bool_)
    keep[np.asarray(rows, np.int64).reshape(-1)] = False
    return np.flatnonzero(keep).astype(np.int64)


def rank(n, rows):
    """new id per old row (int64 [n]); -1 for a removed row.  The new id of a kept row is the number of kept rows below it."""
    k = kept(n, rows)
    out = np.full(n, -1, np.int64)
    out[k] = np.arange(len(k))
    return out


def compact(codes, off, ids, rows):
    """(codes, off, ids) of lsh_get after `rows` left: codes of the kept rows; per table every bucket without its removed
    members, in their order, renumbered; the offsets lowered by the removed members of the buckets below."""
    codes, off, ids = np.asarray(codes), np.asarray(off), np.asarray(ids)
    n, T = codes.shape
    new_id = rank(n, rows)
    k = kept(n, rows)
    new_off = np.zeros_like(off)
    new_ids = np.zeros((T, len(k)), np.int32)
    for t in range(T):
        stays = new_id[ids[t]] >= 0                       # per position of the table's ids
        new_ids[t] = new_id[ids[t]][stays]                # dropped entries close up; nothing else moves
        gone_before = np.concatenate([[0], np.cumsum(~stays)])   # removed entries before every position
        new_off[t] = off[t] - gone_before[off[t]]
    return codes[k], new_off, new_ids
