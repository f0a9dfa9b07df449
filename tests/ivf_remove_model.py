"""numpy statement of what hnswgpu_ivf_remove leaves of the lists, independent of the library: every list without its removed
members, the kept members in their order under their new ids, the offsets lowered by the removed members of the lists below.
Built on lsh_remove_model.kept / rank (which rows remain, a kept row's new id)."""
import numpy as np

from lsh_remove_model import kept, rank  # noqa: F401  (kept: re-exported for the tests)


def compact_lists(off, ids, rows):
    """Lists (off [nlist + 1], ids [n0]) after `rows` (row ids, any order, repeats count once) left -> (off1 int64 [nlist + 1],
    ids1 int32 [n1]).  Dropped entries close up; nothing else moves."""
    off = np.asarray(off, np.int64)
    ids = np.asarray(ids, np.int64)
    new_id = rank(len(ids), rows)
    stays = new_id[ids] >= 0                                 # per list position
    gone_before = np.concatenate([[0], np.cumsum(~stays)])   # removed entries before every position
    return off - gone_before[off], new_id[ids][stays].astype(np.int32)
