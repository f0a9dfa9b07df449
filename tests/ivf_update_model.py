"""numpy statement of what hnswgpu_ivf_update leaves of the lists, independent of the library.  A row whose new nearest list is the
list it sits in keeps its list position; a row whose new nearest list is another one leaves its old list, which closes up, and
joins the new one behind the members that remain there, ascending by row id among the call's movers:

    new list l = (old members of l in their old order, without the movers that left) ++ (the call's movers into l, ascending by id)

The order in which the call names its rows does not matter; two calls are the rule applied twice."""
import numpy as np


def updated_lists(off, ids, rows, assign):
    """Lists (off [nlist + 1], ids [n]) after the rows `rows` (distinct row ids, any order) were assigned to the lists `assign`
    (assign[i] is the new nearest list of rows[i]) -> (off1 int64 [nlist + 1], ids1 int32 [n])."""
    off = np.asarray(off, np.int64)
    ids = np.asarray(ids, np.int64)
    rows = np.asarray(rows, np.int64).reshape(-1)
    assign = np.asarray(assign, np.int64).reshape(-1)
    n, nlist = len(ids), len(off) - 1
    assert len(rows) == len(assign) and len(np.unique(rows)) == len(rows), "one list per row, every row named once"
    assert len(rows) == 0 or (rows.min() >= 0 and rows.max() < n and assign.min() >= 0 and assign.max() < nlist)
    list_of_pos = np.repeat(np.arange(nlist), np.diff(off))   # the list of every old position
    new_list = np.full(n, -1, np.int64)                       # per row: its new nearest list, -1 = not updated
    new_list[rows] = assign
    leaves = (new_list[ids] >= 0) & (new_list[ids] != list_of_pos)   # per old position
    movers = np.sort(ids[leaves])                             # ascending by row id
    to = new_list[movers]
    out = [np.concatenate([ids[off[l]:off[l + 1]][~leaves[off[l]:off[l + 1]]], movers[to == l]]) for l in range(nlist)]
    off1 = np.zeros(nlist + 1, np.int64)
    off1[1:] = np.cumsum([len(x) for x in out])
    ids1 = np.concatenate(out).astype(np.int32) if n else np.zeros(0, np.int32)
    return off1, ids1
