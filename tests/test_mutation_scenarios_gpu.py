"""The observers of mutation_checks.py on the intricate scenarios the per-operation tests already have -- IVF alias handles, lists
that empty and lists that receive their first rows, to-nothing-and-back, the interleaved add / remove / update sequences -- at
dim 136 and rejection mode 2 (every compact copy exists).  Each scenario is rebuilt here from the helpers of the file it comes
from; those files compare searches and saved files, this one the copies no search at test size reads: the base-order int8 rows
(distance_bounds / rejection_bounds / hnsw_rejection_bounds), the list-order half rows (ivf_half_bounds), the list-order int8
tiles (the counters of searches forced through the bounds pass), and exact_knn against a float64 brute force.  Every handle makes
its lazily made copies BEFORE the mutation (mutation_checks.touch): a chain remakes only what the handle holds."""
import numpy as np
import pytest

import hnsw_build_model as H
import hnsw_remove_model as HR
import ivf_remove_model as IR
import ivf_update_model as IU
import mutation_checks as C
import test_hnsw_remove_gpu as THR
import test_ivf_add_gpu as TIA
import test_ivf_remove_gpu as TIR
import test_ivf_update_gpu as TIU
import test_lsh_remove_gpu as TLR
from ivf_add_model import f64_distances, merged_lists

pytestmark = pytest.mark.gpu

DIM, MODE = 136, 2


def _ivf_handle(engine, rows, metric, cen, off, ids, Q):
    """A mode-2 handle over installed lists whose every copy exists."""
    ix = TIU._fresh(engine, rows, metric, MODE, cen, off, ids)
    C.touch(ix, Q)
    return ix


def _ivf_checks(ix, fresh, Q, rows, metric):
    row = rows[len(rows) // 2] if len(rows) else None
    C.same_base_codes(ix, fresh, Q, row, expect=True)
    C.same_list_half(ix, fresh, Q, row, expect=True)
    C.same_list_tiles(ix, fresh, Q, expect=True)
    C.matches_f64(ix, rows, metric, Q)


def _alias_base(engine, oracle, mod):
    """The base of the alias tests: `mod`'s rows in the order of their built lists, so that list_ids is the identity."""
    rows, Q = mod._data(oracle, DIM)
    n0 = mod.N0
    with engine.Index(rows[:n0], "cosine", 0) as b:
        b.ivf_build(mod.NLIST, 3, 42)
        cen, off0, ids_b = b.get_ivf()
    return rows, Q, np.ascontiguousarray(rows[:n0][ids_b]), cen, off0, np.arange(n0, dtype=np.int32)


def _tail(cen, off0, seed=4):
    """40 rows that all belong into the last list with members: added to an alias handle they keep list_ids the identity."""
    last = int(np.flatnonzero(np.diff(off0) > 0)[-1])
    rng = np.random.default_rng(seed)
    return (cen[last][None, :] * (1.0 + 0.001 * rng.standard_normal((40, cen.shape[1])))).astype(np.float32)


# ---- IVF: alias handles -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["scatter", "last_list"])
def test_ivf_add_alias_handle(native_lib, oracle, tune, case):
    from hnsw_clj_amd import engine

    rows, Q, base, cen, off0, ident = _alias_base(engine, oracle, TIA)
    new = rows[TIA.N0:] if case == "scatter" else _tail(cen, off0)
    everything = np.concatenate([base, new])
    assign = TIA._device_assign(engine, tune, everything, "cosine", cen)[TIA.N0:]
    TIA._check_f64_guard("cosine", new, cen, assign)
    off, ids = merged_lists(off0, ident, assign)
    assert (ids == np.arange(len(ids))).all() == (case == "last_list")
    with _ivf_handle(engine, base, "cosine", cen, off0, ident, Q) as ix:
        ix.ivf_add(new[:17])
        ix.ivf_add(new[17:])
        TIA._assert_same_ivf(ix, cen, off, ids)
        with TIU._fresh(engine, everything, "cosine", MODE, cen, off, ids) as fresh:
            _ivf_checks(ix, fresh, Q, everything, "cosine")


def test_ivf_remove_alias_handle_then_add(native_lib, oracle, tune):
    from hnsw_clj_amd import engine

    rows, Q, base, cen, off0, ident = _alias_base(engine, oracle, TIR)
    gone = np.random.default_rng(4).choice(TIR.N0, 333, replace=False)
    for new, stays_identity in ((rows[TIR.N0:], False), (_tail(cen, off0), True)):
        with _ivf_handle(engine, base, "cosine", cen, off0, ident, Q) as ix:
            kept = TIR._remove(ix, gone)
            off, ids = IR.compact_lists(off0, ident, gone)
            TIR._assert_same_ivf(ix, cen, off, ids, "alias")
            with TIU._fresh(engine, base[kept], "cosine", MODE, cen, off, ids) as fresh:
                _ivf_checks(ix, fresh, Q, base[kept], "cosine")
            everything = np.concatenate([base[kept], new])
            assign = TIR._device_assign(engine, tune, everything, "cosine", cen)[len(kept):]
            off2, ids2 = merged_lists(off, ids, assign)
            assert (ids2 == np.arange(len(ids2))).all() == stays_identity
            ix.ivf_add(new[:17])
            ix.ivf_add(new[17:])
            TIR._assert_same_ivf(ix, cen, off2, ids2, "alias, grown")
            with TIU._fresh(engine, everything, "cosine", MODE, cen, off2, ids2) as fresh:
                _ivf_checks(ix, fresh, Q, everything, "cosine")


@pytest.mark.parametrize("case", ["stayers", "mover", "mover_identity"])
def test_ivf_update_alias_handle(native_lib, oracle, tune, case):
    from hnsw_clj_amd import engine

    if case == "mover_identity":                             # the last row moves into the empty last list: still the identity
        rng, cen, b0, off0, order, a0 = TIU._edge_base(dim=DIM)
        base = np.ascontiguousarray(b0[order])
        n, metric, Q = len(base), "l2", base[:64]
        at, to = np.array([n - 1], np.int32), np.array([3])
        new = TIU._near(rng, cen, to)
        ident = np.arange(n, dtype=np.int32)
    else:
        rows, Q, base, cen, off0, ident = _alias_base(engine, oracle, TIU)
        n, metric = TIU.N0, "cosine"
        spare = rows[TIU.N0:]
        assign = TIU._device_assign(engine, tune, spare, metric, cen)
        where = np.repeat(np.arange(TIU.NLIST), np.diff(off0))
        if case == "stayers":                                # 100 values, each for a row of the list it belongs into
            sp, taken, at = np.arange(100), set(), []
            for j in sp:
                r = next(int(r) for r in np.flatnonzero(where == assign[j]) if int(r) not in taken)
                taken.add(r)
                at.append(r)
            at = np.array(at, np.int32)
        else:                                                # 100 values, half for rows of their list and half for rows of another
            at, sp, moves = TIU._Pairing(43, assign).batch(where, 100)
            TIU._assert_mixed(moves)
        new, to = spare[sp], assign[sp]
    off, ids = IU.updated_lists(off0, ident, at, to)
    assert np.array_equal(ids, ident) == (case != "mover")
    cur = base.copy()
    cur[at] = new
    with _ivf_handle(engine, base, metric, cen, off0, ident, Q) as ix:
        ix.ivf_update(at, new)
        TIU._assert_same_ivf(ix, cen, off, ids, case)
        with TIU._fresh(engine, cur, metric, MODE, cen, off, ids) as fresh:
            _ivf_checks(ix, fresh, Q, cur, metric)
            ix.ivf_update(at, new)                           # ... and once more: everybody stays now, whatever the handle became
            TIU._assert_same_ivf(ix, cen, off, ids, case + ", again")
            _ivf_checks(ix, fresh, Q, cur, metric)


# ---- IVF: lists that empty, lists that receive their first rows -----------------------------------------------------------------
def test_ivf_add_an_empty_list_receives_its_first_rows(native_lib):
    from hnsw_clj_amd import engine

    cen, base, off0, ids0 = TIA._edge_base(dim=DIM)
    rng = np.random.default_rng(11)
    a = np.array([3, 0] * 32 + [3], np.int64)               # 65 rows, alternating between the empty list 3 and list 0
    new = (cen[a] + 0.1 * rng.standard_normal((len(a), DIM))).astype(np.float32)
    assert (f64_distances("l2", new, cen).argmin(axis=1) == a).all()
    off, ids = merged_lists(off0, ids0, a)
    assert off[4] - off[3] == 33 and off[3] == off[2]
    everything = np.concatenate([base, new])
    with _ivf_handle(engine, base, "l2", cen, off0, ids0, base[:64]) as ix:
        ix.ivf_add(new)
        TIA._assert_same_ivf(ix, cen, off, ids)
        with TIU._fresh(engine, everything, "l2", MODE, cen, off, ids) as fresh:
            _ivf_checks(ix, fresh, everything[-64:], everything, "l2")


@pytest.mark.parametrize("case", ["list0", "list1"])
def test_ivf_remove_a_list_empties(native_lib, case):
    from hnsw_clj_amd import engine

    cen, base, off0, ids0, _ = TIR._edge_base(dim=DIM)
    gone = ids0[off0[0]:off0[1]][::-1] if case == "list0" else ids0[off0[1]:off0[2]]
    off, ids = IR.compact_lists(off0, ids0, gone)
    with _ivf_handle(engine, base, "l2", cen, off0, ids0, base[:64]) as ix:
        kept = TIR._remove(ix, gone)
        TIR._assert_same_ivf(ix, cen, off, ids, case)
        assert 0 < len(kept) and (off[0] == off[1] if case == "list0" else off[1] == off[2])
        with TIU._fresh(engine, base[kept], "l2", MODE, cen, off, ids) as fresh:
            _ivf_checks(ix, fresh, base[kept][:64], base[kept], "l2")


@pytest.mark.parametrize("case", ["list_emptied", "first_members"])
def test_ivf_update_lists_empty_and_fill(native_lib, case):
    from hnsw_clj_amd import engine

    rng, cen, base, off0, ids0, a0 = TIU._edge_base(dim=DIM)
    n = len(base)
    if case == "list_emptied":                               # every member of list 0 leaves, in descending order of position
        at = ids0[off0[0]:off0[1]][::-1].copy()
        to = np.full(len(at), 1)
    else:                                                    # 65 rows, alternating between the empty list 3 and their own list
        at = rng.permutation(n)[:65].astype(np.int32)
        to = np.where(np.arange(65) % 2 == 0, 3, a0[at])
    new = TIU._near(rng, cen, to)
    off, ids = IU.updated_lists(off0, ids0, at, to)
    assert (off[0] == off[1] == 0) if case == "list_emptied" else (off[4] - off[3] == 33)
    cur = base.copy()
    cur[at] = new
    with _ivf_handle(engine, base, "l2", cen, off0, ids0, base[:64]) as ix:
        ix.ivf_update(at, new)
        TIU._assert_same_ivf(ix, cen, off, ids, case)
        with TIU._fresh(engine, cur, "l2", MODE, cen, off, ids) as fresh:
            _ivf_checks(ix, fresh, cur[:64], cur, "l2")


# ---- to nothing and back --------------------------------------------------------------------------------------------------------
def test_ivf_to_nothing_and_back(native_lib):
    from hnsw_clj_amd import engine

    cen, base, off0, ids0, a0 = TIR._edge_base(dim=DIM)
    n, Q = len(base), base[:64]
    with _ivf_handle(engine, base, "l2", cen, off0, ids0, Q) as ix:
        kept = TIR._remove(ix, np.random.default_rng(34).permutation(n))
        assert len(kept) == 0 and ix.n == 0 and ix.nlist == 4
        none = np.zeros((0, DIM), np.float32)
        with TIU._fresh(engine, none, "l2", MODE, cen, np.zeros(5, np.int64), np.zeros(0, np.int32)) as empty:
            _ivf_checks(ix, empty, Q, none, "l2")            # the bounds entries refuse alike, the forced searches answer empty alike
            one = np.zeros(1, np.int32)
            for call in (lambda h: h.distance_bounds(Q[0], one), lambda h: h.ivf_half_bounds(Q[0], one)):
                m, f = C._outcome(lambda: call(ix)), C._outcome(lambda: call(empty))
                assert m[0] == f[0] == "refused" and m[1] == f[1], (m, f)
        ix.ivf_add(base)                                     # ... and grown again
        off, ids = merged_lists(np.zeros(5, np.int64), np.zeros(0, np.int32), a0)
        TIR._assert_same_ivf(ix, cen, off, ids, "grown again from nothing")
        with TIU._fresh(engine, base, "l2", MODE, cen, off, ids) as fresh:
            _ivf_checks(ix, fresh, Q, base, "l2")


def test_lsh_to_nothing_and_back(native_lib):
    from hnsw_clj_amd import engine

    rows, Q = TLR._data(DIM)
    base = rows[:300]
    with engine.Index(base, "cosine", 0) as ix:
        ix.set_rejection_test(MODE)
        ix.lsh_build(8, 6, 64, 42)
        planes = ix.lsh_get()[0]
        C.touch(ix, Q)
        kept = TLR._remove(ix, np.random.default_rng(16).permutation(300))
        assert len(kept) == 0 and ix.n == 0
        with TLR._fresh(engine, np.zeros((0, DIM), np.float32), "cosine", planes, MODE) as empty:
            C.same_base_codes(ix, empty, Q)
        ix.lsh_add(base)
        with TLR._fresh(engine, base, "cosine", planes, MODE) as fresh:
            TLR._assert_same_tables(ix, fresh, "grown again from nothing")
            C.same_base_codes(ix, fresh, Q, base[150], expect=True)
            C.matches_f64(ix, base, "cosine", Q)


def test_hnsw_to_nothing_and_back(native_lib, oracle):
    from hnsw_clj_amd import engine

    O = oracle
    rows, Q = THR._rows(O, DIM)
    base, again = rows[:THR.N0], rows[THR.N0:THR.N0 + 300]
    with THR._built(engine, base, "l2", True, MODE) as ix:
        C.touch(ix, Q)
        kept = THR._remove(ix, np.random.default_rng(34).permutation(THR.N0).astype(np.int32))
        assert len(kept) == 0 and ix.n == 0 and ix.has_graph
        with THR._fresh(engine, np.zeros((0, DIM), np.float32), "l2", MODE, ix.get_graph()) as empty:
            C.same_base_codes(ix, empty, Q)
            C.same_graph_codes(ix, empty, Q)
        ix.hnsw_add(again, THR.EFC, THR.SEED)
        og, _ = O.hnsw_build_batched(again, H.batch_schedule(300, 1), O.L2, THR.M, THR.EFC, THR.SEED, O.BUILD_HEURISTIC, O.MODE_DEV)
        H.same_graph(ix.get_graph(), og, "grown again from nothing")
        with THR._fresh(engine, again, "l2", MODE, ix.get_graph()) as fresh:
            C.same_base_codes(ix, fresh, Q, again[150], expect=True)
            C.same_graph_codes(ix, fresh, Q, again[150])
            C.same_hnsw_searches(ix, fresh, Q)
            C.matches_f64(ix, again, "l2", Q)


# ---- the interleaved sequences ----------------------------------------------------------------------------------------------------
def test_ivf_add_and_remove_interleaved(native_lib, oracle, tune):
    from hnsw_clj_amd import engine

    rows, Q = TIR._data(oracle, DIM)
    N0 = TIR.N0
    rng = np.random.default_rng(6)
    with engine.Index(rows[:N0], "cosine", 0) as ix:
        ix.set_rejection_test(MODE)
        ix.ivf_build(TIR.NLIST, 3, 42)
        cen, off, ids = ix.get_ivf()
        C.touch(ix, Q)
        assign = TIR._device_assign(engine, tune, rows, "cosine", cen)
        ix.ivf_add(rows[N0:N0 + 300])
        off, ids = merged_lists(off, ids, assign[N0:N0 + 300])
        gone = np.concatenate([rng.choice(N0, 120, replace=False), N0 + rng.choice(300, 80, replace=False)])   # old and new rows
        off, ids = IR.compact_lists(off, ids, gone)
        present = np.arange(N0 + 300)[TIR._remove(ix, gone)]
        ix.ivf_add(rows[N0 + 300:N0 + 400])
        off, ids = merged_lists(off, ids, assign[N0 + 300:N0 + 400])
        present = np.concatenate([present, np.arange(N0 + 300, N0 + 400)])
        gone = np.array([len(present) - 50], np.int32)
        off, ids = IR.compact_lists(off, ids, gone)
        present = present[TIR._remove(ix, gone)]
        TIR._assert_same_ivf(ix, cen, off, ids)
        with TIU._fresh(engine, rows[present], "cosine", MODE, cen, off, ids, ix.ivf_stream_state()) as fresh:
            _ivf_checks(ix, fresh, Q, rows[present], "cosine")


def test_ivf_update_remove_add_update(native_lib, oracle, tune):
    from hnsw_clj_amd import engine

    rows, Q = TIU._data(oracle, DIM)
    N0 = TIU.N0
    spare = rows[N0:]
    rng = np.random.default_rng(6)
    with engine.Index(rows[:N0], "cosine", 0) as ix:
        ix.set_rejection_test(MODE)
        ix.ivf_build(TIU.NLIST, 3, 42)
        cen, off, ids = ix.get_ivf()
        C.touch(ix, Q)
        assign = TIU._device_assign(engine, tune, spare, "cosine", cen)
        pairing = TIU._Pairing(49, assign)
        cur = rows[:N0].copy()
        at, sp, moves = pairing.batch(TIU._list_of(off, ids), 200)
        TIU._assert_mixed(moves)
        off, ids = IU.updated_lists(off, ids, at, assign[sp])
        ix.ivf_update(at, spare[sp])
        cur[at] = spare[sp]
        gone = np.concatenate([rng.choice(N0, 150, replace=False), at[:10]])    # old rows, and ten that were just updated
        off, ids = IR.compact_lists(off, ids, gone)
        cur = cur[ix.ivf_remove(gone)]
        added = np.arange(1000, 1100)                        # spare values the pairing has not reached
        assert pairing.next <= 1000
        ix.ivf_add(spare[added])
        off, ids = merged_lists(off, ids, assign[added])
        cur = np.concatenate([cur, spare[added]])
        pairing.next = 1100
        at, sp, moves = pairing.batch(TIU._list_of(off, ids), 150)
        TIU._assert_mixed(moves)
        off, ids = IU.updated_lists(off, ids, at, assign[sp])
        ix.ivf_update(at, spare[sp])
        cur[at] = spare[sp]
        TIU._assert_same_ivf(ix, cen, off, ids)
        with TIU._fresh(engine, cur, "cosine", MODE, cen, off, ids, ix.ivf_stream_state()) as fresh:
            _ivf_checks(ix, fresh, Q, cur, "cosine")


def test_lsh_add_and_remove_interleaved(native_lib):
    from hnsw_clj_amd import engine

    rows, Q = TLR._data(DIM)
    n0 = 1000
    rng = np.random.default_rng(6)
    with engine.Index(rows[:n0], "cosine", 0) as ix:
        ix.set_rejection_test(MODE)
        ix.lsh_build(8, 6, 64, 42)
        planes = ix.lsh_get()[0]
        C.touch(ix, Q)
        ix.lsh_add(rows[n0:n0 + 257])
        gone = np.concatenate([rng.choice(n0, 100, replace=False), n0 + rng.choice(257, 50, replace=False)])
        now = np.arange(n0 + 257)[TLR._remove(ix, gone)]
        ix.lsh_add(rows[n0 + 257:n0 + 320])
        now = np.concatenate([now, np.arange(n0 + 257, n0 + 320)])
        with TLR._fresh(engine, rows[now], "cosine", planes, MODE) as fresh:
            TLR._assert_same_tables(ix, fresh)
            C.same_base_codes(ix, fresh, Q, rows[now][len(now) // 2], expect=True)
            C.matches_f64(ix, rows[now], "cosine", Q)


@pytest.mark.parametrize("builder", ["closest", "heuristic"])
def test_hnsw_add_and_remove_interleaved(native_lib, oracle, builder):
    from hnsw_clj_amd import engine

    O = oracle
    rows, Q = THR._rows(O, DIM)
    heuristic = builder == "heuristic"
    flags = O.BUILD_HEURISTIC if heuristic else 0
    rng = np.random.default_rng(21)
    nxt = 400
    with THR._built(engine, rows[:nxt], "cosine", heuristic, MODE) as ix:
        C.touch(ix, Q)
        g, present = ix.get_graph(), rows[:nxt]
        for step, m in (("remove", 70), ("add", 90), ("remove", 1), ("add", 1), ("remove", 130), ("add", 40)):
            if step == "remove":
                gone = rng.choice(ix.n, m, replace=False).astype(np.int32)
                g = HR.remove(O, present, O.COSINE, g, gone, heuristic)
                present = present[THR._remove(ix, gone)]
            else:
                n_before = ix.n
                ix.hnsw_add(rows[nxt:nxt + m], THR.EFC, THR.SEED)
                present = np.ascontiguousarray(np.concatenate([present, rows[nxt:nxt + m]]))
                nxt += m
                g, _ = O.hnsw_build_batched(present, H.batch_schedule(len(present), n_before), O.COSINE, THR.M, THR.EFC, THR.SEED, flags,
                                            O.MODE_DEV, start=g)
            H.same_graph(ix.get_graph(), g, "after %s %d" % (step, m))
        with THR._fresh(engine, present, "cosine", MODE, ix.get_graph()) as fresh:
            row = present[len(present) // 2]
            C.same_base_codes(ix, fresh, Q, row, expect=True)
            C.same_graph_codes(ix, fresh, Q, row)
            C.same_hnsw_searches(ix, fresh, Q)
            C.matches_f64(ix, present, "cosine", Q)
