"""The seven live-index mutations (hnswgpu_hnsw_add / _remove, hnswgpu_ivf_add / _remove / _update, hnswgpu_lsh_add / _remove) at
every loader width of pick_nch (engine.hip) and at padded rows (ld != dim), each followed by the searches the per-operation tests
make AND by the observers of mutation_checks.py, which read the compact copies (base-order int8 rows, list-order int8 tiles,
list-order half rows) that no saved file carries and no search at test size shows.

Every case: the handle in mode 2 (copies at every dim; at 127 and 128 mode 1 as well: below 128 such a handle owns none), the
lazily made copies made BEFORE the mutation (mutation_checks.touch: a chain remakes only what the handle holds), two calls of
m = 1 and m = 65 rows (one stays inside a wave, one crosses it), the fresh handle exactly as include/hnswgpu.h's equivalence
says, the expected lists / tables / graphs from the numpy models the per-operation tests use.

Sizes: the smallest at which the chains keep their edges.  IVF and LSH 600 rows + 200 spare: 19 mask words and 3 chunks of 256
positions, the last of each partial; 6 lists; 4 tables of 6 bits.  HNSW 400 rows, M 8, ef_construction 40.  Rows: the oracle's
clustered generator, drawn once per dim.

Input conditions, checked on the CPU against the models alone:
  * every ivf_update batch of 65 rows holds at least a quarter movers and a quarter stayers (test_ivf_update_gpu._assert_mixed,
    the assignment judged by the f64 guard);
  * every ivf_remove / lsh_remove call leaves a list (in every table: a bucket) with members untouched, and every call of more
    than one row removes from two different lists (in every table: buckets) -- the call of ONE row cannot, so the two calls
    together are asserted to;
  * every hnsw_remove call makes a list of a kept node lose a member and leaves another kept node's list untouched
    (hnsw_remove_model.candidates)."""
import numpy as np
import pytest

import hnsw_build_model as H
import hnsw_remove_model as HR
import ivf_remove_model as IR
import ivf_update_model as IU
import lsh_remove_model as LR
import mutation_checks as C
import test_hnsw_remove_gpu as THR
import test_ivf_add_gpu as TIA
import test_ivf_remove_gpu as TIR
import test_ivf_update_gpu as TIU
import test_lsh_remove_gpu as TLR
from ivf_add_model import merged_lists

# loader width (float4 chunks of 64 lanes per row) -> the dims that take it
WIDTHS = {
    1: [5, 127, 128],      # padded to 8; padded to 128, no copies in mode 1; the home pass possible, copies in mode 1
    2: [257],              # padded to 260: the first float4 of the second chunk, the second trip of the mover loops
    3: [768],
    4: [1000],
    6: [1536],
    8: [2048],
    12: [2050, 3072],      # padded to 2052: the first step into the widest loader; the limit
}
DIMS = [d for w in sorted(WIDTHS) for d in WIDTHS[w]]
OPS = ["hnsw_add", "hnsw_remove", "ivf_add", "ivf_remove", "ivf_update", "lsh_add", "lsh_remove"]
METRICS = ["cosine", "l2", "dot"]
# not the full cross: operation i at dim j runs metric (i + j) % 3 -- every operation sees each metric at three dims or more,
# every dim sees each metric across the operations (test_the_matrix_keeps_its_shape)
METRIC_OF = {(op, dim): METRICS[(i + j) % 3] for i, op in enumerate(OPS) for j, dim in enumerate(DIMS)}
BUILDER_OF = {dim: ("closest", "heuristic")[j % 2] for j, dim in enumerate(DIMS)}
CASES = [(op, dim, 2) for op in OPS for dim in DIMS] + [(op, dim, 1) for op in OPS for dim in (127, 128)]

N0, SPARE, NQ, NLIST = 600, 200, 64, 6
NH, HM, HEFC, SEED = 400, 8, 40, 42
TABLES, BITS = 4, 6
CALLS = (1, 65)
_DATA = {}


def _pick_nch(dim):
    """pick_nch (engine.hip) of a handle of this dim: ld = dim rounded up to 4 floats, one float4 per lane and chunk."""
    need = -(-((dim + 3) // 4) // 64)
    return next((o for o in (1, 2, 3, 4, 6, 8, 12) if o >= need), 0)


def test_the_matrix_keeps_its_shape():
    assert sorted(WIDTHS) == [1, 2, 3, 4, 6, 8, 12] and all(WIDTHS.values()), "a loader width went missing"
    for w, dims in WIDTHS.items():
        assert all(_pick_nch(d) == w for d in dims), "width %d: %s take %s" % (w, dims, [_pick_nch(d) for d in dims])
    assert _pick_nch(3072) == 12 and _pick_nch(3073) == 0                      # (the limit is the limit)
    assert any(d % 4 for d in DIMS), "no padded dim"
    assert 127 in DIMS and 128 in DIMS
    assert any(d % 4 and _pick_nch(d) > 1 for d in DIMS), "no padded dim beyond one chunk"
    for op in OPS:
        for metric in METRICS:
            assert sum(METRIC_OF[(op, d)] == metric for d in DIMS) >= 3, (op, metric)
    for d in DIMS:
        assert {METRIC_OF[(op, d)] for op in OPS} == set(METRICS), d
    for builder in ("closest", "heuristic"):
        assert sum(b == builder for b in BUILDER_OF.values()) >= 2
    assert {(op, d, m) for op, d, m in CASES} >= {(op, d, 1) for op in OPS for d in (127, 128)}
    assert len(set(CASES)) == len(CASES) == len(OPS) * (len(DIMS) + 2)


def _data(O, dim):
    """(rows f32 [N0 + SPARE, dim], queries f32 [NQ, dim]): clustered, from the oracle's generator; made once per dim, read-only."""
    if dim not in _DATA:
        rows = O.generate_dataset(N0 + SPARE + NQ, dim, "clustered", num_clusters=10, noise_level=0.1, seed=7).astype(np.float32)
        a, b = np.ascontiguousarray(rows[:N0 + SPARE]), np.ascontiguousarray(rows[N0 + SPARE:])
        a.flags.writeable = b.flags.writeable = False
        _DATA[dim] = (a, b)
    return _DATA[dim]


def _has_copies(mode, dim):
    """engine.hip: codes_wanted"""
    return mode == 2 or (mode == 1 and dim >= 128)


def _same_file(a, b, tmp_path):
    fa, fb = tmp_path / "mutated.idx", tmp_path / "fresh.idx"
    a.save(fa)
    b.save(fb)
    assert fa.read_bytes() == fb.read_bytes(), "the saved files differ"


# ---- IVF ------------------------------------------------------------------------------------------------------------------------
def _removal_from_lists(rng, where, m):
    """m row ids to remove, given every row's list: none from the last list with members (it stays untouched), and for m > 1 rows of
    two different lists at least.  Returns (gone, the lists that lose)."""
    lists = np.flatnonzero(np.bincount(where) > 0)
    assert len(lists) >= 3, "the lists are too few for the input condition"
    untouched = int(lists[-1])
    gone = rng.choice(np.flatnonzero(where != untouched), m, replace=False).astype(np.int32)
    lose = np.unique(where[gone])
    assert untouched not in lose and (m == 1 or len(lose) >= 2), "the removal does not meet its input condition"
    return gone, lose


def _ivf_case(engine, O, tune, tmp_path, op, dim, metric, mode):
    rows, Q = _data(O, dim)
    base, spare = rows[:N0], rows[N0:]
    rng = np.random.default_rng(1000 + dim)
    with engine.Index(base, metric, 0) as ix:
        ix.set_rejection_test(mode)
        ix.ivf_build(NLIST, 3, 42)
        cen, off, ids = ix.get_ivf()
        C.touch(ix, Q)
        cur = base.copy()
        if op == "ivf_add":
            assign = TIA._device_assign(engine, tune, rows, metric, cen)[N0:]
            TIA._check_f64_guard(metric, spare, cen, assign)
            at = 0
            for m in CALLS:
                got = ix.ivf_add(spare[at:at + m])
                np.testing.assert_array_equal(got, np.arange(N0 + at, N0 + at + m, dtype=np.int32))
                off, ids = merged_lists(off, ids, assign[at:at + m])
                cur = np.concatenate([cur, spare[at:at + m]])
                at += m
                TIA._assert_same_ivf(ix, cen, off, ids, "after m %d" % m)
            changed = int(assign[at - 1])
        elif op == "ivf_remove":
            lost = []
            for m in CALLS:
                gone, lose = _removal_from_lists(rng, TIU._list_of(off, ids), m)
                lost.extend(lose.tolist())
                off, ids = IR.compact_lists(off, ids, gone)
                cur = cur[TIR._remove(ix, gone)]
                TIR._assert_same_ivf(ix, cen, off, ids, "after m %d" % m)
            assert len(set(lost)) >= 2
            changed = int(lost[0])
        else:
            assign = TIU._device_assign(engine, tune, spare, metric, cen)
            TIU._check_f64_guard(metric, spare, cen, assign)
            pairing = TIU._Pairing(41, assign)
            for m in CALLS:
                at, sp, moves = pairing.batch(TIU._list_of(off, ids), m, first_moves=(m == 1))
                TIU._assert_mixed(moves)
                off, ids = IU.updated_lists(off, ids, at, assign[sp])
                ix.ivf_update(at, spare[sp])
                cur[at] = spare[sp]
                TIU._assert_same_ivf(ix, cen, off, ids, "after m %d" % m)
            assert moves.any()
            changed = int(assign[sp[moves][0]])              # a list that received a mover
        assert ix.n == len(cur) == off[-1]
        with TIU._fresh(engine, cur, metric, mode, cen, off, ids, ix.ivf_stream_state()) as fresh:
            TIU._assert_same_answers(engine, ix, fresh, Q)   # (the three IVF files' comparisons differ only in where they sample rows)
            _same_file(ix, fresh, tmp_path)
            copies = _has_copies(mode, dim)
            row = cur[len(cur) // 2]
            C.same_base_codes(ix, fresh, Q, row, expect=copies)
            C.same_list_half(ix, fresh, Q, row, expect=copies)
            if (dim + 3) // 4 * 4 % 128 == 0:
                ranges = C.home_ranges(off, changed)
                assert len(ranges) == 3, "no list boundary to straddle"
                C.same_home_pass(ix, fresh, Q, ranges, expect=copies)
            # (mode 1 keeps or drops the bounds pass by its own measurement: there only the equality is asserted)
            C.same_list_tiles(ix, fresh, Q, expect=True if mode == 2 else (None if copies else False))
            C.matches_f64(ix, cur, metric, Q)


# ---- LSH ------------------------------------------------------------------------------------------------------------------------
def _removal_from_buckets(rng, codes, m):
    """m row ids to remove, given every row's code per table: in every table none from its smallest bucket with members (it stays
    untouched), and for m > 1 rows of two different buckets at least."""
    n, T = codes.shape
    protected = np.zeros(n, np.bool_)
    kept_bucket = []
    for t in range(T):
        cnt = np.bincount(codes[:, t], minlength=1 << BITS)
        assert (cnt > 0).sum() >= 3, "table %d: too few buckets with members for the input condition" % t
        b = int(np.argmin(np.where(cnt > 0, cnt, n + 1)))
        kept_bucket.append(b)
        protected |= codes[:, t] == b
    gone = rng.choice(np.flatnonzero(~protected), m, replace=False).astype(np.int32)
    for t in range(T):
        lose = np.unique(codes[gone, t])
        assert kept_bucket[t] not in lose and (m == 1 or len(lose) >= 2), "table %d: the removal does not meet its input condition" % t
    return gone


def _lsh_case(engine, O, tmp_path, op, dim, metric, mode):
    rows, Q = _data(O, dim)
    base, spare = rows[:N0], rows[N0:]
    rng = np.random.default_rng(2000 + dim)
    configs = sorted({(min(p, TABLES), r, tm, tf) for p, r, tm, tf in TLR.CONFIGS})
    with engine.Index(base, metric, 0) as ix:
        ix.set_rejection_test(mode)
        ix.lsh_build(TABLES, BITS, 64, 42)
        planes, codes, boff, bids = ix.lsh_get()
        C.touch(ix, Q)
        cur, model = base.copy(), (codes, boff, bids)
        if op == "lsh_add":
            at = 0
            for m in CALLS:
                got = ix.lsh_add(spare[at:at + m])
                np.testing.assert_array_equal(got, np.arange(N0 + at, N0 + at + m, dtype=np.int32))
                cur = np.concatenate([cur, spare[at:at + m]])
                at += m
        else:
            for m in CALLS:
                gone = _removal_from_buckets(rng, model[0], m)
                model = LR.compact(*model, gone)
                cur = cur[TLR._remove(ix, gone)]
        with TLR._fresh(engine, cur, metric, planes, mode) as fresh:
            _, c1, o1, i1 = TLR._assert_same_tables(ix, fresh)   # (also against lsh_model.buckets, the numpy counting sort)
            if op == "lsh_add":
                np.testing.assert_array_equal(c1[:N0], codes, err_msg="an old row's code changed")
                np.testing.assert_array_equal(ix.lsh_hash(spare[:at]), c1[N0:], err_msg="a row's code depends on how it came")
            else:
                for got, want, what in zip((c1, o1, i1), model, ("codes", "off", "ids")):
                    np.testing.assert_array_equal(got, want, err_msg=what + " against the removal model")
            for cfg in configs:
                for nq in (1, TLR.NQ):
                    C.same(ix.lsh_search(Q[:nq], TLR.K, *cfg), fresh.lsh_search(Q[:nq], TLR.K, *cfg), "lsh_search %s nq %d" % (cfg, nq))
            C.same(ix.exact_knn(Q[:5], TLR.K), fresh.exact_knn(Q[:5], TLR.K), "exact_knn")
            np.testing.assert_array_equal(C.bits(ix.norms()), C.bits(fresh.norms()), err_msg="norms")
            _same_file(ix, fresh, tmp_path)
            C.same_base_codes(ix, fresh, Q, cur[len(cur) // 2], expect=_has_copies(mode, dim))
            C.matches_f64(ix, cur, metric, Q)


# ---- HNSW -----------------------------------------------------------------------------------------------------------------------
def _removal_from_graph(rng, g, m):
    """m row ids to remove from graph g: rows that some layer-0 list names (so a list loses a member), none of them the last node
    or a member of its layer-0 list (clusters of 40 rows under lists of 16: 65 random rows would reach nearly every list).  The
    condition itself -- a kept node's list loses a member, another kept node's list is untouched -- is judged by the model."""
    l0 = g.l0_adj.reshape(g.n, -1)
    named = np.unique(l0[l0 >= 0])
    spared = np.append(l0[g.n - 1], g.n - 1)
    gone = rng.choice(np.setdiff1d(named, spared), m, replace=False).astype(np.int32)
    keep = np.ones(g.n, np.bool_)
    keep[gone] = False
    left = np.array([len(HR.candidates(g, keep, int(u), 0)[1]) for u in np.flatnonzero(keep)])
    assert (left > 0).any() and (left == 0).any(), "the removal does not meet its input condition"
    return gone


def _hnsw_case(engine, O, op, dim, metric, mode):
    rows, Q = _data(O, dim)
    base, spare = rows[:NH], rows[N0:]
    code, heuristic = O.METRICS[metric], BUILDER_OF[dim] == "heuristic"
    flags = O.BUILD_HEURISTIC if heuristic else 0
    rng = np.random.default_rng(3000 + dim)
    Qh = np.ascontiguousarray(Q[:32])
    with engine.Index(base, metric, 0) as ix:
        ix.set_rejection_test(mode)
        ix.hnsw_build(HM, HEFC, SEED, heuristic=heuristic)
        g, cur = ix.get_graph(), base.copy()
        C.touch(ix, Q)
        if op == "hnsw_add":
            at = 0
            for m in CALLS:
                n_before = ix.n
                got = ix.hnsw_add(spare[at:at + m], HEFC, SEED)
                np.testing.assert_array_equal(got, np.arange(n_before, n_before + m, dtype=np.int32))
                cur = np.ascontiguousarray(np.concatenate([cur, spare[at:at + m]]))
                at += m
                g, _ = O.hnsw_build_batched(cur, H.batch_schedule(len(cur), n_before), code, HM, HEFC, SEED, flags, O.MODE_DEV, start=g)
                H.same_graph(ix.get_graph(), g, "after adding %d" % m)
        else:
            for m in CALLS:
                gone = _removal_from_graph(rng, g, m)
                g = HR.remove(O, cur, code, g, gone, heuristic)
                cur = np.ascontiguousarray(cur[THR._remove(ix, gone)])
                H.same_graph(ix.get_graph(), g, "after removing %d" % m)
        with THR._fresh(engine, cur, metric, mode, ix.get_graph()) as fresh:
            THR._assert_same_answers(ix, fresh, Qh, mode)
            copies = _has_copies(mode, dim)
            row = cur[len(cur) // 2]
            C.same_base_codes(ix, fresh, Q, row, expect=copies)
            if copies:
                C.same_graph_codes(ix, fresh, Q, row)
            C.same_hnsw_searches(ix, fresh, Qh)
            C.matches_f64(ix, cur, metric, Q)


@pytest.mark.gpu
@pytest.mark.parametrize("op,dim,mode", CASES, ids=["%s-dim%d-mode%d" % c for c in CASES])
def test_mutation_at_every_row_width(native_lib, oracle, tune, tmp_path, op, dim, mode):
    from hnsw_clj_amd import engine

    metric = METRIC_OF[(op, dim)]
    if op.startswith("ivf"):
        _ivf_case(engine, oracle, tune, tmp_path, op, dim, metric, mode)
    elif op.startswith("lsh"):
        _lsh_case(engine, oracle, tmp_path, op, dim, metric, mode)
    else:
        _hnsw_case(engine, oracle, op, dim, metric, mode)
