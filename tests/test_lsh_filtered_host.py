"""Hybrid LSH filtered search without a GPU: the filtered model (lsh_filtered_model.py) against examples worked by hand and
against lsh_model under an all-ones mask, the four entry points in the library / the binding / the header, the argument codes
that need no device, the protocol classes, and the mirror's mask handling against a fake engine handle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lsh_filtered_model as F
import lsh_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hnswgpu_lsh_search_filtered", "hnswgpu_lsh_search_filtered_dev", "hnswgpu_lsh_search_filtered_each",
         "hnswgpu_lsh_search_filtered_each_dev"]


@pytest.mark.parametrize("case", F.HAND_FILTERED, ids=lambda c: c[0])
def test_model_by_hand(case):
    """Filter-then-take against the hand-worked ids, and take-then-filter beside it: both numbers on record."""
    _, allow, (k, probes, radius, take_main, take_flip), want, want_post = case
    off, ids = M.buckets(M.HAND_CODES, 2)
    d = M.hand_distances()
    assert F.search(d, [3, 3], off, ids, 2, k, probes, radius, take_main, take_flip, allow) == want
    assert F.post_filter(d, [3, 3], off, ids, 2, k, probes, radius, take_main, take_flip, allow) == want_post
    assert all(allow[r] for r in want)


def test_the_two_rules_differ():
    """Case (a): filter-then-take returns [1, 4, 2]; the unfiltered search cut to its takes first keeps only [1]."""
    name, allow, cfg, want, want_post = F.HAND_FILTERED[0]
    assert name == "a_row0_cleared" and cfg == (3, 2, 0, 2, 1)
    assert want == [1, 4, 2] and want_post == [1]
    off, ids = M.buckets(M.HAND_CODES, 2)
    assert F.passing_per_probe([3, 3], off, ids, 2, 2, 0, 2, 1, allow) == [(2, 2), (5, 2)]   # [1, 2] whole; [1, 3, 4, 5, 6] cut


@pytest.mark.parametrize("case", F.HAND_ALL_ONES, ids=lambda c: "k%d_p%d_r%d_t%d_%d" % c[0])
def test_model_all_ones_by_hand(case):
    (k, probes, radius, take_main, take_flip), want = case
    off, ids = M.buckets(M.HAND_CODES, 2)
    allow = np.ones(len(M.HAND_ROWS), np.bool_)
    assert F.search(M.hand_distances(), [3, 3], off, ids, 2, k, probes, radius, take_main, take_flip, allow) == want


def test_model_all_ones_equals_the_unfiltered_model():
    rng = np.random.default_rng(3)
    n, nq, T, bits = 400, 9, 4, 3
    codes = rng.integers(0, 1 << bits, (n, T)).astype(np.uint16)
    qcodes = rng.integers(0, 1 << bits, (nq, T)).astype(np.uint16)
    D = rng.integers(0, 50, (nq, n)).astype(np.float64)   # many ties
    off, ids = M.buckets(codes, bits)
    for cfg in [(2, 1, 20, 10), (4, 3, 5, 7), (4, 0, 30, 1), (9, 9, 1, 1)]:
        ei, ed = M.search_batch(D, qcodes, off, ids, bits, 10, *cfg)
        for allow in (np.ones(n, np.bool_), np.ones((nq, n), np.bool_)):
            gi, gd = F.search_batch(D, qcodes, off, ids, bits, 10, *cfg, allow)
            assert np.array_equal(gi, ei) and np.array_equal(gd, ed)
    # one mask per query: row q is the single-mask search of (query q, mask q)
    masks = rng.random((nq, n)) < 0.3
    masks[2] = False
    gi, gd = F.search_batch(D, qcodes, off, ids, bits, 10, 4, 3, 5, 7, masks)
    for q in range(nq):
        si, sd = F.search_batch(D[q:q + 1], qcodes[q:q + 1], off, ids, bits, 10, 4, 3, 5, 7, masks[q])
        assert np.array_equal(gi[q], si[0]) and np.array_equal(gd[q], sd[0])
        assert all(masks[q, r] for r in gi[q] if r >= 0)
    assert (gi[2] == -1).all()


def test_model_is_the_unfiltered_search_on_the_passing_rows():
    """The equivalence the header states, inside the models: filtering == lsh_model on the sub-index, ids mapped back."""
    rng = np.random.default_rng(4)
    n, nq, T, bits = 300, 6, 3, 2
    codes = rng.integers(0, 1 << bits, (n, T)).astype(np.uint16)
    qcodes = rng.integers(0, 1 << bits, (nq, T)).astype(np.uint16)
    D = rng.integers(0, 40, (nq, n)).astype(np.float64)
    off, ids = M.buckets(codes, bits)
    allow = rng.random(n) < 0.4
    rows = np.flatnonzero(allow)
    soff, sids = M.buckets(codes[rows], bits)
    for cfg in [(3, 2, 8, 4), (2, 0, 3, 1)]:
        gi, gd = F.search_batch(D, qcodes, off, ids, bits, 10, *cfg, allow)
        si, sd = M.search_batch(D[:, rows], qcodes, soff, sids, bits, 10, *cfg)
        assert np.array_equal(gi, np.where(si >= 0, rows[np.maximum(si, 0)], -1)) and np.array_equal(gd, sd)


def test_symbols_everywhere(native_lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", native_lib.SO]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "hnswgpu.h")).read()
    for name in NAMES:
        assert name in exported and name in native_lib.EXPORTS and name in native_lib._SIGS
        assert re.search(r"^int %s\(hnswgpu_index \*idx," % name, header, re.M), name
    assert native_lib._SIGS[NAMES[0]] == native_lib._SIGS[NAMES[2]] == native_lib._SIGS["hnswgpu_lsh_search"][:-2] + ["p", "p", "p"]
    assert native_lib._SIGS[NAMES[1]] == native_lib._SIGS[NAMES[3]] == native_lib._SIGS[NAMES[0]] + ["p"]


def test_null_handle(native_lib):
    """A null handle is refused before any HIP call."""
    L = native_lib.lib()
    buf = (ctypes.c_float * 16)()
    out = (ctypes.c_int32 * 16)()
    mask = (ctypes.c_uint32 * 4)()
    assert L.hnswgpu_lsh_search_filtered(None, buf, 1, 1, 1, 0, 1, 1, mask, out, buf) == -1
    assert b"idx is null" in L.hnswgpu_last_error()
    assert L.hnswgpu_lsh_search_filtered_each(None, buf, 1, 1, 1, 0, 1, 1, mask, out, buf) == -1
    assert L.hnswgpu_lsh_search_filtered_dev(None, buf, 1, 1, 1, 0, 1, 1, mask, out, buf, None) == -1
    assert L.hnswgpu_lsh_search_filtered_each_dev(None, buf, 1, 1, 1, 0, 1, 1, mask, out, buf, None) == -1


def test_protocol_types():
    from hnsw_clj_amd import protocol

    f = protocol.GpuFilterableHybridLshIndex(None)
    assert protocol.supports_filtering(f) is True
    assert protocol.supports_filtering(protocol.GpuHybridLshIndex(None)) is False
    assert f.index_type_star() == "hybrid-lsh" and protocol.supports_batch_search(f) and not protocol.supports_persistence(f)
    assert isinstance(f, protocol.GpuHybridLshIndex)


class _FakeHandle:
    """What hybrid_lsh's filtered mirrors need of engine.Index: records the calls, answers row q with [q-th call row, -1, ...]"""

    def __init__(self, n, dim):
        self.n, self.dim, self.calls = n, dim, []

    def _answer(self, Q, k):
        ids = np.full((len(Q), k), -1, np.int32)
        ids[:, 0] = Q[:, 0].astype(np.int32)      # a query's first component names the row it "finds"
        d = np.full((len(Q), k), np.inf, np.float32)
        d[:, 0] = Q[:, 1]
        return ids, d

    def lsh_search_filtered(self, Q, k, allow, num_probes, probe_radius, take_main, take_flip):
        self.calls.append(("single", np.array(Q), k, np.array(allow), num_probes, probe_radius, take_main, take_flip))
        return self._answer(Q, k)

    def lsh_search_filtered_each(self, Q, k, allow_each, num_probes, probe_radius, take_main, take_flip):
        self.calls.append(("each", np.array(Q), k, np.array(allow_each), num_probes, probe_radius, take_main, take_flip))
        return self._answer(Q, k)


def _fake(n=70, dim=4):
    from hnsw_clj_amd import hybrid_lsh as H

    h = _FakeHandle(n, dim)
    return h, H.HybridIndex(h, ["v%d" % i for i in range(n)], None)


def test_mirror_argument_checks():
    from hnsw_clj_amd import engine
    from hnsw_clj_amd import hybrid_lsh as H

    h, index = _fake()
    Q = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError):
        H.search_batch_filtered(index, Q, 5, np.ones(69, np.bool_))           # a bool array of the wrong length
    with pytest.raises(ValueError):
        H.search_batch_filtered(index, Q, 5, np.ones(70, np.int32))           # not a bool array
    with pytest.raises(ValueError):
        H.search_batch_filtered_each(index, Q, 5, [np.ones(70, np.bool_)] * 2)   # the wrong filter count
    with pytest.raises(ValueError):
        H.search_batch_filtered_each(index, Q, 5, [np.ones(70, np.bool_), np.ones(70, np.bool_), np.ones(71, np.bool_)])
    assert h.calls == []
    assert H.search_batch_filtered(index, Q[:0], 5, lambda i: True) == [] and H.search_batch_filtered_each(index, Q[:0], 5, []) == []
    # a callable predicate sees the caller's ids, once per row; modes map through mode_config with takes 2 k / k
    seen = []
    even = lambda i: seen.append(i) or int(i[1:]) % 2 == 0
    Q[:, 0] = [4, 6, 8]
    Q[:, 1] = [0.5, 0.25, 0.125]
    got = H.search_batch_filtered(index, Q, 5, even, "accurate")
    assert seen == index.ids
    kind, cq, k, allow, probes, radius, take_main, take_flip = h.calls.pop()
    assert (kind, k, probes, radius, take_main, take_flip) == ("single", 5, 8, 3, 10, 5) and np.array_equal(cq, Q)
    assert np.array_equal(allow, engine.pack_mask(np.arange(70) % 2 == 0, 70)) and allow.dtype == np.uint32 and allow.shape == (3,)
    assert got == [[{"id": "v4", "distance": 0.5}], [{"id": "v6", "distance": 0.25}], [{"id": "v8", "distance": 0.125}]]
    assert H.search_knn_filtered(index, Q[1], 5, even) == got[1]
    assert h.calls.pop()[4:6] == H.mode_config(None) == (6, 2)


def test_mirror_each_groups_masks_and_restores_the_order():
    from hnsw_clj_amd import engine
    from hnsw_clj_amd import hybrid_lsh as H
    from hnsw_clj_amd import protocol

    h, index = _fake()
    n = 70
    a = np.arange(n) % 2 == 0
    b = np.arange(n) % 3 == 0
    a_again = a.copy()                                  # equal bits in another object: one mask
    b_fn = lambda i: int(i[1:]) % 3 == 0                # ... and as a predicate
    Q = np.zeros((6, 4), np.float32)
    Q[:, 0] = np.arange(6) + 10                         # query q "finds" row 10 + q
    Q[:, 1] = np.arange(6)
    filters = [b, a, b_fn, a_again, a, b]
    got = H.search_batch_filtered_each(index, Q, 4, filters, "fast")
    assert len(h.calls) == 1
    kind, cq, k, rows, probes, radius, take_main, take_flip = h.calls.pop()
    assert (kind, k, probes, radius, take_main, take_flip) == ("each", 4, 4, 1, 8, 4)
    # mask b was met first: its queries 0, 2, 5 lead, then a's 1, 3, 4 -- equal masks adjacent, packed once each
    assert cq[:, 0].tolist() == [10, 12, 15, 11, 13, 14]
    pa, pb = engine.pack_mask(a, n), engine.pack_mask(b, n)
    assert rows.shape == (6, 3) and rows.dtype == np.uint32
    assert all(np.array_equal(rows[j], pb) for j in range(3)) and all(np.array_equal(rows[j], pa) for j in range(3, 6))
    assert [r[0]["id"] for r in got] == ["v%d" % (10 + q) for q in range(6)]       # the caller's order again
    assert [r[0]["distance"] for r in got] == [float(q) for q in range(6)]
    # one distinct mask: the single-mask call
    got = H.search_batch_filtered_each(index, Q, 4, [a, a_again, a, a, a_again, a])
    assert len(h.calls) == 1
    kind, cq, k, allow, probes, radius, _, _ = h.calls.pop()
    assert kind == "single" and np.array_equal(allow, pa) and np.array_equal(cq, Q) and (probes, radius) == (6, 2)
    assert [r[0]["id"] for r in got] == ["v%d" % (10 + q) for q in range(6)]
    # the protocol class goes through the same two mirrors
    p = protocol.GpuFilterableHybridLshIndex(index)
    assert p.search_knn_filtered_star(Q[2], 4, b, "turbo") == [{"id": "v12", "distance": 2.0}]
    assert h.calls.pop()[0] == "single"
    assert [r[0]["id"] for r in p.search_batch_filtered(Q[:2], 4, [a, b], "turbo")] == ["v10", "v11"]
    assert h.calls.pop()[0] == "each"
