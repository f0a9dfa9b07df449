"""The launch number of the small HNSW launches (hnsw.hip: hnsw_number_launch) across its wrap."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from util import assert_exact  # noqa: E402

pytestmark = pytest.mark.gpu


def test_small_launch_numbers_wrap_without_stale_words(native_lib, oracle, tune):
    """The round-2 helper kernel and the several-CU kernel tag every word they publish with the launch's number: 24 bits of it in
    the helper tables, the low 14 bits beside the node in the several-CU kernel's (solo_tag).  A word of launch s must never be
    read by a later launch whose tag compares equal -- whichever kernel took the launches in between.

    A fresh handle (its numbers start at 0; the build's searches take none), 20,000 clustered rows of dim 40, the int8 test
    off, SOLO = 1 (several CUs from ef 96, the helper kernel below).  Every call is a single-query hnsw_search whose ids,
    distance bits and counters must equal the oracle's:
      1. four several-CU launches (ef 200; queries A1..A4 of one cluster): records under tags 1..4, one per region;
      2. 16,380 helper launches (ef 50): on a shared counter the launch that reaches 0x4000 is a helper launch;
      3. 24 several-CU launches B1, B2, B3, A1, ...: tags 1.. again, in the regions A1..A4 wrote, for OTHER queries of the same
         neighbourhood -- a record that survived would be taken for this launch's distance of that node;
      4. 16,400 several-CU launches rotating over the seven queries (7 divides neither 0x2000 nor 0x4000: the query that
         reuses a tag is never the one that wrote it) -- the same for a design with a counter per table.
    32,808 launches of 0.1 - 0.5 ms; the test prints its wall time (the bound it was given: 60 s on one MI355X -- beyond that,
    shrink the index, not the launch counts)."""
    from hnsw_clj_amd import engine

    O = oracle
    assert engine.device_count() >= 1, "no GPU visible"
    tune.set("SOLO", 1)
    base = O.generate_dataset(20000, 40, "clustered", seed=81).astype(np.float32)
    with engine.Index(base, "cosine") as idx:
        idx.hnsw_build(16, 80, 42)
        idx.set_rejection_test(0)
        g = idx.get_graph()
        # seven queries of ONE cluster: a base row and six of its graph neighbours, each moved a little off its row
        nb = [int(v) for v in g.l0_adj.reshape(g.n, -1)[123] if v >= 0][:6]
        rng = np.random.default_rng(7)
        Q = (base[[123] + nb] + 0.01 * rng.standard_normal((7, 40))).astype(np.float32)
        helper_q = (base[4567:4568] + 0.01 * rng.standard_normal((1, 40))).astype(np.float32)
        want = O.hnsw_search(base, g, Q, 10, ef=200, metric=O.COSINE, mode=O.MODE_DEV)
        want_h = O.hnsw_search(base, g, helper_q, 10, ef=50, metric=O.COSINE, mode=O.MODE_DEV)

        def solo(i, what):
            n0 = engine.debug_counter("hnsw_solo")
            ids, d, st = idx.hnsw_search(Q[i:i + 1], 10, 200, want_stats=True)
            assert engine.debug_counter("hnsw_solo") == n0 + 1, "not the several-CU kernel"
            assert_exact(ids, d, want[0][i:i + 1], want[1][i:i + 1], what)
            np.testing.assert_array_equal(st, want[2][i:i + 1], what)

        t0 = time.perf_counter()
        for i in range(4):
            solo(i, "first launches, query A%d" % (i + 1))
        n0 = engine.debug_counter("hnsw_helpers")
        for j in range(16380):
            ids, d, st = idx.hnsw_search(helper_q, 10, 50, want_stats=True)
            assert_exact(ids, d, want_h[0], want_h[1], "helper launch %d" % j)
            np.testing.assert_array_equal(st, want_h[2])
        assert engine.debug_counter("hnsw_helpers") == n0 + 16380, "not the helper kernel"
        for j in range(24):
            solo((4 + j) % 7, "launch %d behind the wrap, query %d" % (j, (4 + j) % 7))
        for j in range(16400):
            solo(j % 7, "second cycle, launch %d, query %d" % (j, j % 7))
        print("32,808 single-query launches: %.1f s" % (time.perf_counter() - t0))
