"""The P-HNSW kernels on crafted streams (pcaf_streams.py; the inputs' preconditions: test_pcaf_streams_host.py): every
projection and filter width, every waves-per-workgroup plan, the refine merge's cut and the second slice of a batch, held to
candidate sets that are known without a tolerance."""
import numpy as np
import pytest

import pcaf_streams as S
import util
from hnsw_clj_amd import engine, pcaf
from test_pcaf_mutations_gpu import SCRIPTS, observe, play, pool

pytestmark = pytest.mark.gpu


def bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=what)


def search(idx, form, Q, k, kf, allow):
    """allow: None (pcaf_search), bool [n] (one mask) or bool [nq][n] (one per query)"""
    if allow is None:
        return idx.pcaf_search(Q, k, kf)
    if np.ndim(allow) == 1:
        return idx.pcaf_search_filtered(Q, k, engine.pack_mask(allow, idx.n), kf)
    return idx.pcaf_search_filtered_each(Q, k, engine.pack_masks(allow, idx.n), kf)


# ---- 1. exact needles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.NEEDLES))
def test_needles(native_lib, name):
    inp = S.needle_inputs(name)
    X = np.float32(np.random.RandomState(3).randn(131, inp.dim))  # (a ragged second block of the projection kernel)
    with engine.Index(inp.base, "cosine", 0) as idx:
        idx.set_pcaf(inp.P)
        # every product is by 0 or 1: the selected coordinates, bit for bit, in every k-slot and in the chunk tail
        bits_equal(idx.pcaf_get()[1], inp.base[:, inp.pi], "projected rows")
        bits_equal(idx.pcaf_project(inp.Q), inp.Q[:, inp.pi], "projected queries")
        bits_equal(idx.pcaf_project(X), X[:, inp.pi], "projected noise")
        got = {form: search(idx, form, inp.Q, inp.kf, inp.kf, allow) for form, allow in S.needle_masks(name).items()}
    for form, (ids, d) in got.items():
        sets, want_ids, want_d = S.needle_expected(name, form)
        S.check_candidate_sets(ids, sets, "%s %s" % (name, form))
        S.check_bound_distances(ids, d, inp.Q, inp.base)
        util.assert_topk_parity(ids, d, want_ids, want_d, "%s %s" % (name, form))
    bits_equal(got["ones"][1], got["plain"][1], "an all-ones mask changes nothing")
    np.testing.assert_array_equal(got["ones"][0], got["plain"][0])


# ---- 2. stream orders ---------------------------------------------------------------------------------------------------
def check_stream(inp, got, expected, k, exact_sets):
    for form, (ids, d) in got.items():
        want_ids, want_d, _ = expected(form)
        assert ids.shape == d.shape == (len(inp.Q), k)
        if exact_sets:  # k >= kf: the returned ids are phase 1's whole selection
            S.check_candidate_sets(ids, [w[w >= 0] for w in want_ids], form)
        S.check_bound_distances(ids, d, inp.Q, inp.base)
        util.assert_topk_parity(ids, d, want_ids, want_d, form)


@pytest.mark.parametrize("order", [o for o in S.STREAM_ORDERS if o != "identical"])
@pytest.mark.parametrize("kf", S.STREAM_KF)
def test_stream_order(native_lib, order, kf):
    inp = S.stream_inputs(order, kf)
    masks = S.stream_masks(inp.n, len(inp.Q))
    with engine.Index(inp.base, "cosine", 0) as idx:
        idx.set_pcaf(inp.P)
        bits_equal(idx.pcaf_get()[1], inp.base[:, :inp.T], "projected rows")
        got = {form: search(idx, form, inp.Q, kf, kf, allow) for form, allow in masks.items()}
    check_stream(inp, got, lambda form: S.stream_expected(order, kf, kf, form), kf, True)


@pytest.mark.parametrize("kf", S.STREAM_KF)
def test_identical_rows_tie_to_the_lower_id(native_lib, kf):
    """Every projected row is the same: the candidates are the kf lowest passing ids -- keys, not distances, are compared."""
    inp = S.stream_inputs("identical", kf)
    masks = S.stream_masks(inp.n, len(inp.Q))
    with engine.Index(inp.base, "cosine", 0) as idx:
        idx.set_pcaf(inp.P)
        got = {form: search(idx, form, inp.Q, kf, kf, allow) for form, allow in masks.items()}
    for form, (ids, d) in got.items():
        allow = masks[form]
        sets = [np.flatnonzero(np.ones(inp.n, bool) if allow is None else allow if allow.ndim == 1 else allow[q])[:kf]
                for q in range(len(inp.Q))]
        S.check_candidate_sets(ids, sets, form)
        S.check_bound_distances(ids, d, inp.Q, inp.base)
        util.assert_topk_parity(ids, d, *S.exact_phase2(inp.Q, inp.base, sets, kf), form)


@pytest.mark.parametrize("kf,k", [(1, 4), (2, 1), (64, 70), (64, 22), (128, 131), (127, 50)])
def test_k_beside_kf(native_lib, kf, k):
    """k > kf: -1 / +inf behind the kf candidates; k < kf: the refine's own selection among them"""
    inp = S.stream_inputs("sawtooth", kf)
    assert S.effective_kf(k, kf, inp.n) == kf
    masks = S.stream_masks(inp.n, len(inp.Q))
    with engine.Index(inp.base, "cosine", 0) as idx:
        idx.set_pcaf(inp.P)
        got = {form: search(idx, form, inp.Q, k, kf, allow) for form, allow in masks.items()}
    check_stream(inp, got, lambda form: S.stream_expected("sawtooth", kf, k, form), k, k >= kf)
    if k > kf:
        assert (got["plain"][0][:, kf:] == -1).all() and (got["plain"][0][:, :kf] >= 0).all()


@pytest.mark.parametrize("name", list(S.MERGE))
def test_refine_merge(native_lib, name):
    """nslabs * kf > 1024 keys a query: a wave of the merge meets more than 256 keys under its threshold and cuts mid-way (odd
    queries: the best rows come first and must survive the cut; even queries: they come last)."""
    T, n, nq = S.MERGE[name]
    inp = S.stream_inputs("monotone", 128, T, n, nq)
    masks = S.stream_masks(n, nq)
    with engine.Index(inp.base, "cosine", 0) as idx:
        idx.set_pcaf(inp.P)
        got = {form: search(idx, form, inp.Q, 128, 128, allow) for form, allow in masks.items()}
    check_stream(inp, got, lambda form: S.stream_expected("monotone", 128, 128, form, T, n, nq), 128, True)


# ---- 3. the second slice of queries -------------------------------------------------------------------------------------
def test_second_slice(native_lib):
    s, inp = S.SLICED, S.sliced_inputs()
    k, kf, sample = s["k"], s["kf"], inp.sample
    P = pcaf.create_random_projection(s["dim"], s["T"])
    words = S.sliced_each_words()
    one = engine.pack_mask(inp.allow, s["n"])
    with engine.Index(inp.base, "cosine", 0) as idx:
        idx.set_pcaf(P)
        plain = idx.pcaf_search(inp.Q, k, kf)
        masked = idx.pcaf_search_filtered(inp.Q, k, one, kf)
        each = idx.pcaf_search_filtered_each(inp.Q, k, words, kf)
        alone = [(idx.pcaf_search(inp.Q[q:q + 1], k, kf), idx.pcaf_search_filtered(inp.Q[q:q + 1], k, one, kf),
                  idx.pcaf_search_filtered(inp.Q[q:q + 1], k, words[q], kf)) for q in sample]
    for (ids, d), allow, what in ((plain, None, "plain"), (masked, inp.allow, "one mask")):
        assert ids.shape == d.shape == (s["nq"], k)
        want_ids, want_d, decided = S.reference_under(inp.base, P, inp.Q[sample], k, kf, allow)
        assert decided.all()
        util.assert_topk_parity(ids[sample], d[sample], want_ids, want_d, what)
    for i, q in enumerate(sample):
        for (ids, d), (ids1, d1), what in zip((plain, masked, each), alone[i], ("plain", "one mask", "each")):
            np.testing.assert_array_equal(ids[q], ids1[0], err_msg="%s q%d" % (what, q))
            bits_equal(d[q], d1[0], "%s q%d" % (what, q))


# ---- 4. mutated handles at NT = 2 and NT = 8 ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.MUTATION_SCRIPTS)
@pytest.mark.parametrize("dim,T", S.MUTATION_SHAPES)
def test_mutated_handle_equals_fresh(native_lib, dim, T, name):
    """test_pcaf_mutations_gpu's check at the projection widths it leaves out: the plain kernel (add) and its MAP form (update)"""
    rows, Q = pool(dim)
    P = pcaf.create_random_projection(dim, T)
    n0 = SCRIPTS[name][0]
    with engine.Index(rows[:n0], "cosine", 0) as idx:
        idx.set_pcaf(P)
        want_rows = play(idx, dim, SCRIPTS[name])
        assert idx.n == len(want_rows)
        allow = np.random.RandomState(3).rand(idx.n) < 0.5
        got = observe(idx, Q, allow)
    with engine.Index(want_rows, "cosine", 0) as fresh:
        fresh.set_pcaf(P)
        want = observe(fresh, Q, allow)
    for what, a, b in zip(("low rows", "norms", "ids", "distances", "filtered ids", "filtered distances"), got, want):
        np.testing.assert_array_equal(a, b, err_msg=what)
