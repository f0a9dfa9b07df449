"""No-GPU half of the crafted P-HNSW streams (pcaf_streams.py): the shapes reach the instantiations and plans they are meant
to reach, the planted rows sit on the plan's edges, and every input is decided in float64 -- conditions on the inputs, so that
test_pcaf_streams_gpu.py may hold the kernels to exact candidate sets."""
import numpy as np
import pytest

import pcaf_streams as S
from hnsw_clj_amd import pcaf
from test_pcaf_one_handle_gpu import reference


def test_plan_restatement_matches_the_documented_cases():
    """the figures of pcaf.hip's comments and of the shapes the older tests run: all of those plan 8 waves, NT 1 / 4, NV 4 / 13"""
    for n, T, nq, kf in [(1500, 16, 33, 30), (1500, 20, 1, 24), (700, 100, 32, 30), (300, 8, 5, 64), (40000, 8, 260, 30)]:
        assert S.filter_plan(n, T, nq, kf, False).nw == S.filter_plan(n, T, nq, kf, True).nw == 8
        assert S.project_nt(T) in (1, 4) and S.filter_nv(T) in (4, 13)
    assert S.filter_plan(1500, 16, 33, 30, True)[2:] == (256, 6)      # test_pcaf_filtered_gpu "ragged": 6 slabs of 256 rows
    assert S.filter_plan(40000, 8, 260, 30, True)[2:] == (1536, 27)   # "steps": 27 slabs of 1536 rows
    assert S.filter_plan(40000, 8, 8192, 30, True).nslabs == 1        # "refill": one slab
    assert S.filter_lds(256, 128, 1) <= S.LDS_MAX < S.filter_lds(256, 128, 2)


def test_needle_shapes_reach_every_instantiation_and_plan():
    nts, nvs, nws = set(), set(), set()
    for name, (T, dim, n, kf) in S.NEEDLES.items():
        assert dim > T and dim % 32 != 0 and 600 <= n <= 1500 and n % 32 != 0 and kf <= S.MAX_KF
        plain, masked = S.filter_plan(n, T, S.NEEDLE_NQ, kf, False), S.filter_plan(n, T, S.NEEDLE_NQ, kf, True)
        nt, nv, nw_plain, nw_masked = S.NEEDLE_REACH[name]
        assert (S.project_nt(T), S.filter_nv(T)) == (nt, nv), name
        assert nw_plain in (None, plain.nw) and nw_masked in (None, masked.nw), (name, plain, masked)
        assert plain.lds <= S.LDS_MAX and masked.lds <= S.LDS_MAX
        nts.add(nt), nvs.add(nv), nws.update([plain.nw, masked.nw])
    assert nts == {2, 4, 8} and nvs == {8, 16, 24, 32} and nws == {1, 2, 4, 8}
    assert any(dim % 4 != 0 for _, dim, _, _ in S.NEEDLES.values())
    assert S.pcaf_tp(250) == 256
    n = S.NEEDLES["T120_split"][2]
    assert S.filter_plan(n, 120, S.NEEDLE_NQ, 37, False).nw == 8 and S.filter_plan(n, 120, S.NEEDLE_NQ, 37, True).nw == 4


@pytest.mark.parametrize("name", list(S.NEEDLES))
def test_needle_inputs_are_what_the_rule_assumes(name):
    inp = S.needle_inputs(name)
    T, n = inp.T, inp.n
    assert len(set(inp.pi.tolist())) == T and (inp.pi != np.arange(T)).any() and inp.dim - 1 in inp.pi
    assert (inp.P.sum(axis=1) == 1).all() and (inp.P[np.arange(T), inp.pi] == 1).all()
    assert inp.member.any(axis=0).all(), "a component no query asks for"
    sizes = inp.member.sum(axis=1)
    assert sizes.max() <= 12 <= inp.kf and len(set(sizes.tolist())) > 2
    assert (inp.member[32] != inp.member[:32]).any(axis=1).all()   # the ragged block's query asks for a set of its own
    low = inp.base[:, inp.pi]
    assert ((low != 0).sum(axis=1) <= 1).all() and set(np.unique(low).tolist()) == {-1.0, 0.0, 1.0}
    assert (low[inp.needle_id] == np.eye(T)).all() and inp.needle_id.max() == n - 1
    assert (np.diff(np.sort(inp.needle_id)) > 1).all(), "needles are interleaved with fillers"
    assert (inp.sign == 0).sum() > 100 and (inp.sign == -1).sum() > 100
    assert np.isfinite(inp.base).all() and (np.abs(inp.base[inp.base != 0]) > 1e-30).all()
    # the rule against the float64 restatement: equal distances tie to the lower id there as well
    for form in ("plain", "some"):
        allow = S.needle_masks(name)[form]
        rows = np.arange(n) if allow is None else np.flatnonzero(allow)
        want, _, _, _, _ = reference(inp.base[rows], inp.P, inp.Q, inp.kf, inp.kf)
        for q, cand in enumerate(S.needle_candidates(inp, allow)):
            assert set(rows[want[q]].tolist()) == set(cand.tolist()), (form, q)
            needles = [i for i in inp.needle_id[inp.member[q]] if allow is None or allow[i]]
            assert set(needles) <= set(cand.tolist())
    some = S.needle_masks(name)["some"]
    assert (~some[inp.needle_id]).sum() >= T // 3 and some.sum() > inp.kf
    each = S.needle_masks(name)["each"]
    assert each[1].all() and each[2].sum() == 5 < inp.kf and not each[3].any()


def test_stream_plans_and_planted_rows():
    n, T, nq = S.STREAM_N, S.STREAM_T, S.STREAM_NQ
    assert n % 32 != 0
    for kf in S.STREAM_KF:
        plan = S.filter_plan(n, T, nq, kf, False)
        assert plan == S.filter_plan(n, T, nq, kf, True)._replace(lds=plan.lds)
        assert (plan.nw, plan.slab_rows, plan.nslabs) == (8, 256, 6)
        rows = S.planted_rows(n, plan)
        assert rows[0] == n - 1 and len(rows) == len(set(rows)) and max(rows) < n
        edges = {s * 256 for s in range(6)} | {min(n, s * 256 + 256) - 1 for s in range(6)}
        wave_ends = {s * 256 + w * 32 + 31 for s in range(6) for w in range(8) if s * 256 + w * 32 + 31 < n}
        assert edges | wave_ends == set(rows)
        rank = S.stream_inputs("planted", kf).rank
        assert sorted(rank.tolist()) == list(range(n))
        assert set(rows[:kf]) <= set(np.flatnonzero(rank < kf).tolist())   # (kf = 64, 127, 128: every edge row is among the best)
    # one 256-row step of the descending stream beats the threshold with every row: 256 keys against a buffer of 2 kf
    assert all(2 * kf < 256 for kf in (1, 2, 64, 127)) and 2 * 128 == 256


def test_merge_shapes_fill_the_refine_buffer():
    for name, (T, n, nq) in S.MERGE.items():
        plan = S.filter_plan(n, T, nq, 128, False)
        assert plan.nslabs * 128 > 1024, (name, plan)
        assert plan == S.filter_plan(n, T, nq, 128, True)._replace(lds=plan.lds)
    a, b = (S.filter_plan(n, T, nq, 128, False) for T, n, nq in S.MERGE.values())
    assert (a.nw, a.slab_rows, a.nslabs) == (8, 256, 17)   # 2176 keys a query, 544 a wave against a 256-key wave buffer
    assert (b.nw, b.slab_rows, b.nslabs) == (1, 32, 47)    # 32 real keys and 96 all-ones keys a slab
    # (a single query over 40000 rows -- test_pcaf_filtered_gpu's test_identities[steps] -- plans 157 slabs and cuts mid-merge too,
    # on random rows and against the library itself; here the survivors of the cut are known)
    assert S.filter_plan(40000, 8, 1, 30, True).nslabs == 157


@pytest.mark.parametrize("order", S.STREAM_ORDERS)
@pytest.mark.parametrize("kf", S.STREAM_KF)
def test_stream_inputs_are_decided(order, kf):
    inp = S.stream_inputs(order, kf)
    masks = S.stream_masks(inp.n, len(inp.Q))
    if order == "identical":  # every distance ties: the row id decides, which is what that case is about
        low = inp.base[:, :inp.T]
        assert (low == low[0]).all()
        return
    for form, allow in masks.items():
        assert S.boundary_margin(inp, allow) >= 10.0, (form, S.boundary_margin(inp, allow))
        assert S.stream_expected(order, kf, kf, form)[2].all(), form
    if order == "monotone":
        d = S.cosine64(inp.Q[0, :inp.T], inp.base[:, :inp.T]), S.cosine64(inp.Q[1, :inp.T], inp.base[:, :inp.T])
        assert (np.diff(np.float32(d[0])) < 0).all() and (np.diff(np.float32(d[1])) > 0).all()


@pytest.mark.parametrize("name", list(S.MERGE))
def test_merge_inputs_are_decided(name):
    T, n, nq = S.MERGE[name]
    inp = S.stream_inputs("monotone", 128, T, n, nq)
    for form, allow in S.stream_masks(n, nq).items():
        assert S.boundary_margin(inp, allow) >= 10.0, form
        assert S.stream_expected("monotone", 128, 128, form, T, n, nq)[2].all(), form


def test_sliced_sample_is_decided():
    s, inp = S.SLICED, S.sliced_inputs()
    assert s["nq"] == S.SLICE + 33
    assert {0, S.SLICE - 1, S.SLICE, S.SLICE + 1, s["nq"] - 1} <= set(inp.sample.tolist()) and len(inp.sample) == 20
    P = pcaf.create_random_projection(s["dim"], s["T"])
    for allow in (None, inp.allow):
        assert S.reference_under(inp.base, P, inp.Q[inp.sample], s["k"], s["kf"], allow)[2].all()
    words = S.sliced_each_words()
    assert words.shape == (s["nq"], 10) and (words[:, -1] >> (s["n"] & 31) == 0).all()


def test_mutation_shapes_reach_nt_2_and_8():
    assert [S.project_nt(T) for _, T in S.MUTATION_SHAPES] == [2, 8]
