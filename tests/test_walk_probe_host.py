"""Host proofs for tests/test_gpu_walks_exact.py (no GPU, no library): the certificate holds for every case of its case
table, the unflawed walk model equals the float64 reference bit for bit, every flaw of the model is seen by a named
case, and the case table reaches every launch regime of launch_slice at 256 and at 304 CUs."""
import numpy as np
import pytest

import walk_probe as wp

FUSED = [(c[0], w) for c in wp.FUSED_CASES for w in (False, True)]


class _Refs(dict):
    """(graph, dist, P, w, float64 reference) of a fused case, computed on first use."""

    def __missing__(self, key):
        g, dist, P, w = wp.fused_data(*key)
        self[key] = (g, dist, P, w, wp.ref_fused(g, dist, P, w))
        return self[key]


@pytest.fixture(scope="module")
def fused_refs():
    return _Refs()


def test_placed_rows_cover_the_ladders():
    g = wp.graph("ladder")
    N = g.N
    assert N % 16 != 0
    pl = {(q, l0, l1) for q, _, l0, l1 in g.placed}
    slots = {s for q, s, _, _ in g.placed if q == 0}
    assert {0, N - 1, 15, 16, 31, 32} <= slots
    for l in wp.LIGHT_LADDER:
        assert (0, l, 0) in pl and (0, 0, l) in pl, l
    assert {l0 + l1 for q, l0, l1 in pl if q == 0 and l0 and l1 and max(l0, l1) <= 32} >= {8, 9, 16, 17, 33, 64}
    for l in wp.MEDIUM_LADDER:
        assert {(1, l, 0), (1, l, 1)} & pl and {(1, 0, l), (1, 1, l)} & pl, l
    for l in wp.HUGE_LADDER:
        assert {(2, l, 0), (2, 0, l), (2, l, l)} <= pl, l
    assert len(g.big_nodes(1)) <= wp.BIG_CAP and len(g.big_nodes(2)) <= wp.BIG_CAP      # medium / huge rows are LISTED
    for name in ("b41", "b1_n1024", "b1_n2048"):
        gg = wp.graph(name)
        assert 0 < len(gg.big_nodes(gg.B - 1)) <= wp.BIG_CAP, name
    assert sorted(wp.graph("relcounts").rel_cnt.tolist()) == [1, 3, 4, 5, 16, 17, 40]
    h = wp.graph("hubs")
    assert h.R > 1024 and wp.walk_variant(h.rel_max, 200) == wp.WALK_L2_GATHER


@pytest.mark.parametrize("name,wts", FUSED)
def test_certificate_and_model_of_the_fused_cases(fused_refs, name, wts):
    g, dist, P, w, want = fused_refs[name, wts]
    _, _, D, variant, regime, form = wp.FUSED_BY_NAME[name]
    assert wp.walk_variant(g.rel_max, D) == variant
    if regime is not None:
        for cus in (256, 304):
            assert wp.launch_regime(g.B, g.N, D, variant, cus)["regime"] == wp.REGIME_AT[cus][name]
    if form is not None:
        assert wp.hub_form(g, D) == form
    wp.certify_fused(name, g, dist, P, w, want)
    assert (np.asarray(dist) == 0).mean() > 0.2 and ((dist > 0) & (dist <= 3 * 2.0 ** -10)).any()
    assert np.array_equal(wp.walk_model(g, dist, P, w), want)
    if regime is not None and wp.REGIME_AT[304][name] != regime:
        assert np.array_equal(wp.walk_model(g, dist, P, w, cus=304), want)


# which case sees which flaw (the model with the flaw differs from float64 on it)
FLAW_SEEN_BY = {
    "drop_last_mod4": ("ladder_d20", False),
    "drop_last_mod8": ("ladder_d20", False),
    "drop_last_mod64": ("ladder_d20", False),
    "second_from_dir0": ("ladder_d20", False),
    "drop_last_float4": ("ladder_d200", False),
    "skip_small_prior": ("ladder_d20", True),          # w^2 p spans 1/4 .. 60 units: only the weighted family reaches 2^-7
    "skip_partial_last_set": ("ladder_d20", False),
    "huge_missing_in_one_part": ("b41_d200", False),
    "skip_last_question": ("ladder_d20", False),
    "hub_run_twice": ("hubs_d200", False),
    "weight_unsquared": ("ladder_d20", True),
    "swap_tables": ("ladder_d20", False),
}


@pytest.mark.parametrize("flaw", wp.FLAWS)
def test_every_flaw_is_seen_by_its_case(fused_refs, flaw):
    name, wts = FLAW_SEEN_BY[flaw]
    g, dist, P, w, want = fused_refs[name, wts]
    got = wp.walk_model(g, dist, P, w, flaw=flaw)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad), (flaw, name)
    # ... and by rows of the kind the flaw is about
    ln = (g.len0 + g.len1)[bad]
    if flaw == "drop_last_mod64":
        assert (ln % 64 == 1).all() and (ln <= wp.TEAM_DEG).any() and (ln > wp.TEAM_DEG).any()
    if flaw == "drop_last_mod4":
        assert (ln % 4 == 1).all()
    if flaw == "huge_missing_in_one_part":
        assert (ln > wp.TEAM_DEG).all()
    if flaw == "skip_last_question":
        assert (bad // g.N == g.B - 1).all()
    if flaw == "hub_run_twice":
        assert (np.maximum(g.len0, g.len1)[bad] > wp.HEAVY_DEG).all()


def test_the_other_split_cases_see_a_huge_node_missing_too(fused_refs):
    for name in ("b1_n1024_d200", "ladder_d200"):
        g, dist, P, w, want = fused_refs[name, False]
        assert not np.array_equal(wp.walk_model(g, dist, P, w, flaw="huge_missing_in_one_part"), want), name


def test_case_table_reaches_every_launch_regime():
    want = {"every item split", "full rounds plus a split tail", "no split", "pl=2", "pl=3"}
    for cus in (256, 304):
        got = set()
        for name, gname, D, variant, _, _ in wp.FUSED_CASES:
            if variant != wp.WALK_L2_GATHER:
                g = wp.graph(gname)
                got.add(wp.launch_regime(g.B, g.N, D, variant, cus)["regime"])
        assert got == want, (cus, got)
    assert {c[3] for c in wp.FUSED_CASES} == {wp.WALK_L2_GATHER, wp.WALK_LDS_16, wp.WALK_LDS_32}
    # a wide slice that is partial, a narrow last slice of 8 and of 4 columns
    assert any(c[3] == wp.WALK_LDS_32 and c[2] % 32 for c in wp.FUSED_CASES)
    assert any(c[3] == wp.WALK_LDS_16 and c[2] % 16 == 8 for c in wp.FUSED_CASES)


@pytest.mark.parametrize("I,D", wp.UNFUSED_CASES)
@pytest.mark.parametrize("wts", [False, True])
def test_certificate_of_the_unfused_cases(I, D, wts):
    g, dist, ins, Tf, Ti, w = wp.unfused_data(I, D, wts)
    want = wp.ref_unfused(g, dist, ins, Tf, Ti, w)
    wp.certify_unfused(g, dist, ins, Tf, Ti, w, want)
    assert want.shape == (g.B * g.N, 2 * I * D) and np.abs(want).max() > 0


@pytest.mark.parametrize("wts", [False, True])
def test_certificate_of_the_typelayer_cases(wts):
    g, T, w = wp.typelayer_data(200, wts)
    want = wp.ref_typelayer(g, T, w)
    wp.certify_typelayer(g, T, w, want)
    assert (want > 0).any() and (want == 0).any()


@pytest.mark.parametrize("case", wp.FRONTIER_CASES)
def test_certificate_of_the_frontier_cases(case):
    g, dist, P, w, D = wp.frontier_data(case)
    flag, want = wp.ref_frontier(g, dist, P, w)
    wp.certify_fused(case, g, dist, P, w, want)
    assert flag.any() and not want[~flag].any()                 # rows off the frontier are exact zeros
    if case == "more_seeds_than_the_list":
        assert (dist[0] != 0).sum() > 2048
    if case == "reaches_4097_row":
        assert ((g.len0 + g.len1)[flag] > 4096).any()


@pytest.mark.parametrize("gname,D", wp.BACKWARD_CASES)
def test_certificate_of_the_backward_cases(gname, D):
    g, d = wp.backward_data(gname, D)
    fused, unfused, tl = wp.certify_backward(g, d)
    assert all(np.abs(x).max() > 0 for x in fused + unfused + tuple(tl.values()))


def test_unfused_reference_is_the_autograd_restatement():
    """The numpy references of the unfused walk and of its gradients against the float64 autograd oracle the existing
    backward tests use, on a small graph with full-mantissa data."""
    import torch
    import oracle.rearev_grad as og
    g = wp.graph("relcounts")
    rng = np.random.default_rng(5)
    D, I = 12, 2
    dist, w = wp.random_priors(g, rng), 0.5 + rng.random(g.F)
    Tf, Ti, ins = rng.standard_normal((g.R, D)), rng.standard_normal((g.R, D)), rng.standard_normal((g.B, I, D))
    ga = rng.standard_normal((g.B * g.N, 2 * I * D))
    et = (g.h, g.r, g.t)
    agg, gd, gi, gtf, gti = og.aggregate_grads(et, g.B, g.N, dist.astype(np.float64), ins, Tf, Ti, ga, w)
    np.testing.assert_allclose(wp.ref_unfused(g, dist, ins, Tf, Ti, w), agg, rtol=1e-12, atol=1e-14)
    for got, want in zip(wp.ref_unfused_backward(g, dist, ins, Tf, Ti, ga, w), (gd, gi, gtf, gti)):
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-13)
    gp = rng.standard_normal((g.B * g.N, D))
    np.testing.assert_allclose(wp.ref_typelayer_backward(g, gp, w), og.typelayer_grad(et, g.B, g.N, Tf, gp, w), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(wp.ref_typelayer(g, Tf, w), torch.relu(og.typelayer_pre(et, g.B, g.N, torch.tensor(Tf), w)).numpy(),
                               rtol=1e-12, atol=1e-14)
