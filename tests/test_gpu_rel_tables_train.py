"""gnnrag_relation_tables_backward on the GPU against the float64 oracle of its four formulas
(tests/rel_tables_grad_oracle.py): integer cases bit for bit in both math modes and every kernel form the shapes reach,
general floats within the project's kernel bound (2e-5 of each tensor's largest entry, floor 1e-6: test_gpu_backward.py /
test_gpu_update_drop.py), the exact zeros the header promises, the same bits twice, NULL outputs; then
``autograd.RelationTablesFn`` and the switch ``GNNRAG_HIP_REL_TABLES_TRAIN`` in ``ReasonGNNLayer`` against the gradients
recorded from the reference (tests/golden/grad_layer_*.npz)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import rel_tables_grad_oracle as ro
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
TOL_KERNEL = 2e-5
TOL_MODULE = 3e-4
OUTS = ("g_T_fwd", "g_T_inv", "g_ins", "g_W")

# name -> GraphConfig fields; each reaches another corner
SHAPES = {
    "one": dict(B=1, N=8, E=3, R=1, D=4, I=1, self_loop=False),                      # one question, one relation: M = 1
    "d52": dict(B=4, N=40, E=90, R=7, D=52, I=3, n_real_min=5),                      # tiny50-like: partial column tiles
    "d68": dict(B=2, N=33, E=150, R=5, D=68, I=1),
    "tiny": None,                                                                    # D = 200, I = 2
    "d212": dict(B=2, N=40, E=160, R=4, D=212, I=1),                                 # more than one output column block
    "tinyfb": None,                                                                  # 1500 relations, 40 per question
    # about 1000 relations per question: rel_total just above the skinny kernel's 16384 rows, several gemm_tn chunks
    "big": dict(B=17, N=64, E=8000, R=1000, D=4, I=1, zipf_heads=False),
    "noq": dict(B=4, N=24, E=60, R=6, D=8, I=2),                                     # question 2 loses its facts
}
EMPTY_Q = 2


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _structure(name):
    """(plan, rows, cfg): built once per module."""
    from gnnrag_amd import ops, synth
    cfg = synth.CONFIGS[name] if SHAPES[name] is None else synth.GraphConfig(name=name, seed=11, **SHAPES[name])
    et = synth.make_batch(cfg).edge_tuple
    h, r, t = (np.asarray(et[k]).astype(np.int64) for k in range(3))
    if name == "noq":
        keep = (h // cfg.N) != EMPTY_Q
        h, r, t = h[keep], r[keep], t[keep]
    plan = ops.CsrPlan(h, r, t, cfg.B, cfg.N, cfg.R1, torch.device("cuda", 0))
    rows = plan.rel_rows().astype(np.int64)
    assert len(rows) == plan.rel_total > 0
    return plan, rows, cfg


@functools.lru_cache(maxsize=None)
def _reference(name, exact):
    """(case, oracle gradients, bound of the partial sums): computed once, shared by the tests, never changed."""
    plan, rows, cfg = _structure(name)
    lim = 3
    while True:
        c = ro.case(rows, cfg.R1, cfg.B, cfg.D, cfg.I, seed=7, exact=exact, lim=lim)
        bound = ro.largest_sum(rows, cfg.R1, cfg.B, c)
        if not exact or bound < 2 ** 24 or lim == 1:
            break
        lim -= 1                                   # a smaller integer range where the sums would leave fp32's integers
    want = ro.backward(rows, cfg.R1, cfg.B, c["T_fwd"], c["T_inv"], c["ins"], c["W"], c["g_P"])
    for v in list(c.values()) + list(want.values()):
        v.setflags(write=False)
    return c, want, bound


def _call(dev, plan, c, math, **need):
    from gnnrag_amd import ops
    t = {k: torch.tensor(v, device=dev) for k, v in c.items()}
    return ops.relation_tables_backward(plan, t["T_fwd"], t["T_inv"], t["ins"], t["W"], t["g_P"], math=math, **need)


def _bits(x):
    return x.detach().cpu().contiguous().numpy().tobytes()


def _assert_exact_zeros(got, rows, cfg, name):
    unused = np.setdiff1d(np.arange(cfg.R1), rows[:, 1])
    assert cfg.R1 - 1 in unused                                     # the padding row of the tables has no facts
    z = lambda a: not a.cpu().numpy().view(np.int32).any()          # noqa: E731  (+0: every bit clear)
    assert z(got["g_T_fwd"][unused]) and z(got["g_T_inv"][unused]), "rows of unused relations"
    assert z(got["g_W"][:, :cfg.D]), "the self block of g_W"
    no_rows = np.setdiff1d(np.arange(cfg.B), rows[:, 0])
    if name == "noq":
        assert list(no_rows) == [EMPTY_Q]
    assert z(got["g_ins"][no_rows]), "g_ins of a question without facts"


def _assert_form(name, M, D, I, math):
    """The kernel the product in front of the gate runs: the skinny kernel up to 16384 rows, the k-tiled one above (bf16x3
    unless exact fp32 is asked for); the weight gradient on k_gemm_tn with more than one chunk for the large shape."""
    from gnnrag_amd import _lib, ops
    f = ops.dense_form("rel_tables_dx", M, D, I, math=math)
    if name == "big":
        assert 16384 < M < 16384 + 2048
        assert f.family == ops.DENSE_KTILED and f.math == (math != 0) and f.v4 == 1
        assert _lib.load().gnnrag_gemm_tn_workspace_bytes(M, D, I * D) > 4 * D * I * D * 4          # several chunks
    else:
        assert M <= 16384 and f.family == ops.DENSE_SKINNY
    assert ops.dense_form("rel_tables_dw", M, D, I, math=math).family == ops.DENSE_GEMM_TN


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_integer_cases_equal_the_oracle_bit_for_bit(dev, name, math):
    plan, rows, cfg = _structure(name)
    c, want, bound = _reference(name, True)
    assert bound < 2 ** 24, "an oracle sum leaves the integers fp32 holds exactly"
    if name == "one":
        assert plan.rel_total == 1
    _assert_form(name, plan.rel_total, cfg.D, cfg.I, math)
    got = _call(dev, plan, c, math)
    for k in OUTS:
        w = want[k].astype(np.float32)
        assert np.array_equal(w.astype(np.float64), want[k]) and not (np.signbit(w) & (w == 0)).any()      # no -0
        g = got[k].cpu().numpy()
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (k, float(np.abs(g - w).max()))
    _assert_exact_zeros(got, rows, cfg, name)
    again = _call(dev, plan, c, math)
    assert all(_bits(got[k]) == _bits(again[k]) for k in OUTS)


@pytest.mark.parametrize("math", [0, 1, 2])
@pytest.mark.parametrize("name", list(SHAPES))
def test_general_floats_stay_within_the_kernel_bound(dev, name, math):
    plan, rows, cfg = _structure(name)
    c, want, _ = _reference(name, False)
    got = _call(dev, plan, c, math)
    for k in OUTS:
        err, scale = np.abs(got[k].cpu().numpy() - want[k]).max(), max(np.abs(want[k]).max(), 1e-6)
        print("%s math %d %s: error %.3g of %.3g (%.3g relative)" % (name, math, k, err, scale, err / scale))
        assert err <= TOL_KERNEL * scale, (k, err, scale)
    _assert_exact_zeros(got, rows, cfg, name)
    again = _call(dev, plan, c, math)
    assert all(_bits(got[k]) == _bits(again[k]) for k in OUTS), "two calls differ"


@pytest.mark.parametrize("name", ["d52", "tiny", "big", "noq"])
def test_null_outputs_are_honoured(dev, name):
    """Each output alone, and the two table gradients without the others: the same bits as with all four wanted."""
    plan, rows, cfg = _structure(name)
    c, _, _ = _reference(name, False)
    full = _call(dev, plan, c, 1)
    flags = dict(g_T_fwd="need_T_fwd", g_T_inv="need_T_inv", g_ins="need_ins", g_W="need_W")
    for wanted in [(k,) for k in OUTS] + [("g_T_fwd", "g_T_inv"), ("g_ins", "g_W")]:
        got = _call(dev, plan, c, 1, **{flags[k]: k in wanted for k in OUTS})
        for k in OUTS:
            if k in wanted:
                assert _bits(got[k]) == _bits(full[k]), (wanted, k)
            else:
                assert got[k] is None
    from gnnrag_amd import _lib
    with pytest.raises(_lib.GnnragError):
        _call(dev, plan, c, 1, **{f: False for f in flags.values()})


def test_an_empty_batch_zero_fills_every_wanted_output(dev):
    from gnnrag_amd import ops
    z = np.zeros(0, np.int64)
    B, N, R1, D, I = 2, 8, 3, 16, 2
    plan = ops.CsrPlan(z, z, z, B, N, R1, dev)
    assert plan.rel_total == 0
    assert ops._lib.load().gnnrag_relation_tables_backward_workspace_bytes(ctypes.byref(plan.c), D, I) == 0
    g = torch.Generator().manual_seed(2)
    r = lambda *sh: torch.randn(*sh, generator=g).to(dev)          # noqa: E731
    got = ops.relation_tables_backward(plan, r(R1, D), r(R1, D), r(B, I, D), r(D, (2 * I + 1) * D), torch.zeros(2, 0, D, device=dev))
    assert [tuple(got[k].shape) for k in OUTS] == [(R1, D), (R1, D), (B, I, D), (D, (2 * I + 1) * D)]
    for k in OUTS:
        assert not got[k].cpu().numpy().view(np.int32).any(), k
    only = ops.relation_tables_backward(plan, r(R1, D), r(R1, D), r(B, I, D), r(D, (2 * I + 1) * D),
                                        torch.zeros(2, 0, D, device=dev), need_T_fwd=False, need_T_inv=False, need_W=False)
    assert only["g_W"] is None and not only["g_ins"].cpu().numpy().view(np.int32).any()


@pytest.mark.parametrize("name", ["d52", "tinyfb", "big"])
def test_the_autograd_function_is_the_two_library_calls(dev, name):
    """Forward: the bits of ops.relation_tables (what inference computes); backward: the bits of
    ops.relation_tables_backward; an input that needs no gradient gets none."""
    from gnnrag_amd import ops
    from gnnrag_amd.autograd import RelationTablesFn
    plan, rows, cfg = _structure(name)
    c, _, _ = _reference(name, False)
    t = {k: torch.tensor(v, device=dev) for k, v in c.items()}
    leaf = {k: t[k].clone().requires_grad_(True) for k in ("T_fwd", "T_inv", "ins", "W")}
    P = RelationTablesFn.apply(plan, leaf["T_fwd"], leaf["T_inv"], leaf["ins"], leaf["W"])
    assert _bits(P) == _bits(ops.relation_tables(plan, t["T_fwd"], t["T_inv"], t["ins"], t["W"]))
    (P * t["g_P"]).sum().backward()
    want = ops.relation_tables_backward(plan, t["T_fwd"], t["T_inv"], t["ins"], t["W"], t["g_P"])
    for k, o in (("T_fwd", "g_T_fwd"), ("T_inv", "g_T_inv"), ("ins", "g_ins"), ("W", "g_W")):
        assert leaf[k].grad is not None and _bits(leaf[k].grad) == _bits(want[o]), k
    # an expanded (stride-0) upstream gradient, and only the instructions asking
    ins = t["ins"].clone().requires_grad_(True)
    RelationTablesFn.apply(plan, t["T_fwd"], t["T_inv"], ins, t["W"]).sum().backward()
    ones = ops.relation_tables_backward(plan, t["T_fwd"], t["T_inv"], t["ins"], t["W"], torch.ones_like(t["g_P"]),
                                        need_T_fwd=False, need_T_inv=False, need_W=False)
    assert _bits(ins.grad) == _bits(ones["g_ins"])


def _close(got, want, tol, msg, floor=1e-6):
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * max(np.abs(want).max(), floor), err_msg=msg)


@pytest.mark.parametrize("name", ["layer_d200.npz", "layer_d50.npz"])
def test_module_gradients_match_reference_fixture_with_the_tables_on_the_library(dev, monkeypatch, name):
    """test_gpu_backward.test_module_gradients_match_reference_fixture (fused form, same bounds) with
    GNNRAG_HIP_REL_TABLES_TRAIN=1: at D = 200 every layer call takes RelationTablesFn and the torch expression is never
    called; D = 50 falls through to the unfused form as before."""
    from gnnrag_amd import autograd, stack
    from gnnrag_amd.modules.kg_reasoning import reasongnn as rg
    monkeypatch.setenv("GNNRAG_HIP_REL_TABLES_TRAIN", "1")

    def no_torch_tables(*a, **k):
        raise AssertionError("relation_tables_dense was called with the switch on")
    monkeypatch.setattr(rg, "relation_tables_dense", no_torch_tables)
    calls = []
    inner = autograd.RelationTablesFn.apply
    monkeypatch.setattr(rg.RelationTablesFn, "apply", staticmethod(lambda *a: (calls.append(1), inner(*a))[1]))

    cfg, batch, feats, params, ref = load_golden(name)
    z = np.load(os.path.join(GOLDEN, "grad_" + name))
    layer = stack.build_layer(cfg, batch, params, dev).train()
    layer.train_fused = True
    inp = {k: torch.tensor(feats[k], device=dev, requires_grad=True)
           for k in ("h0", "rel_features", "rel_features_inv", "ins")}
    layer.init_reason(local_entity=torch.from_numpy(batch.local_entity).to(dev), kb_adj_mat=batch.edge_tuple,
                      local_entity_emb=inp["h0"], rel_features=inp["rel_features"],
                      rel_features_inv=inp["rel_features_inv"],
                      query_entities=torch.from_numpy(batch.query_entities).float().to(dev))
    seed = torch.from_numpy(batch.seed_dist).float().to(dev)
    Gd = torch.from_numpy(z["cot.Gd"]).to(dev)
    Gh = torch.from_numpy(z["cot.Gh"]).to(dev)
    loss, c = 0.0, 0
    for t in range(cfg.T):
        dist = seed
        for j in range(cfg.L):
            dist, h = layer(dist, inp["ins"][t], step=j)
            assert np.abs(dist.detach().cpu().numpy() - ref["dist"][c]).max() <= 1e-4      # forward parity too
            loss = loss + (dist * Gd[c]).sum()
            c += 1
    loss = loss + (h * Gh).sum()
    loss.backward()
    assert len(calls) == (cfg.T * cfg.L if cfg.D % 4 == 0 else 0)
    assert abs(loss.item() - float(z["loss"])) <= 1e-4 * max(1.0, abs(float(z["loss"])))
    got = {k: v.grad for k, v in inp.items()}
    got.update({k: p.grad for k, p in layer.named_parameters() if p.grad is not None})
    names = [k[5:] for k in z.files if k.startswith("grad.")]
    for k in names:
        assert k in got and got[k] is not None, "no gradient for " + k
        # floor: score_func.bias has a mathematically zero gradient (softmax is shift invariant)
        _close(got[k].cpu().numpy(), z["grad." + k], TOL_MODULE, k, floor=1e-3)
