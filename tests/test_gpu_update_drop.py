"""gnnrag_update_drop_train / gnnrag_update_drop_backward on the GPU against the float64 oracle (tests/update_drop_oracle.py):
exact integer cases that every kernel form and math mode must reproduce bit for bit, general floats within the kernel rule
or four times the error of the existing entries on a materialised dropped operand, the bits of those entries where the same
kernel form runs, repeatability, ``UpdateDropFn`` under autograd and ``ReasonGNNLayer`` with the switch on and off."""
import numpy as np
import pytest
import torch

import update_drop_oracle as uo

pytestmark = pytest.mark.gpu
TOL_KERNEL, FLOOR = 2e-5, 1e-6
TOL_MODULE, FLOOR_MODULE, TOL_MODULE_FWD = 3e-4, 1e-3, 1e-4
# (BN, D, I): one row; partial tiles, 4 column tiles; 8 column tiles; the trainer's K = 1400, 13 tiles, seven dx column
# blocks; two forward column blocks; the 8-wave form and several gemm_tn chunks; two row tiles per wave
SHAPES = [(1, 4, 1), (70, 52, 2), (130, 68, 1), (260, 200, 3), (33, 212, 1), (32769, 4, 1), (131073, 4, 1)]
PS = [0.0, 0.2, 0.5]
MATHS = [0, 1]
OUTS = ("g_h", "g_agg", "dW", "db")


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


_cache = {}


def _case(shape, p, exact=False):
    """The case and the oracle's results for it: computed once, shared, never written to."""
    key = (shape, p, exact)
    if key not in _cache:
        c = uo.case(*shape, p, seed=5, exact=exact)
        want = dict(pre=uo.forward(c["h"], c["agg"], c["keep"], c["scale"], c["W"], c["b"]))
        want.update(uo.backward(c["g_pre"], c["h"], c["agg"], c["keep"], c["scale"], c["W"]))
        c["xd"] = uo.xd_f32(c["h"], c["agg"], c["keep"], c["scale"])
        for v in list(c.values()) + list(want.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = (c, want)
    return _cache[key]


def _to(dev, c):
    return {k: (torch.tensor(v, device=dev) if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _np(t):
    return t.detach().cpu().numpy()


def _fwd(t, math):
    from gnnrag_amd import ops
    return ops.update_drop_train(t["h"], t["agg"], t["keep"], t["scale"], t["W"], t["b"], math=math)


def _bwd(t, math, **need):
    from gnnrag_amd import ops
    return ops.update_drop_backward(t["g_pre"], t["h"], t["agg"], t["keep"], t["scale"], t["W"], math=math, **need)


def _form_key(f):
    return (f.block_family, f.nt, f.mt, f.nw, f.math, f.v4)


def test_the_shapes_reach_every_form_of_the_new_entries(dev):
    """The dispatch chooses a column-tile count (4, 8, 13), one of three (MT, NW) tile shapes and the math form; the shapes
    above reach every value of each in both math modes, for the forward and for the masked input gradient, and every call
    runs on the k-tiled kernel / the masked gemm_tn."""
    from gnnrag_amd import ops
    for math in MATHS:
        for entry, epi in (("update_drop", ops.DENSE_EPI_LINEAR), ("update_drop_dx", ops.DENSE_EPI_KEEP)):
            seen = set()
            for BN, D, I in SHAPES:
                n = ops.dense_form(entry, BN, D, I, math=math).launches
                for blk in range(n):
                    f = ops.dense_form(entry, BN, D, I, math=math, block=blk)
                    assert f.family == ops.DENSE_KTILED and f.epi == epi and f.v4 == 1 and f.v4out == 1 and f.math == math
                    seen.add((f.nt, f.mt, f.nw))
            assert {s[0] for s in seen} == {4, 8, 13} and {s[1:] for s in seen} == {(1, 4), (1, 8), (2, 4)}, (entry, seen)
        for BN, D, I in SHAPES:
            assert ops.dense_form("update_drop_dw", BN, D, I, math=math).family == ops.DENSE_GEMM_TN
    assert ops.dense_form("update_drop", 33, 212, 1).launches == 2
    assert ops.dense_form("update_drop_dx", 260, 200, 3).launches == 7
    assert ops.dense_form("update_drop", 32769, 4, 1).nw == 8 and ops.dense_form("update_drop", 131073, 4, 1).mt == 2
    lib = ops._lib.load()
    assert lib.gnnrag_gemm_tn_workspace_bytes(32769, 4, 12) > 4 * 12 * 4                     # several gemm_tn chunks


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_integers_equal_the_oracle_bit_for_bit(dev, shape, math):
    """Integers in [-3, 3], p = 0.5 (scale 2): every operand is exact in one bf16 plane and every sum stays below 2^24, so
    every form and math mode must give the oracle's numbers; dropped gradient entries are +0."""
    c, want = _case(shape, 0.5, exact=True)
    assert c["scale"] == 2.0 and max(np.abs(v).max() for v in want.values()) < 2 ** 24
    t = _to(dev, c)
    pre = _np(_fwd(t, math))
    assert np.array_equal(pre.astype(np.float64), want["pre"])
    g = {k: _np(v) for k, v in _bwd(t, math).items()}
    for k in OUTS:
        assert g[k].shape == want[k].shape and np.array_equal(g[k].astype(np.float64), want[k]), k
    D = shape[1]
    gx = np.concatenate([g["g_h"], g["g_agg"]], axis=1)
    dropped = c["keep"] == 0
    assert dropped.any() and not gx[dropped].any() and not np.signbit(gx[dropped]).any()
    assert gx.shape[1] == c["keep"].shape[1] and g["g_h"].shape[1] == D


def _materialised(t, math):
    """What the existing entries give on a materialised dropped operand: gnnrag_linear for pre and for the input gradient
    (against the transposed weight, masked afterwards with one fp32 multiply and a select), gnnrag_gemm_tn for dW."""
    from gnnrag_amd import ops
    D = t["h"].shape[1]
    pre = ops.linear(t["xd"], t["W"], t["b"], math=math)
    Wt = t["W"].t().contiguous()
    parts = [ops.linear(t["g_pre"], Wt[:D].contiguous(), math=math), ops.linear(t["g_pre"], Wt[D:].contiguous(), math=math)]
    if t["keep"] is not None:
        s = torch.tensor(t["scale"], dtype=torch.float32, device=pre.device)
        zero = torch.zeros((), dtype=torch.float32, device=pre.device)
        parts = [torch.where(t["keep"][:, :D] != 0, parts[0] * s, zero), torch.where(t["keep"][:, D:] != 0, parts[1] * s, zero)]
    return dict(pre=pre, g_h=parts[0], g_agg=parts[1], dW=ops.gemm_tn(t["g_pre"], t["xd"]))


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("shape", SHAPES)
def test_general_floats_against_the_oracle(dev, shape, p, math):
    """Bound: the larger of the kernel rule (2e-5 of the tensor's largest entry, floor 1e-6) and 4 x the error gnnrag_linear /
    gnnrag_gemm_tn make on a materialised xd against the same oracle in this run.  db (column sums of g_pre through the
    shared colsum kernel, no product) has the kernel rule alone."""
    c, want = _case(shape, p)
    t = _to(dev, c)
    got = dict(pre=_fwd(t, math))
    got.update(_bwd(t, math))
    ref = _materialised(t, math)
    for k in ("pre",) + OUTS:
        w = want[k]
        scale = max(float(np.abs(w).max()), FLOOR)
        err = float(np.abs(_np(got[k]).astype(np.float64) - w).max())
        rerr = float(np.abs(_np(ref[k]).astype(np.float64) - w).max()) if k in ref else 0.0
        print("%s p %.1f math %d %-5s err/scale %.3e  err/(4 x materialised err) %s"
              % (shape, p, math, k, err / scale, "%.3e" % (err / (4 * rerr)) if rerr else "-"))
        assert err <= max(TOL_KERNEL * scale, 4 * rerr), (k, err, scale, rerr)
    if c["keep"] is not None:
        gx = np.concatenate([_np(got["g_h"]), _np(got["g_agg"])], axis=1)
        assert not gx[c["keep"] == 0].any()


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_same_form_same_bits_as_the_existing_entries(dev, shape, math):
    """Where gnnrag_dense_form reports the same family and template arguments for gnnrag_linear and for the new entry, the
    results carry the bits of gnnrag_linear on the materialised operand; dW always carries those of gnnrag_gemm_tn (the same
    chunks, the same reduce)."""
    from gnnrag_amd import ops
    BN, D, I = shape
    K = (2 * I + 1) * D
    c, _ = _case(shape, 0.2)
    t = _to(dev, c)
    ref = _materialised(t, math)
    g = _bwd(t, math)
    assert _bits(g["dW"]) == _bits(ref["dW"])

    def same(entry, lin_k, lin_n, first, count):
        if ops.dense_form("linear", BN, lin_k, lin_n, math=math).launches != count:
            return False                         # k_gemm_skinny: one launch for every column block
        return all(_form_key(ops.dense_form("linear", BN, lin_k, lin_n, math=math, block=b)) ==
                   _form_key(ops.dense_form(entry, BN, D, I, math=math, block=first + b)) for b in range(count))

    nb_h, nb_agg = (D + 207) // 208, (K - D + 207) // 208
    checks = [("pre", _fwd(t, math), same("update_drop", K, D, 0, nb_h)),
              ("g_h", g["g_h"], same("update_drop_dx", D, D, 0, nb_h)),
              ("g_agg", g["g_agg"], same("update_drop_dx", D, K - D, nb_h, nb_agg))]
    for k, got, eq in checks:
        if BN > 16384:
            assert eq, k                         # above gnnrag_linear's skinny bound both run the k-tiled kernel
        else:
            assert not eq, k                     # below it gnnrag_linear runs k_gemm_skinny: values only (the test above)
        if eq:
            assert _bits(got) == _bits(ref[k]), k


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("shape", [(70, 52, 2), (260, 200, 3), (32769, 4, 1)])
def test_a_second_call_gives_the_same_bits_and_all_ones_equal_no_mask(dev, shape, math):
    c, _ = _case(shape, 0.2)
    t = _to(dev, c)
    a, b = [_fwd(t, math)] + list(_bwd(t, math).values()), [_fwd(t, math)] + list(_bwd(t, math).values())
    for x, y in zip(a, b):
        assert _bits(x) == _bits(y)
    ones = dict(t, keep=torch.ones_like(t["keep"]), scale=1.0)
    none = dict(t, keep=None, scale=1.0)
    for x, y in zip([_fwd(ones, math)] + list(_bwd(ones, math).values()), [_fwd(none, math)] + list(_bwd(none, math).values())):
        assert _bits(x) == _bits(y)
    # a scale handed over without a mask is not applied
    assert _bits(_fwd(dict(none, scale=3.0), math)) == _bits(_fwd(none, math))


def test_an_inf_beside_a_dropped_element_does_not_become_nan(dev):
    c, _ = _case((70, 52, 2), 0.5)
    t = _to(dev, c)
    t["g_pre"] = t["g_pre"].clone()
    t["g_pre"][3, 5] = float("inf")
    g = _bwd(t, 0)
    gx = torch.cat([g["g_h"], g["g_agg"]], dim=1)
    assert not gx[t["keep"] == 0].any()                     # +0 where dropped, the row with the Inf included
    t["h"] = t["h"].clone()
    t["h"][0, :] = float("inf")                              # row 0 is dropped entirely
    pre = _fwd(t, 0)
    assert torch.isfinite(pre).all()


# -- autograd --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,p", [((70, 52, 2), 0.2), ((260, 200, 3), 0.5), ((130, 68, 1), 0.0)])
def test_update_drop_fn_gradients_are_those_of_the_backward_entry(dev, monkeypatch, shape, p):
    from gnnrag_amd import ops
    from gnnrag_amd.autograd import UpdateDropFn
    c, _ = _case(shape, p)
    t = _to(dev, c)
    want = _bwd(t, None)
    calls, inner = [], ops.update_drop_backward

    def counting(*a, **k):
        out = inner(*a, **k)
        calls.append(({n: k[n] for n in ("need_h", "need_agg", "need_dW", "need_db")}, {n: v is not None for n, v in out.items()}))
        return out
    monkeypatch.setattr(ops, "update_drop_backward", counting)
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("h", "agg", "W", "b")}
    pre = UpdateDropFn.apply(leaves["h"], leaves["agg"], t["keep"], t["scale"], leaves["W"], leaves["b"])
    assert _bits(pre) == _bits(_fwd(t, None))
    saved = [s.shape for s in pre.grad_fn.saved_tensors]
    K = t["W"].shape[1]
    # h, agg, W and keep are saved: nothing of the concatenation's size in fp32
    assert sorted(saved) == sorted([t["h"].shape, t["agg"].shape, t["W"].shape] + ([t["keep"].shape] if p else []))
    assert all(s.dtype == torch.uint8 for s in pre.grad_fn.saved_tensors if tuple(s.shape) == (shape[0], K))
    (pre * t["g_pre"]).sum().backward()
    for k, o in (("h", "g_h"), ("agg", "g_agg"), ("W", "dW"), ("b", "db")):
        assert _bits(leaves[k].grad) == _bits(want[o]), k
    assert calls == [(dict(need_h=True, need_agg=True, need_dW=True, need_db=True), dict(g_h=True, g_agg=True, dW=True, db=True))]
    # an output nobody asks for is not computed: its pointer goes to the library as NULL and its launches are not made
    del calls[:]
    W = t["W"].clone().requires_grad_(True)
    pre = UpdateDropFn.apply(t["h"], t["agg"], t["keep"], t["scale"], W, t["b"])
    (pre * t["g_pre"]).sum().backward()
    assert calls == [(dict(need_h=False, need_agg=False, need_dW=True, need_db=False),
                      dict(g_h=False, g_agg=False, dW=True, db=False))]
    assert _bits(W.grad) == _bits(want["dW"])
    del calls[:]
    agg = t["agg"].clone().requires_grad_(True)
    pre = UpdateDropFn.apply(t["h"], agg, t["keep"], t["scale"], t["W"], t["b"])
    (pre * t["g_pre"]).sum().backward()
    assert calls[0][1] == dict(g_h=False, g_agg=True, dW=False, db=False) and _bits(agg.grad) == _bits(want["g_agg"])


# -- the module ------------------------------------------------------------------------------------------------------------

class _FixedDrop(torch.nn.Module):
    """Stands in for ``linear_drop``: the k-th call multiplies by ``scale`` (one fp32 multiply) and zeroes what ``masks[k]``
    drops."""

    def __init__(self, masks, scale):
        super().__init__()
        self.masks, self.scale, self.k = masks, scale, 0

    def forward(self, x):
        m = self.masks[self.k].reshape(x.shape)
        self.k += 1
        return torch.where(m != 0, x * self.scale, torch.zeros((), dtype=x.dtype, device=x.device))


def test_module_with_the_switch_on_matches_the_switch_off_under_the_same_masks(dev, monkeypatch):
    """ReasonGNNLayer in training mode, p = 0.2, B = 3, D = 52, num_ins 2, two layers.  Switch on: the keep draw is replaced
    by fixed masks.  Switch off: ``linear_drop`` is replaced by a stand-in that applies the same masks to h and to agg.  The
    dropout in front of the score function gets one fixed mask per layer in both runs.  Outputs within 1e-4, every parameter
    and input gradient within 3e-4 of its largest entry (floor 1e-3); with the switch unset the new entries are not called."""
    from gnnrag_amd import ops, stack, synth
    cfg = synth.GraphConfig(name="ud", B=3, N=45, E=120, R=9, D=52, I=2, L=2, T=1, n_real_min=5)
    batch, feats, params = synth.make_batch(cfg), synth.make_features(cfg), synth.make_layer_params(cfg)
    B, N, D, I, L, p = cfg.B, cfg.N, cfg.D, cfg.I, cfg.L, 0.2
    K = (2 * I + 1) * D
    scale = 1.0 / (1.0 - p)
    gen = torch.Generator().manual_seed(77)
    keeps = [(torch.rand(B * N, K, generator=gen) >= p).to(torch.uint8).to(dev) for _ in range(L)]
    tails = [(torch.rand(B, N, D, generator=gen) >= p).to(torch.uint8).to(dev) for _ in range(L)]
    Gd = torch.randn(L, B, N, generator=gen).to(dev)
    Gh = torch.randn(B, N, D, generator=gen).to(dev)
    calls = {"fwd": 0, "bwd": 0}
    inner_f, inner_b = ops.update_drop_train, ops.update_drop_backward

    def cf(*a, **k):
        calls["fwd"] += 1
        return inner_f(*a, **k)

    def cb(*a, **k):
        calls["bwd"] += 1
        return inner_b(*a, **k)
    monkeypatch.setattr(ops, "update_drop_train", cf)
    monkeypatch.setattr(ops, "update_drop_backward", cb)
    monkeypatch.delenv("GNNRAG_HIP_LAYER_TAIL_TRAIN", raising=False)

    def run(on):
        layer = stack.build_layer(cfg, batch, params, dev).train()
        layer.linear_dropout = p
        if on:
            monkeypatch.setenv("GNNRAG_HIP_UPDATE_DROP_TRAIN", "1")
            draws = iter(keeps)
            layer._draw_update_keep = lambda rows, cols, pp, device: next(draws)
            layer.linear_drop = _FixedDrop(tails, scale)
        else:
            monkeypatch.delenv("GNNRAG_HIP_UPDATE_DROP_TRAIN", raising=False)
            seq = []
            for j in range(L):
                seq += [keeps[j][:, :D], keeps[j][:, D:], tails[j]]
            layer.linear_drop = _FixedDrop(seq, scale)
        inp = {k: torch.tensor(feats[k], device=dev, requires_grad=True) for k in ("h0", "rel_features", "rel_features_inv", "ins")}
        layer.init_reason(local_entity=torch.from_numpy(batch.local_entity).to(dev), kb_adj_mat=batch.edge_tuple,
                          local_entity_emb=inp["h0"], rel_features=inp["rel_features"],
                          rel_features_inv=inp["rel_features_inv"],
                          query_entities=torch.from_numpy(batch.query_entities).float().to(dev))
        dist = torch.from_numpy(batch.seed_dist).float().to(dev)
        loss, outs = 0.0, []
        for j in range(L):
            dist, h = layer(dist, inp["ins"][0], step=j)
            outs += [dist.detach().cpu().numpy(), h.detach().cpu().numpy()]
            loss = loss + (dist * Gd[j]).sum()
        (loss + (h * Gh).sum()).backward()
        assert layer.linear_drop.k == len(layer.linear_drop.masks)
        grads = {k: v.grad.cpu().numpy() for k, v in inp.items()}
        grads.update({k: q.grad.cpu().numpy() for k, q in layer.named_parameters() if q.grad is not None})
        return outs, grads

    outs_off, grads_off = run(False)
    assert calls == {"fwd": 0, "bwd": 0}                      # switch unset: no call to the new entries
    outs_on, grads_on = run(True)
    assert calls == {"fwd": L, "bwd": L}
    for a, b in zip(outs_on, outs_off):
        assert np.abs(a - b).max() <= TOL_MODULE_FWD
    assert set(grads_on) == set(grads_off) and {"e2e_linear0.weight", "e2e_linear1.bias", "rel_linear0.weight", "h0", "ins"} <= set(grads_on)
    for k in grads_off:
        want = grads_off[k]
        err, bound = float(np.abs(grads_on[k] - want).max()), TOL_MODULE * max(float(np.abs(want).max()), FLOOR_MODULE)
        print("%-24s max|diff| %.3e  bound %.3e" % (k, err, bound))
        assert err <= bound, k
