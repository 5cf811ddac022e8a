"""gnnrag_layer_tail_train / gnnrag_layer_tail_backward on the MI355X against the float64 oracle (tests/layer_tail_oracle.py),
through ``ops``, ``autograd.LayerTailFn`` and ``ReasonGNNLayer`` with ``GNNRAG_HIP_LAYER_TAIL_TRAIN=1``.

Bounds: live scores, ``g_pre`` and ``dw`` within 2e-5 of the larger of their tensor's largest entry and 1e-6 (the project's
kernel rule, ``TOL_KERNEL``), ``dist`` within 2e-5 absolute (``TOL_FWD``); at module level the bounds of
``test_module_gradients_match_reference_fixture`` (3e-4 with floor 1e-3, forward 1e-4).  Everything else is equality of
values or of bits."""
import os

import numpy as np
import pytest
import torch

import layer_tail_oracle as lo
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
TOL_KERNEL = 2e-5
TOL_FWD = 2e-5
TOL_MODULE = 3e-4

# (B, N, D): the smallest case; D % 4 != 0 and N over a wave; the trainer's hidden size; D % 4 == 0 but no multiple of 64; a
# second float4 round per row (D > 256); N over a 1024-thread workgroup (k_lt_gs strides, the softmax takes two items per
# thread); 6150 rows: more rows than the backward's grid has waves, so its workgroups walk several rows each, write 1024
# partial rows, and the reduce adds them in 16 slices of 64 (asserted below through the workspace size - no further shape is
# needed for that with kLtBwdGrid = 1024 and four rows per workgroup)
SHAPES = [(1, 1, 1), (3, 70, 50), (2, 130, 200), (4, 64, 52), (2, 65, 260), (2, 1030, 8), (3, 2050, 20)]


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _to(dev, c):
    return {k: (torch.tensor(v, device=dev) if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _close(got, want, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    err, scale = float(np.abs(got - want).max()), max(float(np.abs(want).max()), 1e-6)
    print("%-8s max|diff| %.3e  scale %.3e  ratio %.3e" % (what, err, scale, err / scale))
    assert err <= TOL_KERNEL * scale, (what, err, scale)


def _fwd(t):
    from gnnrag_amd import ops
    return ops.layer_tail_train(t["pre_a"], t["pre_b"], t["keep"], t["scale"], t["w"], t["b"], t["mask"])


def _bwd(t, h, dist, g_h="g_h", g_dist="g_dist", **need):
    from gnnrag_amd import ops
    return ops.layer_tail_backward(h, dist, t["keep"], t["scale"], t["w"], t[g_h] if g_h else None,
                                   t[g_dist] if g_dist else None, **need)


_oracle_cache = {}


def _case(B, N, D, p, with_b, seed=11):
    """The case and the oracle's results for it: computed once, shared, never written to."""
    key = (B, N, D, p, with_b, seed)
    if key not in _oracle_cache:
        c = lo.case(B, N, D, seed=seed, p=p, with_b=with_b)
        h, s, score, dist = lo.forward(c["pre_a"], c["pre_b"], c["keep"], c["scale"], c["w"], c["b"], c["mask"])
        want = dict(h=h, s=s, score=score, dist=dist)
        want.update(lo.backward(h, dist, c["keep"], c["scale"], c["w"], c["g_h"], c["g_dist"]))
        for v in list(c.values()) + list(want.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _oracle_cache[key] = (c, want)
    return _oracle_cache[key]


@pytest.mark.parametrize("with_b", [True, False], ids=["ab", "a"])
@pytest.mark.parametrize("p", [0.0, 0.2, 0.5])
@pytest.mark.parametrize("B,N,D", SHAPES)
def test_forward_and_backward_against_the_oracle(dev, B, N, D, p, with_b):
    from gnnrag_amd import ops
    c, want = _case(B, N, D, p, with_b)
    mask, live = c["mask"], c["mask"] != 0
    pre = c["pre_a"] + c["pre_b"] if with_b else c["pre_a"]
    if B > 1:                                                   # what the generator promises
        assert (mask.sum(1) < N).all() and not mask[B - 1].any() and (mask.sum(1) == 1).any()
        assert 0.4 < (pre < 0).mean() < 0.6 and (pre == 0).any()
        assert (c["keep"] is None) == (p == 0)
    if (B, N, D) == SHAPES[-1]:
        rows = B * N
        al = lambda x: (x + 255) // 256 * 256                   # noqa: E731
        assert rows // 4 > 1024                                 # more workgroups' worth of rows than the capped grid
        assert ops._lib.load().gnnrag_layer_tail_backward_workspace_bytes(B, N, D) == al(rows * 4) + al(1024 * D * 4)
    t = _to(dev, c)
    h, score, dist = _fwd(t)
    assert tuple(h.shape) == (B * N, D) and tuple(score.shape) == (B, N) and tuple(dist.shape) == (B, N)
    assert np.array_equal(h.cpu().numpy(), np.maximum(pre, np.float32(0)))
    sc = score.cpu().numpy()
    s_err, s_scale = np.abs(sc[live].astype(np.float64) - want["s"][live]).max(), max(np.abs(want["s"][live]).max(), 1e-6)
    print("score    max|diff| %.3e  scale %.3e  ratio %.3e" % (s_err, s_scale, s_err / s_scale))
    assert s_err <= TOL_KERNEL * s_scale
    assert (sc[~live] == np.float32(-1e11)).all()
    d = dist.cpu().numpy()
    d_err = float(np.abs(d - want["dist"]).max())
    print("dist     max|diff| %.3e" % d_err)
    assert d_err <= TOL_FWD
    if B > 1:
        assert (d[B - 1] == np.float32(1) / np.float32(N)).all()        # the fully padded question
    assert _bits(dist) == _bits(ops.masked_softmax(score, B, N))

    # the backward reads the h and dist the forward just wrote, as autograd.LayerTailFn hands them over
    g = _bwd(t, h, dist)
    _close(g["g_pre"], want["g_pre"], "g_pre")
    _close(g["dw"], want["dw"], "dw")
    assert tuple(g["db"].shape) == (1,) and float(g["db"].item()) == 0.0 and not np.signbit(g["db"].cpu().numpy()).any()
    assert not g["g_pre"].cpu().numpy()[h.cpu().numpy() == 0].any()
    if B > 1:
        assert g["g_pre"][(B - 1) * N:].abs().max().item() > 0          # the padded question passes a gradient
    # a second call: the same bits
    h2, score2, dist2 = _fwd(t)
    g2 = _bwd(t, h2, dist2)
    assert _bits(h2) == _bits(h) and _bits(score2) == _bits(score) and _bits(dist2) == _bits(dist)
    assert all(_bits(g2[k]) == _bits(g[k]) for k in ("g_pre", "dw", "db"))


@pytest.mark.parametrize("B,N,D,p", [(3, 70, 50, 0.2), (2, 130, 200, 0.5), (2, 65, 260, 0.0)])
def test_absent_upstream_gradients_and_unwanted_outputs(dev, B, N, D, p):
    from gnnrag_amd import _lib, ops
    c, _ = _case(B, N, D, p, True)
    t = _to(dev, c)
    h, _, dist = _fwd(t)
    full = _bwd(t, h, dist)
    # g_dist None: gs = 0
    g = _bwd(t, h, dist, g_dist=None)
    assert torch.equal(g["g_pre"], (h > 0) * t["g_h"])
    assert not g["dw"].cpu().numpy().any() and float(g["db"].item()) == 0.0
    # g_h None: the run with a zero g_h
    t0 = dict(t, zero=torch.zeros_like(t["g_h"]))
    g = _bwd(t, h, dist, g_h=None)
    z = _bwd(t0, h, dist, g_h="zero")
    assert torch.equal(g["g_pre"], z["g_pre"]) and torch.equal(g["dw"], z["dw"])
    # both None: refused
    with pytest.raises(_lib.GnnragError) as e:
        ops.layer_tail_backward(h, dist, t["keep"], t["scale"], t["w"], None, None)
    assert "(-1)" in str(e.value)
    for need in (dict(need_dw=False), dict(need_db=False), dict(need_dw=False, need_db=False)):
        g = _bwd(t, h, dist, **need)
        assert (g["dw"] is None) == (not need.get("need_dw", True)) and (g["db"] is None) == (not need.get("need_db", True))
        assert _bits(g["g_pre"]) == _bits(full["g_pre"])
        assert g["dw"] is None or _bits(g["dw"]) == _bits(full["dw"])


@pytest.mark.parametrize("B,N,D,p", [(3, 70, 50, 0.2), (4, 64, 52, 0.5), (3, 2050, 20, 0.0)])
def test_a_question_alone_gives_the_bits_of_its_rows_in_the_batch(dev, B, N, D, p):
    c, _ = _case(B, N, D, p, True)
    t = _to(dev, c)
    h, score, dist = _fwd(t)
    g = _bwd(t, h, dist)
    for b in range(B):
        rows = slice(b * N, (b + 1) * N)
        one = dict(t, mask=t["mask"][b:b + 1], g_dist=t["g_dist"][b:b + 1])
        for k in ("pre_a", "pre_b", "keep", "g_h"):
            one[k] = None if t[k] is None else t[k][rows]
        h1, score1, dist1 = _fwd(one)
        g1 = _bwd(one, h1, dist1)
        assert _bits(h1) == _bits(h[rows]) and _bits(score1[0]) == _bits(score[b]) and _bits(dist1[0]) == _bits(dist[b]), b
        assert _bits(g1["g_pre"]) == _bits(g["g_pre"][rows]), b


def _shifted(x):
    """The same values at a base pointer offset by one element (4 bytes for floats: no 16-byte alignment)."""
    flat = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    out = flat[1:].view(x.shape)
    out.copy_(x)
    assert out.is_contiguous() and out.data_ptr() == flat.data_ptr() + x.element_size()
    return out


@pytest.mark.parametrize("B,N,D,p", [(2, 130, 200, 0.2), (4, 64, 52, 0.0), (2, 65, 260, 0.5)])
def test_unaligned_bases_take_the_element_form_and_give_the_same_values(dev, B, N, D, p):
    assert D % 4 == 0
    c, _ = _case(B, N, D, p, True)
    t = _to(dev, c)
    h, score, dist = _fwd(t)
    g = _bwd(t, h, dist)
    for which in (("pre_a",), ("pre_b",), ("w",), ("keep",), ("pre_a", "pre_b", "w", "g_h", "keep")):
        u = dict(t)
        for k in which:
            if t[k] is not None:
                u[k] = _shifted(t[k])
        hu, su, du = _fwd(u)
        assert torch.equal(hu, h) and torch.equal(su, score) and torch.equal(du, dist), which
        gu = _bwd(u, _shifted(h) if len(which) > 1 else h, dist)
        assert torch.equal(gu["g_pre"], g["g_pre"]) and torch.equal(gu["dw"], g["dw"]), which


def _torch_tail(t, leaves):
    """The expression written out in fp32 torch ops, with the same keep flags (reasongnn.py:163-169)."""
    a, pb, w, b = leaves
    B, N = t["mask"].shape
    h = torch.relu(a if pb is None else a + pb)
    x = h if t["keep"] is None else h * t["keep"].float() * t["scale"]
    score = torch.nn.functional.linear(x, w, b).view(B, N) + (1 - t["mask"]) * -100000000000
    return h, score, torch.softmax(score, dim=1)


@pytest.mark.parametrize("use", ["both", "h", "dist"])
@pytest.mark.parametrize("B,N,D,p,with_b", [(3, 70, 50, 0.2, True), (2, 130, 200, 0.0, True), (4, 64, 52, 0.5, False)])
def test_layer_tail_fn_against_torch_autograd(dev, B, N, D, p, with_b, use):
    from gnnrag_amd.autograd import LayerTailFn
    c, _ = _case(B, N, D, p, with_b)
    t = _to(dev, c)

    def leaves():
        return (t["pre_a"].clone().requires_grad_(True), t["pre_b"].clone().requires_grad_(True) if with_b else None,
                t["w"].clone().view(1, D).requires_grad_(True), t["b"].clone().requires_grad_(True))

    def loss(h, dist):
        out = 0.0
        if use in ("both", "h"):
            out = out + (h * t["g_h"]).sum()
        if use in ("both", "dist"):
            out = out + (dist * t["g_dist"]).sum()
        return out

    want = leaves()
    h_w, score_w, dist_w = _torch_tail(t, want)
    loss(h_w, dist_w).backward()
    got = leaves()
    h, score, dist = LayerTailFn.apply(got[0], got[1], t["keep"], t["scale"], got[2], got[3], t["mask"])
    assert not score.requires_grad and h.requires_grad and dist.requires_grad
    loss(h, dist).backward()
    h_w, score_w, dist_w = h_w.detach(), score_w.detach(), dist_w.detach()
    assert torch.equal(h.detach(), h_w) and float((dist.detach() - dist_w).abs().max()) <= TOL_FWD
    live = t["mask"] != 0
    assert torch.equal(score[~live], score_w[~live])
    _close(score[live], score_w[live].cpu().numpy().astype(np.float64), "score")
    names = ("pre_a", "pre_b", "w", "b")
    for k, x, y in zip(names, got, want):
        if x is None:
            continue
        if use == "h" and k in ("w", "b"):                       # dist was not used: torch leaves them without a gradient
            assert y.grad is None and (x.grad is None or not x.grad.cpu().numpy().any()), k
            continue
        assert x.grad is not None and x.grad.shape == x.shape, k
        if k == "b":
            assert float(x.grad.item()) == 0.0                  # torch's own: rounding residue of a zero
            continue
        _close(x.grad, y.grad.cpu().numpy().astype(np.float64), "d" + k)
    if with_b:
        assert torch.equal(got[0].grad, got[1].grad)


# -- the module, switch on -------------------------------------------------------------------------------------------------

def _counted(monkeypatch):
    from gnnrag_amd import ops
    calls, inner = [], ops.layer_tail_train

    def counting(pre_a, pre_b, keep, *a, **k):
        calls.append((pre_b is not None, keep is not None))
        return inner(pre_a, pre_b, keep, *a, **k)
    monkeypatch.setattr(ops, "layer_tail_train", counting)
    return calls


def _mclose(got, want, tol, msg, floor=1e-6):
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * max(np.abs(want).max(), floor), err_msg=msg)


@pytest.mark.parametrize("form", ["fused", "unfused"])
@pytest.mark.parametrize("name", ["layer_d200.npz", "layer_d50.npz"])
def test_module_gradients_match_reference_fixture_with_the_tail_on_the_library(dev, monkeypatch, name, form):
    """The body of test_gpu_backward.py::test_module_gradients_match_reference_fixture with the switch set, same bounds; every
    layer call must have ended in the library's tail: the fused form and the native unfused form at D = 200 (two
    pre-activations), the nn.Linear form at D = 50 (one)."""
    from gnnrag_amd import stack
    monkeypatch.setenv("GNNRAG_HIP_LAYER_TAIL_TRAIN", "1")
    calls = _counted(monkeypatch)
    cfg, batch, feats, params, ref = load_golden(name)
    z = np.load(os.path.join(GOLDEN, "grad_" + name))
    layer = stack.build_layer(cfg, batch, params, dev).train()
    layer.train_fused = form == "fused"
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
    assert calls == [(cfg.D % 4 == 0, False)] * (cfg.T * cfg.L)
    loss.backward()
    assert abs(loss.item() - float(z["loss"])) <= 1e-4 * max(1.0, abs(float(z["loss"])))
    got = {k: v.grad for k, v in inp.items()}
    got.update({k: p.grad for k, p in layer.named_parameters() if p.grad is not None})
    names = [k[5:] for k in z.files if k.startswith("grad.")]
    for k in names:
        assert k in got and got[k] is not None, "no gradient for " + k
        # floor: score_func.bias has a mathematically zero gradient (softmax is shift invariant)
        _mclose(got[k].cpu().numpy(), z["grad." + k], TOL_MODULE, k, floor=1e-3)
    assert float(layer.score_func.bias.grad.abs().max()) == 0.0
    assert len(layer.possible_cand) == cfg.T * cfg.L


def test_return_score_and_the_unset_switch_stay_on_torch(dev, monkeypatch):
    from gnnrag_amd import stack
    calls = _counted(monkeypatch)
    cfg, batch, feats, params, _ = load_golden("layer_d200.npz")
    layer = stack.build_layer(cfg, batch, params, dev).train()
    devin = stack.DeviceInputs(batch, feats, dev)

    def run(**kw):
        layer.init_reason(local_entity=devin.local_entity, kb_adj_mat=batch.edge_tuple, local_entity_emb=devin.h0,
                          rel_features=devin.rel_features, rel_features_inv=devin.rel_features_inv,
                          query_entities=devin.query_entities)
        return layer(devin.seed_dist, devin.ins[0], step=0, **kw)

    monkeypatch.delenv("GNNRAG_HIP_LAYER_TAIL_TRAIN", raising=False)
    dist_off, h_off = run()
    monkeypatch.setenv("GNNRAG_HIP_LAYER_TAIL_TRAIN", "0")
    run()
    monkeypatch.setenv("GNNRAG_HIP_LAYER_TAIL_TRAIN", "1")
    score, dist_rs = run(return_score=True)
    assert calls == []
    dist_on, h_on = run()
    assert calls == [(True, False)]
    assert torch.equal(h_on, h_off) and float((dist_on - dist_off).detach().abs().max()) <= TOL_FWD
    assert torch.equal(dist_rs, dist_off) and tuple(score.shape) == tuple(dist_off.shape)


def test_training_mode_with_dropout_runs_on_the_tail_and_is_stochastic(dev, monkeypatch):
    """linear_dropout = 0.2 in training mode with the switch set (the body of
    test_training_mode_with_dropout_runs_and_is_stochastic): finite outputs, gradients for every used parameter, two passes
    differ, and every layer call ended in the library's tail with keep flags."""
    from gnnrag_amd import stack
    monkeypatch.setenv("GNNRAG_HIP_LAYER_TAIL_TRAIN", "1")
    calls = _counted(monkeypatch)
    cfg, batch, feats, params, _ = load_golden("layer_d200.npz")
    layer = stack.build_layer(cfg, batch, params, dev).train()
    layer.linear_dropout = 0.2
    layer.linear_drop.p = 0.2
    devin = stack.DeviceInputs(batch, feats, dev)
    outs = []
    for rep in range(2):
        layer.zero_grad()
        layer.init_reason(local_entity=devin.local_entity, kb_adj_mat=batch.edge_tuple, local_entity_emb=devin.h0,
                          rel_features=devin.rel_features, rel_features_inv=devin.rel_features_inv,
                          query_entities=devin.query_entities)
        dist = devin.seed_dist
        for j in range(cfg.L):
            dist, h = layer(dist, devin.ins[0], step=j)
        (dist * dist).sum().backward()
        assert torch.isfinite(dist).all()
        for k, p in layer.named_parameters():
            if k.startswith(("rel_linear", "e2e_linear", "score_func")):
                assert p.grad is not None and torch.isfinite(p.grad).all(), k
        outs.append(dist.detach().cpu().numpy())
    assert np.abs(outs[0] - outs[1]).max() > 0
    assert calls == [(True, True)] * (2 * cfg.L)
