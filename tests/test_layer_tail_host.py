"""The tail of the reasoning layer under autograd, host side: the float64 oracle of the GPU tests
(tests/layer_tail_oracle.py) reproduces the scores and distributions the live reference recorded (``ref.h`` / ``ref.score`` /
``ref.dist`` of tests/golden/layer_d50.npz and layer_d200.npz) and equals torch's float64 autograd of the expression
written out; the entry points are declared in gnnrag.h and in the binding (additive to ABI 16) and refuse bad arguments
before they touch a device; ``GNNRAG_HIP_LAYER_TAIL_TRAIN`` is read at every call, defaults to off, and - unset or set - leaves
a layer on CPU tensors under autograd the torch form bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

import layer_tail_oracle as lo
from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_FIXTURE = 2e-6
TOL_F64 = 1e-12


@pytest.mark.parametrize("name,calls", [("layer_d50.npz", 4), ("layer_d200.npz", 6)])
def test_oracle_forward_reproduces_the_recorded_reference_calls(name, calls):
    """``ref.h[c]`` goes in as pre_a (relu is idempotent on it): live scores within 2e-6 of the largest live score, masked
    scores equal exactly, distributions within 2e-6."""
    cfg, batch, _, params, ref = load_golden(name)
    mask = (batch.local_entity != batch.num_entity).astype(np.float32)
    B, N, D = cfg.B, cfg.N, cfg.D
    assert ref["h"].shape == (calls, B, N, D)
    if name == "layer_d50.npz":
        assert (mask.sum(1) == 0).any()                          # a question with no live node
    live = mask != 0
    for c in range(calls):
        h, _, score, dist = lo.forward(ref["h"][c].reshape(B * N, D), None, None, 1.0, params["score_func.weight"],
                                       params["score_func.bias"], mask)
        assert np.array_equal(h, ref["h"][c].reshape(B * N, D).astype(np.float64))
        want = ref["score"][c]
        scale = float(np.abs(want[live]).max())
        err = float(np.abs(score[live].astype(np.float64) - want[live]).max())
        derr = float(np.abs(dist - ref["dist"][c]).max())
        print("%s call %d: score %.3e of %.3e (%.3e)  dist %.3e" % (name, c, err, scale, err / scale, derr))
        assert err <= TOL_FIXTURE * scale
        assert np.array_equal(score[~live], want[~live]) and (score[~live] == np.float32(-1e11)).all()
        assert derr <= TOL_FIXTURE


class _MaskAddFp32(torch.autograd.Function):
    """``(s.float() + (1 - mask) * -1e11).double()``: the reference's fp32 addition inside a float64 graph.  Its derivative
    with respect to s is 1; written as a Function because autograd's own ``.float()`` / ``.double()`` pair would round the
    gradient passing through it to fp32 (8e-9 on the case below)."""

    @staticmethod
    def forward(ctx, s, mask):
        return (s.float() + (1 - mask) * -100000000000).double()

    @staticmethod
    def backward(ctx, g):
        return g, None


def _written_out(c, use_keep, use_b, use_gh, use_gd):
    """Torch's float64 autograd of the expression; the mask term is added in fp32 (through ``.float()``), as the oracle does."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)      # noqa: E731
    a, w, b = t(c["pre_a"]), t(c["w"]), t(c["b"])
    pb = t(c["pre_b"]) if use_b else None
    pre = a if pb is None else a + pb
    h = torch.relu(pre)
    x = h
    if use_keep:
        x = h * torch.tensor(c["keep"].astype(np.float64) * float(np.float32(c["scale"])))
    mask = torch.tensor(c["mask"])
    B, N = mask.shape
    s = (x @ w + b).view(B, N)
    score = _MaskAddFp32.apply(s, mask)
    dist = torch.softmax(score, dim=1)
    loss = 0.0
    if use_gh:
        loss = loss + (h * torch.tensor(c["g_h"].astype(np.float64))).sum()
    if use_gd:
        loss = loss + (dist * torch.tensor(c["g_dist"].astype(np.float64))).sum()
    loss.backward()
    return h.detach().numpy(), dist.detach().numpy(), a.grad, (None if pb is None else pb.grad), w.grad, b.grad


@pytest.mark.parametrize("use_keep", [False, True])
@pytest.mark.parametrize("use_b", [False, True])
@pytest.mark.parametrize("use_gh,use_gd", [(True, True), (False, True), (True, False)])
def test_oracle_against_float64_autograd(use_keep, use_b, use_gh, use_gd):
    B, N, D = 3, 7, 5
    c = lo.case(B, N, D, seed=5, p=0.4, with_b=True)
    assert not c["mask"][B - 1].any() and c["mask"][0].sum() == 1           # a fully padded question among them
    # multiples of 2^-10: the oracle's one fp32 addition pre_a + pre_b is then exact, as autograd's float64 one is
    for k in ("pre_a", "pre_b"):
        c[k] = (np.round(c[k] * 1024) / 1024).astype(np.float32)
    assert ((c["pre_a"] + c["pre_b"]) == 0).any()
    keep, scale = (c["keep"], c["scale"]) if use_keep else (None, 1.0)
    h64, dist64, ga, gb, gw, gbias = _written_out(c, use_keep, use_b, use_gh, use_gd)
    h, _, _, dist = lo.forward(c["pre_a"], c["pre_b"] if use_b else None, keep, scale, c["w"], c["b"], c["mask"])
    assert np.array_equal(h, h64)
    assert np.abs(dist - dist64).max() <= TOL_F64
    got = lo.backward(h, dist, keep, scale, c["w"], c["g_h"] if use_gh else None, c["g_dist"] if use_gd else None)
    errs = [np.abs(got["g_pre"] - ga.numpy()).max()]
    if use_b:
        errs.append(np.abs(got["g_pre"] - gb.numpy()).max())
    if use_gd:
        errs.append(np.abs(got["dw"] - gw.numpy()).max())
        print("g_pre / dw errors %s, autograd's db %.3e" % (errs, float(gbias)))
        assert abs(float(gbias)) <= 1e-15 and got["db"] == 0.0               # autograd's db: rounding residue
        assert np.abs(got["g_pre"][(B - 1) * N:]).max() > 0                  # the padded question passes a gradient
    else:
        assert not got["dw"].any() and (gw is None or not gw.numpy().any())
    assert max(errs) <= TOL_F64


# -- the entry points ------------------------------------------------------------------------------------------------------

SYMBOLS = {"gnnrag_layer_tail_train": 14, "gnnrag_layer_tail_backward_workspace_bytes": 3, "gnnrag_layer_tail_backward": 16}


def test_header_binding_and_python_layers_declare_the_tail():
    from gnnrag_amd import _lib, autograd, ops
    from gnnrag_amd.modules.kg_reasoning.reasongnn import ReasonGNNLayer
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gnnrag.h")).read(), flags=re.S)
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "gnnrag.h does not declare " + name
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    assert re.search(r"#define\s+GNNRAG_ABI_VERSION\s+16\b", src) and _lib.ABI_VERSION == 16
    assert re.search(r"#define\s+GNNRAG_LAYER_TAIL_MAX_D\s+4096\b", src) and ops.LAYER_TAIL_MAX_D == 4096
    for fn in (ops.layer_tail_train, ops.layer_tail_backward, ops.layer_tail_supported, autograd.LayerTailFn.apply,
               ReasonGNNLayer._layer_tail):
        assert callable(fn)
    assert "layer_tail.hip" in __import__("gnnrag_amd.build", fromlist=["SOURCES"]).SOURCES
    ok = ops.layer_tail_supported
    assert ok(1) and ok(50) and ok(4096) and not ok(4097) and not ok(0)


@pytest.fixture(scope="module")
def lib():
    from gnnrag_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.gnnrag_abi_version() == 16
    return lib


def _train(lib, B=2, N=5, D=4, **null):
    v = dict(pre_a=4096, pre_b=4096, keep=4096, w=4096, b=4096, mask=4096, h=4096, score=4096, dist=4096)
    v.update(null)
    return lib.gnnrag_layer_tail_train(v["pre_a"], v["pre_b"], v["keep"], 1.25, v["w"], v["b"], v["mask"], B, N, D, v["h"],
                                       v["score"], v["dist"], None)


def _backward(lib, B=2, N=5, D=4, ws=4096, ws_bytes=0, **null):
    v = dict(h=4096, dist=4096, keep=4096, w=4096, g_h=4096, g_dist=4096, g_pre=4096, dw=4096, db=4096)
    v.update(null)
    return lib.gnnrag_layer_tail_backward(v["h"], v["dist"], v["keep"], 1.25, v["w"], v["g_h"], v["g_dist"], B, N, D,
                                          v["g_pre"], v["dw"], v["db"], ws, ws_bytes, None)


def test_bad_arguments_are_refused_before_anything_is_launched(lib):
    """Every pointer is a dummy non-NULL address and there is no device here: each answer comes from the argument checks (a
    call that passed them would fault on the dummy addresses, so every call below is one that must not pass)."""
    for k in ("pre_a", "w", "b", "mask", "h", "score", "dist"):
        assert _train(lib, **{k: None}) == -1, k
    assert _train(lib, B=0) == -1 and _train(lib, N=-1) == -1 and _train(lib, D=0) == -1
    assert _train(lib, D=4097) == -2 and _train(lib, B=1 << 16, N=1 << 15) == -2
    assert _train(lib, pre_b=None, keep=None, D=4097) == -2                 # the optional ones are optional
    need = lib.gnnrag_layer_tail_backward_workspace_bytes(2, 5, 4)
    assert need >= 2 * 5 * 4 + 3 * 4 * 4
    for B, N, D in ((0, 5, 4), (2, 0, 4), (2, 5, 0), (2, 5, 4097), (1 << 16, 1 << 15, 4), (-1, 5, 4)):
        assert lib.gnnrag_layer_tail_backward_workspace_bytes(B, N, D) == 0
    assert lib.gnnrag_layer_tail_backward_workspace_bytes(1 << 15, (1 << 16) - 1, 4) > 0       # B N = 2^31 - 2^15
    for k in ("h", "dist", "w", "g_pre"):
        assert _backward(lib, ws_bytes=need, **{k: None}) == -1, k
    assert _backward(lib, ws_bytes=need, g_h=None, g_dist=None) == -1
    assert _backward(lib, ws_bytes=need, B=0) == -1 and _backward(lib, ws_bytes=need, D=-3) == -1
    assert _backward(lib, ws_bytes=1 << 30, D=4097) == -2 and _backward(lib, ws_bytes=1 << 30, B=1 << 16, N=1 << 15) == -2
    assert _backward(lib, ws=None, ws_bytes=need) == -3 and _backward(lib, ws_bytes=need - 1) == -3
    assert _backward(lib, ws_bytes=0, keep=None, dw=None, db=None, g_h=None) == -3


def test_the_wrappers_refuse_cpu_tensors():
    from gnnrag_amd import _lib, ops
    c = lo.case(2, 3, 4, seed=0, p=0.5)
    t = {k: (None if v is None or isinstance(v, float) else torch.from_numpy(v)) for k, v in c.items()}
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.layer_tail_train(t["pre_a"], t["pre_b"], t["keep"], c["scale"], t["w"], t["b"], t["mask"])
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.layer_tail_backward(t["pre_a"], t["mask"], t["keep"], c["scale"], t["w"], t["g_h"], t["g_dist"])


# -- the module layer ------------------------------------------------------------------------------------------------------

class _Plan:
    rel_total = 0


def _cpu_layer(D, I, R, B, N, p):
    from gnnrag_amd.modules.kg_reasoning.reasongnn import ReasonGNNLayer
    torch.manual_seed(4)
    args = dict(use_cuda=False, normalized_gnn=False, num_ins=I, num_gnn=1, pos_emb=False, linear_dropout=p)
    layer = ReasonGNNLayer(args, 1000, R, D, "bfs").train()
    g = torch.Generator().manual_seed(9)
    layer.batch_size, layer.max_local_entity, layer.plan = B, N, _Plan()
    layer.rel_features = torch.randn(R, D, generator=g)
    layer.rel_features_inv = torch.randn(R, D, generator=g)
    layer.local_entity_mask = (torch.rand(B, N, generator=g) < 0.7).float()
    layer.possible_cand = []
    return layer, g


def _fake_aggregate(plan, dist, ins, T_fwd, T_inv):
    """Stands in for AggregateFn.apply (a HIP call): any differentiable [B*N, 2 I D] function of the same inputs."""
    B, I, D = ins.shape
    N = dist.shape[1]
    parts = []
    for i in range(I):
        for T in (T_fwd, T_inv):
            parts.append(dist.reshape(B, N, 1) * (ins[:, i] * T[i % T.shape[0]]).reshape(B, 1, D))
    return torch.cat(parts, dim=2).reshape(B * N, 2 * I * D)


def _torch_form(layer, h0, dist, ins, drop):
    """``_forward_autograd`` on its nn.Linear branch as it stood before the switch existed, written out."""
    from gnnrag_amd.modules.kg_reasoning import reasongnn as rg
    B, N, D = layer.batch_size, layer.max_local_entity, layer.entity_dim
    T_fwd, T_inv = layer.rel_linear0(layer.rel_features.float()), layer.rel_linear0(layer.rel_features_inv.float())
    agg = _fake_aggregate(layer.plan, dist.float(), ins.float(), T_fwd, T_inv)
    state = torch.cat((h0.float(), agg.view(B, N, -1)), dim=2)
    h = torch.nn.functional.relu(layer.e2e_linear0(drop(state)))
    score = layer.score_func(drop(h)).squeeze(dim=2) + (1 - layer.local_entity_mask) * rg.VERY_NEG_NUMBER
    return layer.softmax_d1(score), h


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_the_switch_defaults_to_off_is_read_per_call_and_leaves_cpu_tensors_on_the_torch_form(monkeypatch, p):
    from gnnrag_amd import ops
    from gnnrag_amd.modules.kg_reasoning import reasongnn as rg
    D, I, R, B, N = 8, 2, 5, 3, 6
    layer, g = _cpu_layer(D, I, R, B, N, p)
    monkeypatch.setattr(rg.AggregateFn, "apply", staticmethod(_fake_aggregate))

    def no_library(*a, **k):
        raise AssertionError("the library was called on CPU tensors")
    monkeypatch.setattr(ops, "layer_tail_train", no_library)
    tail_calls = []
    inner = rg.ReasonGNNLayer._layer_tail

    def spy(self, *a, **k):
        got = inner(self, *a, **k)
        tail_calls.append((os.environ.get("GNNRAG_HIP_LAYER_TAIL_TRAIN"), got is None))
        return got
    monkeypatch.setattr(rg.ReasonGNNLayer, "_layer_tail", spy)
    h0 = torch.randn(B, N, D, generator=g)
    dist0 = torch.softmax(torch.randn(B, N, generator=g), dim=1)
    ins = torch.randn(B, I, D, generator=g)

    def run(fn):
        layer.zero_grad(set_to_none=True)
        a, b, c = h0.clone().requires_grad_(True), dist0.clone().requires_grad_(True), ins.clone().requires_grad_(True)
        torch.manual_seed(21)                                   # the same dropout draws in every run
        dist, h = fn(a, b, c)
        ((dist * dist).sum() + (h * h).sum()).backward()
        return [dist.detach(), h.detach(), a.grad, b.grad, c.grad] + [q.grad for q in layer.parameters()]

    def module(a, b, c):
        layer.local_entity_emb = a
        return layer(b, c, step=0)

    want = run(lambda a, b, c: _torch_form(layer, a, b, c, layer.linear_drop))
    for value in (None, "0", "1", None):
        if value is None:
            monkeypatch.delenv("GNNRAG_HIP_LAYER_TAIL_TRAIN", raising=False)
        else:
            monkeypatch.setenv("GNNRAG_HIP_LAYER_TAIL_TRAIN", value)
        got = run(module)
        assert len(got) == len(want)
        for x, y in zip(got, want):
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), value
    # one look at the switch per layer call; every call stayed on torch (CPU tensors are not eligible)
    assert tail_calls == [(None, True), ("0", True), ("1", True), (None, True)]
    assert layer.score_func.weight.grad is not None and layer.e2e_linear0.weight.grad is not None
