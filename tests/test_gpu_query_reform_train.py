"""gnnrag_query_reform_train / gnnrag_query_reform_backward on the MI355X against the float64 oracle
(tests/query_reform_grad_oracle.py), through ``ops``, ``autograd.QueryReformFn`` and the bound ``QueryReform`` modules.

Bounds: forward within 2e-5 absolute (``TOL_FWD`` of test_gpu_instruction.py); every gradient within 2e-5 of the larger of
its tensor's largest entry and 1e-6 (the project's kernel rule, ``TOL_KERNEL``).  Everything else is equality of bits."""
import copy

import numpy as np
import pytest
import torch

import query_reform_grad_oracle as qo

pytestmark = pytest.mark.gpu
TOL_FWD = 2e-5
TOL_KERNEL = 2e-5

# (B, N, D, n): the smallest case; D % 4 != 0 and N over one 64-lane ballot round; the trainer's hidden size; D % 4 == 0
# but no multiple of 64; D beyond 256 threads; the maximum n
SHAPES = [(1, 1, 1, 1), (3, 70, 50, 3), (2, 130, 200, 2), (4, 64, 52, 2), (2, 65, 260, 1), (5, 9, 130, 8)]


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _to(dev, c):
    to = lambda a: [torch.from_numpy(x).to(dev) for x in a] if isinstance(a, list) else torch.from_numpy(a).to(dev)  # noqa: E731
    return {k: to(v) for k, v in c.items()}


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _close(got, want, what):
    got = got.detach().cpu().numpy()
    err, scale = float(np.abs(got - want).max()), max(float(np.abs(want).max()), 1e-6)
    print("%-12s max|diff| %.3e  scale %.3e  ratio %.3e" % (what, err, scale, err / scale))
    assert err <= TOL_KERNEL * scale, (what, err, scale)


def _run(t, g_outs=None, need=None, idx=None):
    """Forward and backward over the reforms ``idx`` (default: all); (out, grads)."""
    from gnnrag_amd import ops
    idx = list(range(len(t["qs"]))) if idx is None else idx
    qs, W_rs, W_gs = ([t[k][j] for j in idx] for k in ("qs", "W_rs", "W_gs"))
    out, reserve = ops.query_reform_train(qs, t["seed"], t["ent"], W_rs, W_gs)
    g_outs = [t["G"][j] for j in idx] if g_outs is None else g_outs
    return out, ops.query_reform_backward(qs, t["seed"], W_rs, W_gs, reserve, g_outs, need=need)


@pytest.mark.parametrize("B,N,D,n", SHAPES)
def test_forward_and_backward_against_the_oracle(dev, B, N, D, n):
    from gnnrag_amd import ops
    c = qo.train_case(B, N, D, n, seed=11)
    seed = c["seed"]
    if B > 1:
        assert not seed[B - 1].any() and (seed[0] != 0).sum() == 2 and seed[0, N - 1] == 1.0 and 0.5 in seed[0]
    t = _to(dev, c)
    want_out, saved = qo.forward(c["qs"], seed, c["ent"], c["W_rs"], c["W_gs"])
    want = qo.backward(saved, list(c["G"]))
    out, g = _run(t)
    assert tuple(out.shape) == (n, B, D)
    err = float(np.abs(out.cpu().numpy() - want_out).max())
    print("out          max|diff| %.3e" % err)
    assert err <= TOL_FWD
    for j in range(n):
        single = ops.query_reform(t["qs"][j], t["seed"], t["ent"], t["W_rs"][j], t["W_gs"][j])
        assert _bits(out[j]) == _bits(single), "out[%d] is not the inference launch's bits" % j
        for k in ("dq", "dW_r", "dW_g"):
            _close(g[k][j], want[k][j], "%s[%d]" % (k, j))
    _close(g["d_ent"], want["d_ent"], "d_ent")
    d_ent = g["d_ent"].cpu().numpy()
    assert d_ent.shape == (B, N, D)
    assert not d_ent[seed == 0].any()                          # exactly zero on every row without a flag
    if B > 1:
        assert not d_ent[B - 1].any()                           # a question without a seed
    # a second call: the same bits
    out2, g2 = _run(t)
    assert _bits(out2) == _bits(out) and _bits(g2["d_ent"]) == _bits(g["d_ent"])
    for k in ("dq", "dW_r", "dW_g"):
        for j in range(n):
            assert _bits(g2[k][j]) == _bits(g[k][j]), (k, j)


def test_an_unused_reform_is_left_out(dev):
    B, N, D, n = 3, 70, 50, 3
    t = _to(dev, qo.train_case(B, N, D, n, seed=12))
    _, g = _run(t, g_outs=[t["G"][0], None, t["G"][2]])
    _, two = _run(t, idx=[0, 2])
    assert g["dq"][1] is None and g["dW_r"][1] is None and g["dW_g"][1] is None
    for k in ("dq", "dW_r", "dW_g"):
        assert _bits(g[k][0]) == _bits(two[k][0]) and _bits(g[k][2]) == _bits(two[k][1]), k
    assert _bits(g["d_ent"]) == _bits(two["d_ent"])


def test_need_subsets_skip_outputs(dev):
    B, N, D, n = 3, 70, 50, 3
    t = _to(dev, qo.train_case(B, N, D, n, seed=13))
    _, full = _run(t)
    _, g = _run(t, need={"dq": [True, False, True], "dW_r": False, "dW_g": [False, True, False], "d_ent": False})
    assert g["d_ent"] is None and g["dq"][1] is None and all(x is None for x in g["dW_r"])
    assert g["dW_g"][0] is None and g["dW_g"][2] is None
    assert _bits(g["dq"][0]) == _bits(full["dq"][0]) and _bits(g["dq"][2]) == _bits(full["dq"][2])
    assert _bits(g["dW_g"][1]) == _bits(full["dW_g"][1])
    _, g = _run(t, need={"d_ent": True})
    assert all(x is None for k in ("dq", "dW_r", "dW_g") for x in g[k]) and _bits(g["d_ent"]) == _bits(full["d_ent"])
    _, g = _run(t, need={"dW_r": True})                         # the weight gradients alone: no transposed products
    assert g["d_ent"] is None and all(_bits(a) == _bits(b) for a, b in zip(g["dW_r"], full["dW_r"]))


def test_a_question_alone_and_the_reforms_one_by_one_give_the_same_bits(dev):
    """``dq`` and ``d_ent`` of a question do not depend on the batch around it; ``out``, ``dq``, ``dW`` of a reform do not
    depend on the reforms beside it.  For ``d_ent`` the three single-reform results are added on the host in fp32 in j order
    and must EQUAL the one call's bits: the kernel computes seed * ((dy_0 + dy_1) + dy_2), the host (seed dy_0 + seed dy_1) +
    seed dy_2, and the seed weights of the case are 1 and 0.5 - a power of two scales every term and every partial sum
    exactly (no result here is near the subnormal range), so both round at the same places to the same values."""
    B, N, D, n = 4, 64, 52, 3
    c = qo.train_case(B, N, D, n, seed=14)
    assert set(np.unique(c["seed"]).tolist()) == {0.0, 0.5, 1.0}
    t = _to(dev, c)
    out, g = _run(t)
    for b in (0, 2):
        alone = _to(dev, dict(qs=[q[b:b + 1] for q in c["qs"]], W_rs=c["W_rs"], W_gs=c["W_gs"], seed=c["seed"][b:b + 1],
                              ent=c["ent"][b:b + 1], G=c["G"][:, b:b + 1]))
        out1, g1 = _run(alone)
        assert _bits(out1[:, 0]) == _bits(out[:, b])
        assert _bits(g1["d_ent"][0]) == _bits(g["d_ent"][b])
        for j in range(n):
            assert _bits(g1["dq"][j][0]) == _bits(g["dq"][j][b]), (b, j)
    d_ent = None
    for j in range(n):
        outj, gj = _run(t, idx=[j])
        assert _bits(outj[0]) == _bits(out[j])
        for k in ("dq", "dW_r", "dW_g"):
            assert _bits(gj[k][0]) == _bits(g[k][j]), (k, j)
        d_ent = gj["d_ent"] if d_ent is None else d_ent + gj["d_ent"]
    assert _bits(d_ent) == _bits(g["d_ent"])


def test_a_padded_node_state_is_read_in_place(dev):
    from gnnrag_amd import ops
    B, N, D, n, ld = 3, 70, 50, 2, 56
    c = qo.train_case(B, N, D, n, seed=15, ld=ld)
    t = _to(dev, c)
    padded = t["ent"]
    view = padded[:, :, :D]
    assert not view.is_contiguous()
    same, stride = ops._ent_in_place(view, B, N)
    assert same.data_ptr() == padded.data_ptr() and stride == ld
    want, _ = ops.query_reform_train(t["qs"], t["seed"], view.contiguous(), t["W_rs"], t["W_gs"])
    for ent in (view, padded):
        out, _ = ops.query_reform_train(t["qs"], t["seed"], ent, t["W_rs"], t["W_gs"])
        assert _bits(out) == _bits(want)
    want_out, _ = qo.forward(c["qs"], c["seed"], c["ent"], c["W_rs"], c["W_gs"])
    assert float(np.abs(want.cpu().numpy() - want_out).max()) <= TOL_FWD


# -- the modules, switch on ----------------------------------------------------------------------------------------------

def _counted(monkeypatch):
    from gnnrag_amd import ops
    calls, inner = [], ops.query_reform_train

    def counting(qs, *a, **k):
        calls.append(len(qs))
        return inner(qs, *a, **k)
    monkeypatch.setattr(ops, "query_reform_train", counting)
    return calls


def _inputs(dev, c, dtype, iters=2):
    ins0 = [torch.from_numpy(q).to(dev, dtype).requires_grad_(True) for q in c["qs"]]
    ents = [torch.from_numpy(c["ent"] * (1.0 - 0.25 * i)).to(dev, dtype).requires_grad_(True) for i in range(iters)]
    return ins0, ents, torch.from_numpy(c["seed"]).to(dev, dtype), torch.ones(c["seed"].shape, device=dev, dtype=dtype)


def _loss(outs):
    return sum((o * (k + 1)).sum() for k, o in enumerate(outs))


def _grads(model, ins0, ents):
    named = [("ins%d" % j, t.grad) for j, t in enumerate(ins0)] + [("ent%d" % i, t.grad) for i, t in enumerate(ents)]
    return named + [(k, p.grad) for k, p in model.named_parameters()]


def _model_pair(dev, D, n):
    from gnnrag_amd.modules import query_update as mq
    torch.manual_seed(7)
    model = mq.bind_reforms(qo.standin(D, n).to(dev))
    return model, copy.deepcopy(model).double()


def _compare(model, wide, ins0, ents, ins64, ents64):
    for (k, got), (k64, want) in zip(_grads(model, ins0, ents), _grads(wide, ins64, ents64)):
        assert k == k64 and (got is None) == (want is None), k
        if got is not None:
            _close(got, want.cpu().numpy(), k)


def test_bound_reforms_make_one_call_per_iteration(dev, monkeypatch):
    monkeypatch.setenv("GNNRAG_HIP_QUERY_REFORM_TRAIN", "1")
    B, N, D, n = 3, 70, 50, 3
    c = qo.train_case(B, N, D, n, seed=16)
    model, wide = _model_pair(dev, D, n)
    calls = _counted(monkeypatch)
    ins0, ents, seed, mask = _inputs(dev, c, torch.float32)
    outs = model.loop(ins0, ents, seed, mask)
    assert calls == [n, n]                                      # one call per iteration, all reforms in it
    _loss(outs).backward()
    ins64, ents64, seed64, mask64 = _inputs(dev, c, torch.float64)
    outs64 = wide.loop(ins64, ents64, seed64, mask64)           # float64 is not eligible: the torch form
    assert calls == [n, n]
    _loss(outs64).backward()
    for j in range(n):
        assert float((outs[j].detach().double() - outs64[j].detach()).abs().max()) <= TOL_FWD
        assert getattr(model, "reform%d" % j).q_ent_attn.weight.grad is None
    _compare(model, wide, ins0, ents, ins64, ents64)


def test_a_foreign_node_state_gets_a_single_call_and_a_copy_binds_to_itself(dev, monkeypatch):
    monkeypatch.setenv("GNNRAG_HIP_QUERY_REFORM_TRAIN", "1")
    B, N, D, n = 3, 70, 50, 3
    c = qo.train_case(B, N, D, n, seed=17)
    model, wide = _model_pair(dev, D, n)
    twin = copy.deepcopy(model)
    assert twin.reform0._qr_bound is twin.reform2._qr_bound and twin.reform0._qr_bound is not model.reform0._qr_bound
    assert twin.reform0._qr_bound.instruction is twin.instruction
    calls = _counted(monkeypatch)

    def round_(m, ins0, ents, seed, mask):
        m.instruction.instructions = [t.unsqueeze(1) for t in ins0]
        outs = []
        for j in range(n):
            ent = ents[0].clone() if j == 1 else ents[0]        # reform 1 sees a clone of the node state
            outs.append(getattr(m, "reform%d" % j)(m.instruction.instructions[j].squeeze(1), ent, seed, mask))
        return outs

    ins0, ents, seed, mask = _inputs(dev, c, torch.float32, iters=1)
    outs = round_(model, ins0, ents, seed, mask)
    assert calls == [n, 1]                                      # all reforms at reform 0, a single call for reform 1
    _loss(outs).backward()
    ins64, ents64, seed64, mask64 = _inputs(dev, c, torch.float64, iters=1)
    _loss(round_(wide, ins64, ents64, seed64, mask64)).backward()
    _compare(model, wide, ins0, ents, ins64, ents64)
    # the copy runs on its own bound state and leaves the original's kept outputs alone
    kept = model.reform0._qr_bound.kept
    del calls[:]
    ins1, ents1, _, _ = _inputs(dev, c, torch.float32, iters=1)
    outs1 = twin.loop(ins1, ents1, seed, mask)
    assert calls == [n] and model.reform0._qr_bound.kept is kept and twin.reform0._qr_bound.kept is not None
    assert all(_bits(a) == _bits(b) for a, b in zip(outs1, model.loop(ins0, ents, seed, mask)))
    # an unbound module always makes single calls
    from gnnrag_amd.modules.query_update import QueryReform
    del calls[:]
    lone = QueryReform(D).to(dev)
    lone(ins0[0], ents[0], seed, mask).sum().backward()
    assert calls == [1] and lone.fusion.r.weight.grad is not None and lone.q_ent_attn.weight.grad is None


def test_switch_off_never_calls_the_library(dev, monkeypatch):
    B, N, D, n = 3, 70, 50, 3
    c = qo.train_case(B, N, D, n, seed=18)
    model, _ = _model_pair(dev, D, n)
    calls = _counted(monkeypatch)
    for value in (None, "0"):
        if value is None:
            monkeypatch.delenv("GNNRAG_HIP_QUERY_REFORM_TRAIN", raising=False)
        else:
            monkeypatch.setenv("GNNRAG_HIP_QUERY_REFORM_TRAIN", value)
        ins0, ents, seed, mask = _inputs(dev, c, torch.float32)
        _loss(model.loop(ins0, ents, seed, mask)).backward()
        assert calls == [] and ents[0].grad is not None
