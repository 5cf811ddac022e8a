"""The training form of instruction generation on the MI355X: gnnrag_instructions_train / gnnrag_instructions_backward,
autograd.InstructionsFn and a patched module under autograd with GNNRAG_HIP_INSTRUCTION_TRAIN=1.

Truth: the float64 oracle with explicit dropout multipliers (tests/instruction_grad_oracle.py), which the host tests hold
against the live reference's autograd.  Tolerance of every gradient tensor: the project's kernel rule (test_gpu_backward._close,
TOL_KERNEL) ``|diff| <= 2e-5 * max(max|want|, 1e-6)`` - torch's own fp32 autograd stays within 6.1e-7 of that scale on these
shapes, so the bound leaves about 30x over an fp32 reference.  ins / attn with multipliers: 2e-5 absolute, the bound of
tests/test_gpu_instruction.py (values in [-1, 1]).  db_ca is exactly 0.

The module tests start from the encoder's fp32 LSTM states - device and truth do not see equal inputs - and, in the second
round, from weights that carry the first round's gradient error: they are held to TOL_MODULE (3e-4) with plain SGD, for the
reasons tests/test_gpu_lstm_train.py writes down.  Where the oracle is given the device's own token states (the fixed-mask
test) the inputs are equal and the kernel rule applies."""
import copy
import functools

import numpy as np
import pytest
import torch

import instruction_grad_oracle as igo
import instruction_oracle as io

pytestmark = pytest.mark.gpu

TOL_KERNEL = 2e-5          # test_gpu_backward.py
TOL_MODULE = 3e-4          # test_gpu_lstm_train.py
TOL_FWD = 2e-5             # test_gpu_instruction.py

# (B, T, D, n, p): the smallest; D % 4 != 0 (padded copies) without and with multipliers; the encoder's shape; D % 4 == 0 but
# no multiple of 64; T over 64 lanes at the maximum step count; one step, D over two waves' worth of lanes, half dropped
SHAPES = [(1, 1, 1, 1, 0.0), (3, 5, 50, 3, 0.0), (3, 5, 50, 3, 0.2), (2, 12, 200, 2, 0.2), (4, 7, 52, 2, 0.2),
          (2, 70, 64, 8, 0.0), (5, 3, 130, 1, 0.5)]
FLAT = ("dhidden", "dnode", "dr_in", "dW_cq", "db_cq", "dw_ca")


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(shape):
    return igo.train_case(*shape, seed=sum(int(10 * v) for v in shape))


@functools.lru_cache(maxsize=None)
def _truth(shape, with_r, with_ga):
    """float64 forward and gradients of a case (computed once, never changed)."""
    c = _case(shape)
    ins, attn, saved = igo.forward(*[c[k] for k in io.ARGS], r_in=c["r_in"] if with_r else None, m1=c["m1"], m2=c["m2"],
                                   m3=c["m3"])
    return ins, attn, igo.backward(saved, c["g_ins"], c["g_attn"] if with_ga else None)


def _to(dev, a):
    if a is None:
        return None
    return [torch.from_numpy(x).to(dev) for x in a] if isinstance(a, list) else torch.from_numpy(a).to(dev)


def _close(got, want, tol, msg, floor=1e-6):
    got = got.detach().cpu().numpy().astype(np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, msg
    err, scale = np.abs(got - want).max(), max(np.abs(want).max(), floor)
    print("%-34s max|diff| %.3e  scale %.3e  ratio %.3e" % (msg, err, scale, err / scale))
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * scale, err_msg=msg)


def _check_grads(got, want, tag, tol=TOL_KERNEL):
    for k in FLAT:
        if got[k] is not None:
            _close(got[k], want[k], tol, "%s %s" % (tag, k))
    for k in ("dW_q", "db_q"):
        for s, t in enumerate(got[k]):
            if t is not None:
                _close(t, want[k][s], tol, "%s %s[%d]" % (tag, k, s))
    assert got["db_ca"] is None or (tuple(got["db_ca"].shape) == (1,) and float(got["db_ca"][0]) == 0.0)


def _same(a, b):
    for k in igo.GRADS:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            assert (x is None and y is None) or torch.equal(x, y), k


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_T%d_D%d_n%d_p%g" % s)
def test_forward_and_gradients_against_the_float64_oracle(dev, shape):
    from gnnrag_amd import ops
    B, T, D, n, p = shape
    assert ops.instructions_backward_supported(T, D, n)
    c = _case(shape)
    t = {k: _to(dev, c[k]) for k in io.ARGS + ("r_in", "g_ins", "g_attn", "m1", "m2", "m3")}
    fwd_args = [t[k] for k in io.ARGS]
    masks = dict(drop_node=t["m1"], drop_cat=t["m2"], drop_tok=t["m3"])
    for with_r in (True, False):
        r_in = t["r_in"] if with_r else None
        ins, attn, reserve = ops.instructions_train(*fwd_args, r_in=r_in, **masks)
        assert reserve.dtype == torch.uint8 and reserve.numel() == n * B * 2 * D * 4
        # without multipliers: the bits of the inference form (the same kernel, the reserve is a side output)
        plain = ops.instructions(*fwd_args, r_in=r_in)
        bare_ins, bare_attn, bare_res = ops.instructions_train(*fwd_args, r_in=r_in)
        assert torch.equal(bare_ins, plain[0]) and torch.equal(bare_attn, plain[1])
        if p == 0:
            assert torch.equal(ins, plain[0]) and torch.equal(attn, plain[1]) and torch.equal(reserve, bare_res)
        for with_ga in (True, False):
            want_ins, want_attn, want = _truth(shape, with_r, with_ga)
            tag = "%s r_in=%d g_attn=%d" % (shape, with_r, with_ga)
            err = max(float(np.abs(ins.cpu().numpy() - want_ins).max()), float(np.abs(attn.cpu().numpy() - want_attn).max()))
            print("%-34s forward max|diff| %.3e" % (tag, err))
            assert err <= TOL_FWD

            def run():
                return ops.instructions_backward(t["hidden"], t["node"], t["W_q"], t["W_cq"], t["w_ca"], ins, attn, reserve,
                                                 t["g_ins"], t["g_attn"] if with_ga else None, r_in=r_in, **masks)

            got = run()
            _check_grads(got, want, tag)
            _same(got, run())                                       # one fixed summation order
    # a question of padding only: uniform attention, and the gradient still passes the mask addition
    if B > 1:
        assert np.abs(attn[:, -1].cpu().numpy() - np.float32(1.0) / np.float32(T)).max() <= 1e-7
        if T > 1:
            assert float(np.abs(want["dhidden"][-1]).max()) > 0 and float(got["dhidden"][-1].abs().max()) > 0


def test_null_upstream_gradients_are_zeros_and_unwanted_outputs_are_none(dev):
    from gnnrag_amd import ops
    shape = (3, 5, 50, 3, 0.2)
    B, T, D, n, _ = shape
    c = _case(shape)
    t = {k: _to(dev, c[k]) for k in io.ARGS + ("r_in", "g_ins", "g_attn", "m1", "m2", "m3")}
    masks = dict(drop_node=t["m1"], drop_cat=t["m2"], drop_tok=t["m3"])
    ins, attn, reserve = ops.instructions_train(*[t[k] for k in io.ARGS], r_in=t["r_in"], **masks)

    def run(g_ins, g_attn, need=None):
        return ops.instructions_backward(t["hidden"], t["node"], t["W_q"], t["W_cq"], t["w_ca"], ins, attn, reserve, g_ins,
                                         g_attn, r_in=t["r_in"], need=need, **masks)

    full = run(t["g_ins"], t["g_attn"])
    _same(run(t["g_ins"], None), run(t["g_ins"], torch.zeros_like(t["g_attn"])))
    _same(run(None, t["g_attn"]), run(torch.zeros_like(t["g_ins"]), t["g_attn"]))
    need = {"dhidden": True, "dW_cq": True, "dW_q": [False, True, False], "db_q": [True, False, False]}
    part = run(t["g_ins"], t["g_attn"], need)
    for k in ("dnode", "dr_in", "db_cq", "dw_ca", "db_ca"):
        assert part[k] is None, k
    assert [x is None for x in part["dW_q"]] == [True, False, True] and [x is None for x in part["db_q"]] == [False, True, True]
    assert torch.equal(part["dhidden"], full["dhidden"]) and torch.equal(part["dW_cq"], full["dW_cq"])
    assert torch.equal(part["dW_q"][1], full["dW_q"][1]) and torch.equal(part["db_q"][0], full["db_q"][0])


def _fn_grads(dev, c, splits, with_r=True):
    """Gradients through autograd.InstructionsFn with the steps cut into ``splits`` (a list of (lo, hi)) chained calls."""
    from gnnrag_amd.autograd import InstructionsFn
    leaf = lambda a: _to(dev, a).requires_grad_(True)          # noqa: E731
    hidden, node, W_cq, b_cq, w_ca, b_ca = (leaf(c[k]) for k in ("hidden", "node", "W_cq", "b_cq", "w_ca", "b_ca"))
    W_q, b_q = [leaf(w) for w in c["W_q"]], [leaf(b) for b in c["b_q"]]
    r0 = leaf(c["r_in"]) if with_r else None
    mask = _to(dev, c["mask"])
    r, ins, attn = r0, [], []
    for lo, hi in splits:
        m = [None if c[k] is None else _to(dev, c[k][lo:hi]) for k in ("m1", "m2", "m3")]
        i, a = InstructionsFn.apply(hidden, node, mask, r, W_cq, b_cq, w_ca, b_ca, *m, *W_q[lo:hi], *b_q[lo:hi])
        r = i[-1]
        ins.append(i)
        attn.append(a)
    ins, attn = torch.cat(ins), torch.cat(attn)
    ((ins * _to(dev, c["g_ins"])).sum() + (attn * _to(dev, c["g_attn"])).sum()).backward()
    out = {"dhidden": hidden.grad, "dnode": node.grad, "dr_in": None if r0 is None else r0.grad, "dW_cq": W_cq.grad,
           "db_cq": b_cq.grad, "dw_ca": w_ca.grad.reshape(-1), "db_ca": b_ca.grad, "dW_q": [w.grad for w in W_q],
           "db_q": [b.grad for b in b_q]}
    assert tuple(w_ca.grad.shape) == tuple(w_ca.shape)
    return ins.detach(), attn.detach(), out


@pytest.mark.parametrize("shape", [(3, 5, 50, 3, 0.2), (2, 12, 200, 2, 0.0)], ids=str)
def test_a_chain_of_single_step_calls_gives_the_gradients_of_the_one_call(dev, shape):
    B, T, D, n, _ = shape
    c = _case(shape)
    _, _, want = _truth(shape, True, True)
    ins1, attn1, one = _fn_grads(dev, c, [(0, n)])
    insn, attnn, chain = _fn_grads(dev, c, [(s, s + 1) for s in range(n)])
    assert torch.equal(ins1, insn) and torch.equal(attn1, attnn)               # the forward: the same bits
    _check_grads(one, want, "one call")
    _check_grads(chain, want, "chain")
    for k in FLAT:
        _close(chain[k], one[k].cpu().numpy(), TOL_KERNEL, "chain vs one call " + k)
    assert float(one["db_ca"][0]) == 0.0 and float(chain["db_ca"][0]) == 0.0
    # without r_in nothing comes back for it, and the rest is the run from zeros
    _, _, no_r = _fn_grads(dev, c, [(0, n)], with_r=False)
    assert no_r["dr_in"] is None
    _check_grads(no_r, _truth(shape, False, True)[2], "no r_in")


def test_only_what_autograd_asks_for_is_computed(dev, monkeypatch):
    from gnnrag_amd import ops
    from gnnrag_amd.autograd import InstructionsFn
    shape = (3, 5, 50, 3, 0.0)
    c = _case(shape)
    seen = {}
    real = ops.instructions_backward

    def spy(*a, **k):
        seen.update(k["need"])
        return real(*a, **k)

    monkeypatch.setattr(ops, "instructions_backward", spy)
    t = {k: _to(dev, c[k]) for k in io.ARGS}
    t["W_cq"].requires_grad_(True)
    t["W_q"][1].requires_grad_(True)
    ins, attn = InstructionsFn.apply(t["hidden"], t["node"], t["mask"], None, t["W_cq"], t["b_cq"], t["w_ca"], t["b_ca"],
                                     None, None, None, *t["W_q"], *t["b_q"])
    ins[-1].sum().backward()                                      # attn unused: g_attn arrives as None
    assert seen == {"dhidden": False, "dnode": False, "dr_in": False, "dW_cq": True, "db_cq": False, "dw_ca": False,
                    "db_ca": False, "dW_q": [False, True, False], "db_q": [False, False, False]}
    assert t["W_cq"].grad is not None and t["W_q"][1].grad is not None and t["W_q"][0].grad is None


def test_unsupported_shapes_raise_the_bindings_error(dev):
    from gnnrag_amd import _lib, ops
    c = io.random_case(1, 2, 8, 9, seed=0)
    with pytest.raises(_lib.GnnragError, match=r"\(-2\)"):
        ops.instructions_train(*[_to(dev, c[k]) for k in io.ARGS])
    assert not ops.instructions_backward_supported(2, 8, 9)
    # the backward's own budget: the forward takes (T, D) = (8, 2048), the backward does not
    B, T, D, n = 1, 8, 2048, 1
    assert ops.instructions_supported(T, D, n) and not ops.instructions_backward_supported(T, D, n)
    z = lambda *s: torch.zeros(*s, device=dev)                   # noqa: E731
    with pytest.raises(_lib.GnnragError, match=r"\(-2\)"):
        ops.instructions_backward(z(B, T, D), z(B, D), [z(D, D)], z(D, 4 * D), z(D), z(n, B, D), z(n, B, T),
                                  torch.zeros(n * B * 2 * D * 4, dtype=torch.uint8, device=dev))


# -- the module layer ------------------------------------------------------------------------------------------------------

def _fp32_mask_semantics(mod):
    """The float64 truth of the module tests: the stand-in's steps with the mask addition as fp32 performs it - a padded
    logit is the constant VERY_NEG (in float64 ``ca - 1e11`` would keep ca's low bits and a question of padding only would
    get softmax(ca) instead of the uniform 1/T) - and the gradient passing the addition with derivative 1, as autograd's."""
    def get_instruction(relational_ins, step=0, query_node_emb=None):
        node = mod.query_node_emb if query_node_emb is None else query_node_emb
        r = relational_ins[:, None, :]
        q = getattr(mod, "question_linear%d" % step)(mod.linear_drop(node))
        cq = mod.cq_linear(mod.linear_drop(torch.cat([r, q, q - r, q * r], -1)))
        ca = mod.ca_linear(mod.linear_drop(cq * mod.query_hidden_emb))
        pad = mod.query_mask[:, :, None] == 0
        logit = ca + (torch.where(pad, torch.full_like(ca, io.VERY_NEG), ca) - ca).detach()
        a = torch.softmax(logit, 1)
        return (a * mod.query_hidden_emb).sum(1), a

    mod.get_instruction = get_instruction
    return mod


def _standin_pair(dev, monkeypatch, entity_dim=52, p=0.0, seed=11):
    """(float64 CPU stand-in, patched device stand-in whose own get_instruction raises, question tensor)."""
    from gnnrag_amd.modules.question_encoding.instruction import patch_instruction
    torch.manual_seed(seed)
    cpu = io.make_standin(20, entity_dim, 3, num_word=30, linear_dropout=p)
    gpu = copy.deepcopy(cpu).to(dev).train()

    def refuse(*a, **k):
        raise AssertionError("the steps went to the module's own torch ops")

    gpu.get_instruction = refuse
    assert patch_instruction(gpu) is gpu
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION", "1")
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION_TRAIN", "1")
    rng = np.random.default_rng(5)
    text = rng.integers(0, 30, (4, 6))
    text[1, 2:] = 30
    text[3, :] = 30                             # a question of padding only
    return _fp32_mask_semantics(cpu.double().train()), gpu, torch.from_numpy(text).long()


def _module_round(mod, q, weights):
    """The ReaRev sequence under autograd (forward, then init_reason and the steps one by one, rearev.py:192-196), every
    result weighted into one loss, one backward."""
    ins, attn = mod(q)
    outs = list(ins) + [a.reshape(a.shape[0], -1) for a in attn]
    mod.init_reason(q)
    for i in range(mod.num_ins):
        r, a = mod.get_instruction(mod.relational_ins, step=i)
        mod.instructions.append(r)
        mod.relational_ins = r
        outs += [r, a.reshape(a.shape[0], -1)]
    sum((o * w.to(device=o.device, dtype=o.dtype)).sum() for o, w in zip(outs, weights)).backward()
    return outs


def test_two_training_rounds_track_the_float64_module(dev, monkeypatch):
    """forward/backward, SGD step, forward/backward with the stand-in's own arithmetic made to raise: the test passes only
    when every step of both passes runs on the library.  One all-steps call per init_reason."""
    from gnnrag_amd import autograd
    cpu, gpu, q = _standin_pair(dev, monkeypatch)
    calls = []
    real = autograd.InstructionsFn.apply
    monkeypatch.setattr(autograd.InstructionsFn, "apply", lambda *a: (calls.append(len(a[11:]) // 2), real(*a))[1])
    B, T, D, n = 4, 6, 52, 3
    torch.manual_seed(3)
    weights = ([torch.randn(B, D) for _ in range(n)] + [torch.randn(B, T) for _ in range(n)] +
               [w for _ in range(n) for w in (torch.randn(B, D), torch.randn(B, T))])
    opts = [torch.optim.SGD(m.parameters(), lr=0.002) for m in (cpu, gpu)]
    first = None
    for rnd in range(2):
        for o in opts:
            o.zero_grad(set_to_none=True)
        want_outs = _module_round(cpu, q, weights)
        got_outs = _module_round(gpu, q.to(dev), weights)
        assert calls == [n, n] * (rnd + 1)                          # forward and the direct chain: one call each
        for k, (a, b) in enumerate(zip(got_outs, want_outs)):
            _close(a, b.detach().numpy(), TOL_MODULE, "round %d out %d" % (rnd, k), floor=1.0)
        for (name, pg), pc in zip(gpu.named_parameters(), cpu.parameters()):
            assert (pg.grad is None) == (pc.grad is None), name
            if pc.grad is not None:
                _close(pg.grad, pc.grad.numpy(), TOL_MODULE, "round %d %s" % (rnd, name))
        if rnd == 0:
            assert float(gpu.ca_linear.bias.grad[0]) == 0.0
            first = [None if pc.grad is None else pc.grad.clone() for pc in cpu.parameters()]
            for o in opts:
                o.step()
    # the step matters at this tolerance: the truth's own gradients moved by more than the bound
    moved = [float((f - pc.grad).abs().max() / pc.grad.abs().max()) for f, pc in zip(first, cpu.parameters())
             if f is not None and float(pc.grad.abs().max()) > 0]
    assert max(moved) > 10 * TOL_MODULE


def test_fixed_masks_give_the_oracle_with_those_masks(dev, monkeypatch):
    """linear_drop.p = 0.2 in training mode, the mask helper replaced by fixed multipliers: the module's results and the
    gradients of the steps' parameters are the oracle's on the device's own token states (equal inputs: the kernel rule)."""
    from gnnrag_amd.modules.question_encoding import instruction as mi
    _, gpu, q = _standin_pair(dev, monkeypatch, p=0.2, seed=12)
    B, T, D, n = 4, 6, 52, 3
    rng = np.random.default_rng(8)
    scale = np.float32(1.0) / np.float32(0.8)
    fixed = [(rng.random(s) >= 0.2).astype(np.float32) * scale for s in ((n, B, D), (n, B, 4 * D), (n, B, T, D))]
    asked = []

    def fixed_masks(p, n_, B_, T_, D_, device):
        asked.append((p, n_, B_, T_, D_))
        return tuple(torch.from_numpy(m).to(device) for m in fixed)

    monkeypatch.setattr(mi, "draw_masks", fixed_masks)
    ins, attn = gpu(q.to(dev))
    assert asked == [(0.2, n, B, T, D)]
    g_ins = torch.from_numpy(rng.standard_normal((n, B, D)).astype(np.float32))
    (torch.stack(list(ins)) * g_ins.to(dev)).sum().backward()
    c = lambda t: t.detach().cpu().numpy()      # noqa: E731
    lins = [getattr(gpu, "question_linear%d" % s) for s in range(n)]
    want_ins, want_attn, saved = igo.forward(c(gpu.query_hidden_emb), c(gpu.query_node_emb).reshape(B, D), c(gpu.query_mask),
                                             [c(m.weight) for m in lins], [c(m.bias) for m in lins], c(gpu.cq_linear.weight),
                                             c(gpu.cq_linear.bias), c(gpu.ca_linear.weight), c(gpu.ca_linear.bias),
                                             m1=fixed[0], m2=fixed[1], m3=fixed[2])
    assert float(np.abs(c(torch.stack(list(ins))) - want_ins).max()) <= TOL_FWD
    assert float(np.abs(c(torch.stack(list(attn)))[..., 0] - want_attn).max()) <= TOL_FWD
    want = igo.backward(saved, g_ins.numpy())
    _close(gpu.cq_linear.weight.grad, want["dW_cq"], TOL_KERNEL, "fixed masks dW_cq")
    _close(gpu.cq_linear.bias.grad, want["db_cq"], TOL_KERNEL, "fixed masks db_cq")
    _close(gpu.ca_linear.weight.grad.reshape(-1), want["dw_ca"], TOL_KERNEL, "fixed masks dw_ca")
    for s, m in enumerate(lins):
        _close(m.weight.grad, want["dW_q"][s], TOL_KERNEL, "fixed masks dW_q[%d]" % s)
        _close(m.bias.grad, want["db_q"][s], TOL_KERNEL, "fixed masks db_q[%d]" % s)
    assert float(gpu.ca_linear.bias.grad[0]) == 0.0


def test_a_shape_the_backward_does_not_take_runs_the_original_methods(dev, monkeypatch):
    from gnnrag_amd import autograd, ops
    from gnnrag_amd.modules.question_encoding.instruction import patch_instruction
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION", "1")
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION_TRAIN", "1")

    def no_library(*a, **k):
        raise AssertionError("an unsupported shape reached the library")

    monkeypatch.setattr(autograd.InstructionsFn, "apply", no_library)
    torch.manual_seed(2)
    mod = io.make_standin(8, 2048, 1, num_word=30, device=dev).train()
    patch_instruction(mod)
    q = torch.randint(0, 30, (2, 8), device=dev)
    assert ops.instructions_supported(8, 2048, 1) and not ops.instructions_backward_supported(8, 2048, 1)
    ins, _ = mod(q)
    ins[-1].sum().backward()
    assert float(mod.cq_linear.weight.grad.abs().sum()) > 0
    # the switch off: the same, whatever the shape
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION_TRAIN", "0")
    small = patch_instruction(io.make_standin(8, 16, 2, num_word=30, device=dev).train())
    ins, _ = small(q)
    ins[-1].sum().backward()
    assert float(small.cq_linear.weight.grad.abs().sum()) > 0
