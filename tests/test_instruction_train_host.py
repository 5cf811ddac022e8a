"""The training form of instruction generation, host side: the float64 oracle of the GPU tests
(tests/instruction_grad_oracle.py) reproduces the gradients torch's autograd derives on the live reference's module
(tests/golden/instruction_grad_ref.npz); the entry points are declared in gnnrag.h and in the binding (additive to ABI 16) and
refuse bad arguments before they touch a device; ``GNNRAG_HIP_INSTRUCTION_TRAIN`` is read at every call, defaults to off, and
unset leaves a patched module under autograd the module's own methods bit for bit; the mask helper draws 0 or 1/(1-p).

Bound of the oracle check: every gradient within 2e-6 of the tensor's largest entry.  The fixture is fp32 as shipped; torch's
fp32 autograd stays within 6.1e-7 of that scale against float64 on these shapes.  db_ca, exactly zero in the oracle, is held
to the same figure as an absolute bound (torch leaves rounding residue there)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import instruction_grad_oracle as igo
import instruction_oracle as io

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "instruction_grad_ref.npz")
TOL_FIXTURE = 2e-6


def _fixture():
    g = np.load(GOLDEN)
    n = g["ins"].shape[0]
    args = dict(hidden=g["hidden"], node=g["node"], mask=g["mask"], W_q=[g["W_q%d" % s] for s in range(n)],
                b_q=[g["b_q%d" % s] for s in range(n)], W_cq=g["W_cq"], b_cq=g["b_cq"], w_ca=g["w_ca"], b_ca=g["b_ca"])
    return g, n, args


def test_fixture_is_what_the_issue_states():
    g, n, _ = _fixture()
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert g["hidden"].shape == (3, 5, 20) and n == 3 and g["hidden"].dtype == np.float32
    assert g["mask"][0].all() and not g["mask"][-1].any()                   # one question of padding only
    assert np.abs(g["attn"][:, -1] - 0.2).max() <= 1e-7 and np.abs(g["dhidden"][-1]).max() > 0


def test_oracle_reproduces_the_reference_modules_autograd():
    g, n, args = _fixture()
    ins, attn, saved = igo.forward(*[args[k] for k in io.ARGS], r_in=g["r_in"])
    assert np.abs(ins - g["ins"]).max() <= 1e-6 and np.abs(attn - g["attn"]).max() <= 1e-6
    got = igo.backward(saved, g["g_ins"], g["g_attn"])
    want = {"dhidden": g["dhidden"], "dnode": g["dnode"], "dr_in": g["dr_in"], "dW_cq": g["dW_cq"], "db_cq": g["db_cq"],
            "dw_ca": g["dw_ca"].reshape(-1)}
    have = {k: got[k] for k in want}
    for s in range(n):
        want["dW_q%d" % s], want["db_q%d" % s] = g["dW_q%d" % s], g["db_q%d" % s]
        have["dW_q%d" % s], have["db_q%d" % s] = got["dW_q"][s], got["db_q"][s]
    for k, w in want.items():
        scale = float(np.abs(w).max())
        err = float(np.abs(have[k] - w).max())
        print("%-8s max|diff| %.3e  scale %.3e  ratio %.3e" % (k, err, scale, err / scale))
        assert scale > 0 and err <= TOL_FIXTURE * scale, k
    assert got["db_ca"].shape == (1,) and got["db_ca"][0] == 0.0
    assert abs(float(g["db_ca"][0])) <= TOL_FIXTURE


def test_oracle_without_masks_is_the_inference_oracle_and_ones_are_no_masks():
    c = io.random_case(3, 5, 8, 2, seed=1)
    want_ins, want_attn = io.instructions(*[c[k] for k in io.ARGS])
    ins, attn, saved = igo.forward(*[c[k] for k in io.ARGS])
    assert np.array_equal(ins, want_ins) and np.array_equal(attn, want_attn)
    ones = dict(m1=np.ones((2, 3, 8)), m2=np.ones((2, 3, 32)), m3=np.ones((2, 3, 5, 8)))
    ins1, _, saved1 = igo.forward(*[c[k] for k in io.ARGS], **ones)
    assert np.array_equal(ins1, ins)
    rng = np.random.default_rng(0)
    g_ins = rng.standard_normal(ins.shape)
    a, b = igo.backward(saved, g_ins), igo.backward(saved1, g_ins)
    for k in ("dhidden", "dnode", "dr_in", "dW_cq", "db_cq", "dw_ca"):
        assert np.array_equal(a[k], b[k]), k


def test_oracle_with_masks_against_float64_autograd():
    """The explicit-mask backward against torch's float64 autograd of the same arithmetic (the stand-in's statement of the
    steps with the multipliers written out)."""
    B, T, D, n = 3, 4, 6, 2
    c = io.random_case(B, T, D, n, seed=2)
    rng = np.random.default_rng(3)
    keep = lambda *shape: (rng.random(shape) < 0.7) / 0.7       # noqa: E731
    m1, m2, m3 = keep(n, B, D), keep(n, B, 4 * D), keep(n, B, T, D)
    r_in, g_ins, g_attn = rng.standard_normal((B, D)), rng.standard_normal((n, B, D)), rng.standard_normal((n, B, T))
    _, _, saved = igo.forward(*[c[k] for k in io.ARGS], r_in=r_in, m1=m1, m2=m2, m3=m3)
    got = igo.backward(saved, g_ins, g_attn)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)     # noqa: E731
    hidden, node, r0, W_cq, b_cq, w_ca, b_ca = (t(x) for x in (c["hidden"], c["node"], r_in, c["W_cq"], c["b_cq"],
                                                               c["w_ca"].reshape(-1), c["b_ca"]))
    W_q, b_q = [t(w) for w in c["W_q"]], [t(b) for b in c["b_q"]]
    mask = torch.tensor(c["mask"], dtype=torch.float64)
    r, loss = r0, 0.0
    for s in range(n):
        q = (node * torch.tensor(m1[s])) @ W_q[s].T + b_q[s]
        z = torch.cat([r, q, q - r, q * r], -1) * torch.tensor(m2[s])
        cq = z @ W_cq.T + b_cq
        ca = ((cq[:, None, :] * hidden * torch.tensor(m3[s])) * w_ca).sum(-1) + b_ca
        # the fp32 sum of the reference is the constant for a padded token; the addition passes the gradient
        logit = ca + (torch.where(mask != 0, ca, torch.full_like(ca, io.VERY_NEG)) - ca).detach()
        a = torch.softmax(logit, 1)
        r = (a[:, :, None] * hidden).sum(1)
        loss = loss + (r * torch.tensor(g_ins[s])).sum() + (a * torch.tensor(g_attn[s])).sum()
    loss.backward()
    want = {"dhidden": hidden.grad, "dnode": node.grad, "dr_in": r0.grad, "dW_cq": W_cq.grad, "db_cq": b_cq.grad,
            "dw_ca": w_ca.grad}
    for k, w in want.items():
        assert np.abs(got[k] - w.numpy()).max() <= 1e-12 * max(1.0, float(w.abs().max())), k
    for s in range(n):
        assert np.abs(got["dW_q"][s] - W_q[s].grad.numpy()).max() <= 1e-12
        assert np.abs(got["db_q"][s] - b_q[s].grad.numpy()).max() <= 1e-12
    assert abs(float(b_ca.grad[0])) <= 1e-12 and got["db_ca"][0] == 0.0


# -- the entry points ------------------------------------------------------------------------------------------------------

SYMBOLS = {"gnnrag_instructions_reserve_bytes": 4, "gnnrag_instructions_train": 22,
           "gnnrag_instructions_backward_workspace_bytes": 4, "gnnrag_instructions_backward": 31}


def test_header_binding_and_python_layers_declare_the_training_form():
    from gnnrag_amd import _lib, autograd, ops
    from gnnrag_amd.modules.question_encoding import instruction as mi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gnnrag.h")).read(), flags=re.S)
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "gnnrag.h does not declare " + name
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    assert re.search(r"#define\s+GNNRAG_ABI_VERSION\s+16\b", src) and _lib.ABI_VERSION == 16
    assert len(_lib.SIGNATURES["gnnrag_instructions"][1]) == 17                  # the inference entry keeps its shape
    for fn in (ops.instructions_train, ops.instructions_backward, ops.instructions_backward_supported,
               autograd.InstructionsFn.apply, mi.draw_masks, mi.train_enabled):
        assert callable(fn)
    assert "instruction_bwd.hip" in __import__("gnnrag_amd.build", fromlist=["SOURCES"]).SOURCES


def test_binding_states_the_backwards_limits():
    from gnnrag_amd import ops
    ok = ops.instructions_backward_supported
    for T in (1, 5, 12, 63, 64):
        for D in (1, 50, 200, 255, 256):
            assert ok(T, D, 8) and ok(T, D, 1), (T, D)
    assert ok(70, 64, 8) and ok(12, 200, 2)
    assert not ok(12, 200, 9) and not ok(0, 4, 1) and not ok(4, 0, 1) and not ok(4, 4, 0)
    assert not ok(41, 1000, 1) and not ok(8, 4096, 1)              # the forward refuses them too
    assert ops.instructions_supported(8, 2048, 2) and not ok(8, 2048, 2)         # 12 D of vectors on top of the states


@pytest.fixture(scope="module")
def lib():
    from gnnrag_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.gnnrag_abi_version() == 16
    return lib


def test_sizes_follow_the_header(lib):
    assert lib.gnnrag_instructions_reserve_bytes(3, 5, 50, 3) == 3 * 3 * 2 * 50 * 4
    assert lib.gnnrag_instructions_reserve_bytes(3, 5, 50, 9) == 0 and lib.gnnrag_instructions_reserve_bytes(0, 5, 50, 1) == 0
    assert lib.gnnrag_instructions_backward_workspace_bytes(2, 5, 50, 3) > 0
    assert lib.gnnrag_instructions_backward_workspace_bytes(2, 8, 2048, 2) == 0
    assert lib.gnnrag_instructions_backward_workspace_bytes(2, 5, 50, 9) == 0


def _train(lib, B=2, T=3, D=4, n=2, reserve=4096, reserve_bytes=1 << 20, **null):
    p = 4096
    v = dict(hidden=p, node=p, mask=p, W_cq=p, b_cq=p, w_ca=p, b_ca=p, ins_out=p, attn_out=p)
    v.update(null)
    Wq, bq = (C.c_void_p * 9)(*[p] * 9), (C.c_void_p * 9)(*[p] * 9)
    return lib.gnnrag_instructions_train(v["hidden"], v["node"], v["mask"], None, Wq, bq, v["W_cq"], v["b_cq"], v["w_ca"],
                                         v["b_ca"], None, None, None, B, T, D, n, v["ins_out"], v["attn_out"], reserve,
                                         reserve_bytes, None)


def _backward(lib, B=2, T=3, D=4, n=2, reserve=4096, reserve_bytes=1 << 20, ws=4096, ws_bytes=0, Wq_null=False, **null):
    p = 4096
    v = dict(hidden=p, node=p, W_cq=p, w_ca=p, ins=p, attn=p)
    v.update(null)
    Wq = (C.c_void_p * 9)(*[p] * 9)
    if Wq_null:
        Wq[1] = None
    return lib.gnnrag_instructions_backward(v["hidden"], v["node"], None, Wq, v["W_cq"], v["w_ca"], None, None, None,
                                            v["ins"], v["attn"], reserve, reserve_bytes, None, None, p, p, p, None, None, p,
                                            p, p, p, B, T, D, n, ws, ws_bytes, None)


def test_bad_arguments_are_refused_before_anything_is_launched(lib):
    """Every pointer is a dummy non-NULL address and there is no device here: each answer comes from the argument checks."""
    for k in ("hidden", "node", "mask", "W_cq", "b_cq", "w_ca", "b_ca", "ins_out", "attn_out"):
        assert _train(lib, **{k: None}) == -1, k
    assert _train(lib, n=9) == -2 and _train(lib, T=41, D=1000, n=1) == -2 and _train(lib, B=0) == -1
    need = lib.gnnrag_instructions_reserve_bytes(2, 3, 4, 2)
    assert _train(lib, reserve=None) == -3 and _train(lib, reserve_bytes=need - 1) == -3
    for k in ("hidden", "node", "W_cq", "w_ca", "ins", "attn"):
        assert _backward(lib, **{k: None}) == -1, k
    assert _backward(lib, Wq_null=True) == -1 and _backward(lib, T=0) == -1
    assert _backward(lib, n=9) == -2 and _backward(lib, T=8, D=2048) == -2
    assert _backward(lib, T=70000, D=70000, n=1) == -2                        # no 32-bit overflow in the check
    assert _backward(lib, reserve=None) == -3 and _backward(lib, reserve_bytes=need - 1) == -3
    assert _backward(lib, ws=None) == -3


def test_the_wrappers_refuse_cpu_tensors():
    from gnnrag_amd import _lib, ops
    c = io.random_case(2, 3, 4, 1, seed=0)
    t = lambda a: [torch.from_numpy(x) for x in a] if isinstance(a, list) else torch.from_numpy(a)   # noqa: E731
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.instructions_train(*[t(c[k]) for k in io.ARGS])
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.instructions_backward(t(c["hidden"]), t(c["node"]), t(c["W_q"]), t(c["W_cq"]), t(c["w_ca"]),
                                  torch.zeros(1, 2, 4), torch.zeros(1, 2, 3), torch.zeros(64, dtype=torch.uint8))


# -- the module layer ------------------------------------------------------------------------------------------------------

def test_the_switch_is_read_at_every_call_and_defaults_to_off(monkeypatch):
    from gnnrag_amd.modules.question_encoding import instruction as mi
    monkeypatch.delenv("GNNRAG_HIP_INSTRUCTION_TRAIN", raising=False)
    assert mi.TRAIN_DEFAULT == "0" and not mi.train_enabled()
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION_TRAIN", "1")
    assert mi.train_enabled()
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION_TRAIN", "0")
    assert not mi.train_enabled()


def _train_round(mod, q):
    """forward, the direct chain of rearev.py:192-196, one backward; returns everything the round produced."""
    mod.zero_grad(set_to_none=True)
    ins, attn = mod(q)
    outs = list(ins) + list(attn)
    mod.init_reason(q)
    for i in range(mod.num_ins):
        r, a = mod.get_instruction(mod.relational_ins, step=i)
        mod.instructions.append(r)
        mod.relational_ins = r
        outs += [r, a]
    sum((o * (k + 1)).sum() for k, o in enumerate(outs)).backward()
    return [o.detach().clone() for o in outs] + [p.grad.clone() for p in mod.parameters() if p.grad is not None]


@pytest.mark.parametrize("train_switch", [None, "0", "1"])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_patched_module_under_autograd_is_the_original_bit_for_bit(monkeypatch, train_switch, p):
    """CPU tensors, the inference switch on: with the training switch unset, off - and on, where CPU tensors are not
    eligible - a training round is the module's own methods and its own dropout draws, bit for bit."""
    from gnnrag_amd import autograd
    from gnnrag_amd.modules.question_encoding import instruction as mi
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION", "1")
    if train_switch is None:
        monkeypatch.delenv("GNNRAG_HIP_INSTRUCTION_TRAIN", raising=False)
    else:
        monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION_TRAIN", train_switch)

    def no_library(*a, **k):
        raise AssertionError("the library was called on CPU tensors")
    monkeypatch.setattr(autograd.InstructionsFn, "apply", no_library)
    monkeypatch.setattr(mi, "draw_masks", no_library)
    torch.manual_seed(0)
    plain = io.make_standin(6, 8, 3, num_word=20, linear_dropout=p).train()
    patched = io.make_standin(6, 8, 3, num_word=20, linear_dropout=p).train()
    patched.load_state_dict(plain.state_dict())
    assert mi.patch_instruction(patched) is patched
    q = torch.tensor([[1, 2, 3, 20, 20], [4, 5, 6, 7, 8], [20, 20, 20, 20, 20]])
    for rnd in range(2):
        torch.manual_seed(100 + rnd)
        want = _train_round(plain, q)
        torch.manual_seed(100 + rnd)
        got = _train_round(patched, q)
        assert len(want) == len(got)
        for a, b in zip(want, got):
            assert torch.equal(a, b)


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_mask_helper_draws_zero_or_the_inverse_keep_rate(p):
    from gnnrag_amd.modules.question_encoding.instruction import draw_masks
    torch.manual_seed(4)
    n, B, T, D = 2, 16, 12, 200
    masks = draw_masks(p, n, B, T, D, torch.device("cpu"))
    assert [tuple(m.shape) for m in masks] == [(n, B, D), (n, B, 4 * D), (n, B, T, D)]
    scale = np.float32(1.0) / np.float32(1.0 - p)
    for m in masks:
        assert m.dtype == torch.float32
        a = m.numpy()
        assert np.isin(a, [np.float32(0.0), scale]).all()
        kept, N = float((a != 0).mean()), a.size
        assert abs(kept - (1.0 - p)) <= 5.0 * np.sqrt(p * (1.0 - p) / N), (kept, N)
