"""The training form of the instruction update, host side: the float64 oracle of the GPU tests
(tests/query_reform_grad_oracle.py) reproduces the gradients torch's autograd derives on the live reference's ``QueryReform``
(tests/golden/query_reform_grad_ref.npz) and equals torch's float64 autograd on a random case; the entry points are declared
in gnnrag.h and in the binding (additive to ABI 16) and refuse bad arguments before they touch a device;
``GNNRAG_HIP_QUERY_REFORM_TRAIN`` is read at every call, defaults to off, and - unset or set - leaves a bound group of modules
on CPU tensors under autograd the reference's ``bmm`` + ``Fusion`` bit for bit.

Bound of the fixture check: every tensor within 2e-6 of its largest entry (the bound of test_instruction_train_host.py).  The
fixture is fp32 as shipped; torch's fp32 autograd stays within 4.3e-7 of that scale against float64 on these shapes."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import query_reform_grad_oracle as qo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "query_reform_grad_ref.npz")
TOL_FIXTURE = 2e-6


def test_fixture_is_what_the_issue_states():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 256 * 1024
    B, N, D, n = 3, 7, 20, 3
    assert g["ent"].shape == (B, N, D) and g["seed"].shape == (B, N) and g["ent"].dtype == np.float32
    per_question = sorted((g["seed"] != 0).sum(1).tolist())
    assert per_question == [0, 1, 2]                            # one question without a seed, one with two
    two = int(np.argmax((g["seed"] != 0).sum(1)))
    assert g["seed"][two, N - 1] != 0                          # one of the two in the last slot
    for j in range(n):
        for k, shape in (("q", (B, D)), ("G", (B, D)), ("out", (B, D)), ("dq", (B, D)), ("W_r", (D, 3 * D)),
                         ("W_g", (D, 3 * D)), ("dW_r", (D, 3 * D)), ("dW_g", (D, 3 * D))):
            assert g["%s%d" % (k, j)].shape == shape and g["%s%d" % (k, j)].dtype == np.float32
    assert "q%d" % n not in g.files and g["d_ent"].shape == (B, N, D)
    assert not g["d_ent"][g["seed"] == 0].any() and g["d_ent"][g["seed"] != 0].any()


def test_oracle_reproduces_the_reference_modules_autograd():
    g = np.load(GOLDEN)
    n = 3
    out, saved = qo.forward([g["q%d" % j] for j in range(n)], g["seed"], g["ent"], [g["W_r%d" % j] for j in range(n)],
                            [g["W_g%d" % j] for j in range(n)])
    got = qo.backward(saved, [g["G%d" % j] for j in range(n)])
    want, have = {"d_ent": g["d_ent"]}, {"d_ent": got["d_ent"]}
    for j in range(n):
        for k in ("dq", "dW_r", "dW_g"):
            want["%s%d" % (k, j)], have["%s%d" % (k, j)] = g["%s%d" % (k, j)], got[k][j]
        want["out%d" % j], have["out%d" % j] = g["out%d" % j], out[j]
    for k, w in want.items():
        scale = float(np.abs(w).max())
        err = float(np.abs(have[k] - w).max())
        print("%-8s max|diff| %.3e  scale %.3e  ratio %.3e" % (k, err, scale, err / scale))
        assert scale > 0 and err <= TOL_FIXTURE * scale, k


def _plain(q, ent, seed, W_r, W_g):
    """query_update.py:40,44 with Fusion :6-16, written out."""
    y = torch.bmm(seed.unsqueeze(1), ent).squeeze(1)
    feats = torch.cat([q, y, q - y], dim=-1)
    gate = torch.sigmoid(feats @ W_g.t())
    return gate * (feats @ W_r.t()) + (1 - gate) * q


def test_oracle_against_float64_autograd_with_an_unused_reform():
    B, N, D, n = 4, 9, 6, 3
    c = qo.train_case(B, N, D, n, seed=5)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)     # noqa: E731
    qs, W_rs, W_gs, ent = [t(q) for q in c["qs"]], [t(w) for w in c["W_rs"]], [t(w) for w in c["W_gs"]], t(c["ent"])
    seed = torch.tensor(c["seed"], dtype=torch.float64)
    G = [c["G"][0], None, c["G"][2]]
    outs = [_plain(qs[j], ent, seed, W_rs[j], W_gs[j]) for j in range(n)]
    sum((outs[j] * torch.tensor(G[j], dtype=torch.float64)).sum() for j in range(n) if G[j] is not None).backward()
    out, saved = qo.forward(c["qs"], c["seed"], c["ent"], c["W_rs"], c["W_gs"])
    got = qo.backward(saved, G)
    for j in range(n):
        assert np.abs(out[j] - outs[j].detach().numpy()).max() <= 1e-13
        if G[j] is None:
            assert qs[j].grad is None and got["dq"][j] is None and got["dW_r"][j] is None and got["dW_g"][j] is None
            continue
        for k, w in (("dq", qs[j].grad), ("dW_r", W_rs[j].grad), ("dW_g", W_gs[j].grad)):
            assert np.abs(got[k][j] - w.numpy()).max() <= 1e-12 * max(1.0, float(w.abs().max())), (k, j)
    assert np.abs(got["d_ent"] - ent.grad.numpy()).max() <= 1e-12
    assert (c["seed"][-1] == 0).all() and (c["seed"][0] != 0).sum() == 2 and c["seed"][0, N - 1] == 1.0
    assert 0.5 in c["seed"][0]


# -- the entry points ------------------------------------------------------------------------------------------------------

SYMBOLS = {"gnnrag_query_reform_reserve_bytes": 3, "gnnrag_query_reform_train": 14,
           "gnnrag_query_reform_backward_workspace_bytes": 4, "gnnrag_query_reform_backward": 18}


def test_header_binding_and_python_layers_declare_the_training_form():
    from gnnrag_amd import _lib, autograd, install, ops
    from gnnrag_amd.modules import query_update as mq
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gnnrag.h")).read(), flags=re.S)
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "gnnrag.h does not declare " + name
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    assert re.search(r"#define\s+GNNRAG_ABI_VERSION\s+16\b", src) and _lib.ABI_VERSION == 16
    assert re.search(r"#define\s+GNNRAG_MAX_REFORMS\s+8\b", src) and ops.MAX_REFORMS == 8
    assert re.search(r"#define\s+GNNRAG_QUERY_REFORM_MAX_D\s+4096\b", src) and ops.QUERY_REFORM_MAX_D == 4096
    assert len(_lib.SIGNATURES["gnnrag_query_reform"][1]) == 11                 # the inference entry keeps its shape
    for fn in (ops.query_reform_train, ops.query_reform_backward, ops.query_reform_backward_supported,
               autograd.QueryReformFn.apply, mq.bind_reforms, mq.train_enabled):
        assert callable(fn)
    assert "query_update_bwd.hip" in __import__("gnnrag_amd.build", fromlist=["SOURCES"]).SOURCES
    ok = ops.query_reform_backward_supported
    assert ok(1, 1) and ok(200, 2) and ok(4096, 8) and not ok(4097, 1) and not ok(200, 9) and not ok(0, 1) and not ok(4, 0)


@pytest.fixture(scope="module")
def lib():
    from gnnrag_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.gnnrag_abi_version() == 16
    return lib


def test_sizes_follow_the_header(lib):
    assert lib.gnnrag_query_reform_reserve_bytes(3, 50, 3) == (3 * 50 + 3 * 3 * 2 * 50) * 4
    for B, D, n in ((0, 50, 1), (3, 0, 1), (3, 50, 0), (3, 50, 9), (3, 4097, 1)):
        assert lib.gnnrag_query_reform_reserve_bytes(B, D, n) == 0
        assert lib.gnnrag_query_reform_backward_workspace_bytes(B, 7, D, n) == 0
    assert lib.gnnrag_query_reform_backward_workspace_bytes(3, 7, 50, 3) >= 3 * 3 * 6 * 50 * 4
    assert lib.gnnrag_query_reform_backward_workspace_bytes(3, 0, 50, 3) == 0


def _arr(n=9, null=None):
    a = (C.c_void_p * n)(*[4096] * n)
    if null is not None:
        a[null] = None
    return a


def _train(lib, B=2, N=5, D=4, n=2, ld=None, q=None, Wr=None, Wg=None, reserve=4096, reserve_bytes=1 << 20, **null):
    v = dict(seed=4096, ent=4096, out=4096)
    v.update(null)
    return lib.gnnrag_query_reform_train(q or _arr(), v["seed"], v["ent"], D if ld is None else ld, Wr or _arr(),
                                         Wg or _arr(), v["out"], reserve, reserve_bytes, B, N, D, n, None)


def _backward(lib, B=2, N=5, D=4, n=2, q=None, Wr=None, Wg=None, g_out=None, seed=4096, reserve=4096,
              reserve_bytes=1 << 20, ws=4096, ws_bytes=0):
    return lib.gnnrag_query_reform_backward(q or _arr(), seed, Wr or _arr(), Wg or _arr(), reserve, reserve_bytes,
                                            g_out or _arr(), _arr(), _arr(), _arr(), 4096, B, N, D, n, ws, ws_bytes, None)


def test_bad_arguments_are_refused_before_anything_is_launched(lib):
    """Every pointer is a dummy non-NULL address and there is no device here: each answer comes from the argument checks."""
    for k in ("seed", "ent", "out"):
        assert _train(lib, **{k: None}) == -1, k
    assert _train(lib, n=0) == -1 and _train(lib, n=9) == -2
    assert _train(lib, ld=3) == -1 and _train(lib, D=4097) == -2
    assert _train(lib, B=0) == -1 and _train(lib, N=0) == -1
    for k in ("q", "Wr", "Wg"):
        assert _train(lib, **{k: _arr(null=1)}) == -1, k
        assert _backward(lib, **{k: _arr(null=1)}) == -1, k
    assert _train(lib, q=_arr(null=2), reserve_bytes=0) == -3  # past n = 2: not read; the next check answers
    need = lib.gnnrag_query_reform_reserve_bytes(2, 4, 2)
    assert _train(lib, reserve=None) == -3 and _train(lib, reserve_bytes=need - 1) == -3
    assert _backward(lib, n=0) == -1 and _backward(lib, n=9) == -2 and _backward(lib, D=4097) == -2
    assert _backward(lib, seed=None) == -1 and _backward(lib, B=0) == -1
    assert _backward(lib, reserve=None) == -3 and _backward(lib, reserve_bytes=need - 1) == -3
    assert _backward(lib, ws=None) == -3 and _backward(lib, ws_bytes=16) == -3


def test_the_wrappers_refuse_cpu_tensors():
    from gnnrag_amd import _lib, ops
    c = qo.train_case(2, 3, 4, 1, seed=0)
    t = lambda a: [torch.from_numpy(x) for x in a] if isinstance(a, list) else torch.from_numpy(a)   # noqa: E731
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.query_reform_train(t(c["qs"]), t(c["seed"]), t(c["ent"]), t(c["W_rs"]), t(c["W_gs"]))
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.query_reform_backward(t(c["qs"]), t(c["seed"]), t(c["W_rs"]), t(c["W_gs"]), torch.zeros(64, dtype=torch.uint8),
                                  [torch.zeros(2, 4)])


# -- the module layer ------------------------------------------------------------------------------------------------------

def test_the_switch_is_read_at_every_call_and_defaults_to_off(monkeypatch):
    from gnnrag_amd.modules import query_update as mq
    monkeypatch.delenv("GNNRAG_HIP_QUERY_REFORM_TRAIN", raising=False)
    assert mq.TRAIN_DEFAULT == "0" and not mq.train_enabled()
    monkeypatch.setenv("GNNRAG_HIP_QUERY_REFORM_TRAIN", "1")
    assert mq.train_enabled()
    monkeypatch.setenv("GNNRAG_HIP_QUERY_REFORM_TRAIN", "0")
    assert not mq.train_enabled()


def _cpu_round(model, c, plain):
    ins0 = [torch.from_numpy(q).clone().requires_grad_(True) for q in c["qs"]]
    ents = [torch.from_numpy(c["ent"]).clone().requires_grad_(True), torch.from_numpy(c["ent"] * 0.5).requires_grad_(True)]
    seed, mask = torch.from_numpy(c["seed"]), torch.ones(c["seed"].shape)
    model.zero_grad(set_to_none=True)
    if plain:
        outs = list(ins0)
        for ent in ents:
            outs = [_plain(outs[j], ent, seed, getattr(model, "reform%d" % j).fusion.r.weight,
                           getattr(model, "reform%d" % j).fusion.g.weight) for j in range(len(outs))]
    else:
        outs = model.loop(ins0, ents, seed, mask)
    sum((o * (k + 1)).sum() for k, o in enumerate(outs)).backward()
    grads = [t.grad for t in ins0 + ents] + [p.grad for p in model.parameters()]
    return [o.detach().clone() for o in outs], grads


@pytest.mark.parametrize("switch", [None, "0", "1"])
def test_bound_modules_on_cpu_tensors_are_the_torch_form_bit_for_bit(monkeypatch, switch):
    from gnnrag_amd import ops
    from gnnrag_amd.modules import query_update as mq
    if switch is None:
        monkeypatch.delenv("GNNRAG_HIP_QUERY_REFORM_TRAIN", raising=False)
    else:
        monkeypatch.setenv("GNNRAG_HIP_QUERY_REFORM_TRAIN", switch)

    def no_library(*a, **k):
        raise AssertionError("the library was called on CPU tensors")
    monkeypatch.setattr(ops, "query_reform_train", no_library)
    torch.manual_seed(3)
    B, N, D, n = 3, 7, 8, 3
    model = qo.standin(D, n)
    assert mq.bind_reforms(model) is model
    assert [getattr(model, "reform%d" % j)._qr_index for j in range(n)] == [0, 1, 2]
    assert model.reform0._qr_bound is model.reform2._qr_bound and model.reform0._qr_bound.instruction is model.instruction
    assert not any(k.startswith("reform0.") and "reform1" in k for k in model.state_dict())   # no sibling became a submodule
    assert len(list(model.reform0.modules())) == 5              # itself, fusion, its two linears and q_ent_attn
    c = qo.train_case(B, N, D, n, seed=6)
    want_out, want_grad = _cpu_round(model, c, plain=True)
    got_out, got_grad = _cpu_round(model, c, plain=False)
    for a, b in zip(want_out, got_out):
        assert torch.equal(a, b)
    assert len(want_grad) == len(got_grad)
    for a, b in zip(want_grad, got_grad):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    for j in range(n):
        assert getattr(model, "reform%d" % j).q_ent_attn.weight.grad is None


def test_a_deep_copy_binds_to_itself_and_an_unbound_module_has_no_state():
    from gnnrag_amd.modules import query_update as mq
    model = mq.bind_reforms(qo.standin(4, 2))
    twin = copy.deepcopy(model)
    b = twin.reform0._qr_bound
    assert b is twin.reform1._qr_bound and b is not model.reform0._qr_bound
    assert b.reforms[0] is twin.reform0 and b.reforms[1] is twin.reform1 and b.instruction is twin.instruction
    assert b.kept is None and twin.reform1._qr_index == 1
    assert list(twin.state_dict()) == list(model.state_dict())
    assert "_qr_bound" not in mq.QueryReform(4).__dict__
