"""Instruction generation, host side: the float64 oracle of the GPU tests reproduces the live reference's fixture; the entry
point is declared in gnnrag.h and in the binding (additive to ABI 16) and refuses bad arguments before it touches a device;
``patch_instruction`` on CPU tensors is the module's own methods, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import instruction_oracle as io

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "lstm_encoder.npz")
N_ARGS = 17


@pytest.mark.parametrize("tag", ["d50", "d128"])
def test_oracle_reproduces_the_live_reference_fixture(tag):
    c = io.fixture_case(np.load(GOLDEN), tag)
    ins, attn = io.instructions(*[c[k] for k in io.ARGS])
    assert ins.shape == c["want_ins"].shape and attn.shape == c["want_attn"].shape
    assert np.abs(ins - c["want_ins"]).max() <= 1e-6
    assert np.abs(attn - c["want_attn"]).max() <= 1e-6


def test_oracle_gives_a_question_of_padding_only_the_uniform_attention():
    c = io.random_case(3, 5, 8, 2, seed=1)
    assert c["mask"][0].all() and not c["mask"][-1].any()
    _, attn = io.instructions(*[c[k] for k in io.ARGS])
    assert np.abs(attn[:, -1] - 1.0 / 5).max() <= 1e-15


def test_header_and_binding_declare_the_entry_point():
    from gnnrag_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gnnrag.h")).read(), flags=re.S)
    m = re.search(r"\bgnnrag_instructions\s*\(([^)]*)\)\s*;", src)
    assert m, "gnnrag.h does not declare gnnrag_instructions"
    assert len(m.group(1).split(",")) == N_ARGS
    assert "gnnrag_instructions" in _lib.SIGNATURES and len(_lib.SIGNATURES["gnnrag_instructions"][1]) == N_ARGS
    assert re.search(r"#define\s+GNNRAG_MAX_INS\s+8\b", src)
    assert re.search(r"#define\s+GNNRAG_ABI_VERSION\s+16\b", src) and _lib.ABI_VERSION == 16


@pytest.fixture(scope="module")
def lib():
    from gnnrag_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.gnnrag_abi_version() == 16
    return lib


def _call(lib, B=2, T=3, D=4, n=2, null=None, null_in_list=False):
    """Every pointer is a dummy non-NULL address: an argument error must come back before anything is dereferenced on a
    device (there is none here)."""
    p = 4096
    ptrs = dict(hidden=p, node=p, mask=p, W_cq=p, b_cq=p, w_ca=p, b_ca=p, ins_out=p, attn_out=p)
    Wq = (C.c_void_p * 9)(*[p] * 9)
    bq = (C.c_void_p * 9)(*[p] * 9)
    if null_in_list:
        Wq[1] = None
    if null == "W_q":
        Wq = None
    elif null == "b_q":
        bq = None
    elif null is not None:
        ptrs[null] = None
    return lib.gnnrag_instructions(ptrs["hidden"], ptrs["node"], ptrs["mask"], None, Wq, bq, ptrs["W_cq"], ptrs["b_cq"],
                                   ptrs["w_ca"], ptrs["b_ca"], B, T, D, n, ptrs["ins_out"], ptrs["attn_out"], None)


@pytest.mark.parametrize("null", ["hidden", "node", "mask", "W_q", "b_q", "W_cq", "b_cq", "w_ca", "b_ca", "ins_out",
                                  "attn_out"])
def test_null_pointers_are_bad_arguments(lib, null):
    assert _call(lib, null=null) == -1


def test_sizes_and_budget_are_checked_before_anything_is_launched(lib):
    assert _call(lib, null_in_list=True) == -1
    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(D=0), dict(D=-1), dict(n=0), dict(n=-1)):
        assert _call(lib, **kw) == -1, kw
    assert _call(lib, n=9) == -2
    # one question's working set, 4 * (ceil4(T D) + (n + 2) D + T) bytes, must fit 160 KB
    assert _call(lib, T=1, D=40961, n=1) == -2
    assert _call(lib, T=41, D=1000, n=1) == -2
    assert _call(lib, T=8, D=4096, n=8) == -2                 # the token states alone would fit, the vectors do not
    assert _call(lib, T=70000, D=70000, n=1) == -2            # no 32-bit overflow in the check


def test_binding_states_the_same_budget():
    from gnnrag_amd import ops
    assert ops.MAX_INS == 8
    assert ops.instructions_supported(12, 200, 3) and ops.instructions_supported(8, 2048, 8)
    assert ops.instructions_supported(16384, 1, 8) and ops.instructions_supported(1, 1, 1)
    assert not ops.instructions_supported(12, 200, 9) and not ops.instructions_supported(8, 4096, 8)
    assert not ops.instructions_supported(41, 1000, 1) and not ops.instructions_supported(0, 4, 1)


def test_the_wrapper_refuses_cpu_tensors():
    from gnnrag_amd import _lib, ops
    c = io.random_case(2, 3, 4, 1, seed=0)
    t = lambda a: [torch.from_numpy(x) for x in a] if isinstance(a, list) else torch.from_numpy(a)   # noqa: E731
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.instructions(*[t(c[k]) for k in io.ARGS])


def _sequence(mod, q):
    """The ReaRev call sequence (forward, then init_reason and the steps one by one)."""
    with torch.no_grad():
        ins, attn = mod(q)
        first = [t.clone() for t in ins] + [t.clone() for t in attn] + [mod.relational_ins.clone()]
        mod.init_reason(q)
        for i in range(mod.num_ins):
            r, a = mod.get_instruction(mod.relational_ins, step=i)
            mod.instructions.append(r)
            mod.relational_ins = r
            first += [r.clone(), a.clone()]
    return first


@pytest.mark.parametrize("switch", [None, "0", "1"])
def test_patched_module_on_cpu_tensors_is_the_original_bit_for_bit(monkeypatch, switch):
    from gnnrag_amd import ops
    from gnnrag_amd.modules.question_encoding.instruction import patch_instruction
    if switch is None:
        monkeypatch.delenv("GNNRAG_HIP_INSTRUCTION", raising=False)
    else:
        monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION", switch)

    def no_library(*a, **k):
        raise AssertionError("ops.instructions called on CPU tensors")
    monkeypatch.setattr(ops, "instructions", no_library)
    torch.manual_seed(0)
    plain = io.make_standin(6, 8, 3, num_word=20).eval()
    patched = io.make_standin(6, 8, 3, num_word=20).eval()
    patched.load_state_dict(plain.state_dict())
    assert patch_instruction(patched) is patched
    q = torch.tensor([[1, 2, 3, 20, 20], [4, 5, 6, 7, 8], [20, 20, 20, 20, 20]])
    for want, got in zip(_sequence(plain, q), _sequence(patched, q)):
        assert torch.equal(want, got)
    assert len(patched.instructions) == 3 and patched.relational_ins is patched.instructions[-1]
    # a second pass on the same tensor (the repeated-encode rule applies with the switch on) and under autograd
    for want, got in zip(_sequence(plain, q), _sequence(patched, q)):
        assert torch.equal(want, got)
    patched.train()
    ins, _ = patched(q)
    ins[-1].sum().backward()
    assert patched.cq_linear.weight.grad is not None and float(patched.cq_linear.weight.grad.abs().sum()) > 0


def test_patch_instruction_is_idempotent_and_leaves_other_modules_alone():
    from gnnrag_amd.modules.question_encoding.instruction import patch_instruction
    mod = io.make_standin(6, 8, 2, num_word=20)
    keys = list(mod.state_dict())
    patch_instruction(mod)
    wrapped = (mod.forward, mod.init_reason, mod.get_instruction)
    assert patch_instruction(mod) is mod
    assert (mod.forward, mod.init_reason, mod.get_instruction) == wrapped
    assert list(mod.state_dict()) == keys
    other = torch.nn.Linear(3, 3)
    fwd = other.forward
    assert patch_instruction(other) is other and other.forward == fwd and "forward" not in other.__dict__


def test_switch_off_goes_straight_to_the_original_methods(monkeypatch):
    """GNNRAG_HIP_INSTRUCTION=0 is read at every call: the wrappers hand over before they look at anything (here: a
    module whose encoder state would otherwise be inspected holds attributes that raise when touched)."""
    from gnnrag_amd.modules.question_encoding import instruction as mi
    calls = []

    class Probe(torch.nn.Module):
        num_ins = 1

        def __init__(self):
            super().__init__()
            self.cq_linear, self.ca_linear = torch.nn.Linear(4, 1), torch.nn.Linear(1, 1)
            self.question_linear0, self.linear_drop = torch.nn.Linear(1, 1), torch.nn.Dropout(0.0)

        query_hidden_emb = property(lambda self: (_ for _ in ()).throw(AssertionError("state inspected")))

        def init_reason(self, q):
            calls.append(("init_reason", q))

        def get_instruction(self, r, step=0, query_node_emb=None):
            calls.append(("get_instruction", r, step, query_node_emb))
            return "r", "a"

        def forward(self, q, lm=None):
            calls.append(("forward", q, lm))
            return "f"

    mod = mi.patch_instruction(Probe())
    assert "forward" in mod.__dict__
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION", "0")
    assert not mi.enabled()
    assert mod("q") == "f" and mod.get_instruction("r0", 0, "n") == ("r", "a")
    mod.init_reason("q2")
    assert calls == [("forward", "q", None), ("get_instruction", "r0", 0, "n"), ("init_reason", "q2")]
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION", "1")
    assert mi.enabled()
    monkeypatch.delenv("GNNRAG_HIP_INSTRUCTION")
    assert mi.enabled() == (mi.DEFAULT != "0")
