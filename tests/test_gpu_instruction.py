"""gnnrag_instructions / ops.instructions / patch_instruction on the MI355X against the float64 oracle
(tests/instruction_oracle.py) and the live reference's fixture (tests/golden/lstm_encoder.npz).

Tolerance 2e-5 absolute, the bound tests/test_gpu_lstm.py:164-165 applies to these very arrays: both sides are fp32 with
different summation orders, the values (convex combinations of LSTM states, softmax weights) lie in [-1, 1]."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import instruction_oracle as io

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "lstm_encoder.npz")
TOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _to(dev, a):
    return [torch.from_numpy(x).to(dev) for x in a] if isinstance(a, list) else torch.from_numpy(a).to(dev)


def _run(dev, c, **kw):
    from gnnrag_amd import ops
    return ops.instructions(*[_to(dev, c[k]) for k in io.ARGS], **kw)


def _err(got, want):
    return float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())


@pytest.mark.parametrize("tag", ["d50", "d128"])
def test_fixture_parity(dev, tag):
    c = io.fixture_case(np.load(GOLDEN), tag)
    want_ins, want_attn = io.instructions(*[c[k] for k in io.ARGS])
    ins, attn = _run(dev, c)
    errs = {"ins vs fixture": _err(ins, c["want_ins"]), "attn vs fixture": _err(attn, c["want_attn"]),
            "ins vs oracle": _err(ins, want_ins), "attn vs oracle": _err(attn, want_attn)}
    print(tag, errs)
    assert max(errs.values()) <= TOL, errs


# (B, T, D, I): one token; D no multiple of 64; D % 4 == 0 but T D odd rows; more questions than one wave's worth; T over 64
# lanes; D over 256; the maximum step count; T D = 16384, the working set above 64 KB of LDS (the raised cap)
SWEEP = [(1, 1, 50, 1), (3, 13, 200, 2), (2, 5, 52, 3), (65, 9, 64, 2), (4, 70, 200, 3), (2, 3, 260, 2), (2, 4, 64, 8),
         (2, 64, 256, 2)]


@pytest.mark.parametrize("B,T,D,I", SWEEP)
def test_shape_sweep_against_the_oracle(dev, B, T, D, I):
    c = io.random_case(B, T, D, I, seed=B + T + D + I)
    want_ins, want_attn = io.instructions(*[c[k] for k in io.ARGS])
    ins, attn = _run(dev, c)
    assert tuple(ins.shape) == (I, B, D) and tuple(attn.shape) == (I, B, T)
    errs = (_err(ins, want_ins), _err(attn, want_attn))
    print((B, T, D, I), errs)
    assert max(errs) <= TOL, errs
    ins2, attn2 = _run(dev, c)
    assert torch.equal(ins, ins2) and torch.equal(attn, attn2)                 # one fixed summation order
    a = attn.cpu().numpy()
    assert np.abs(a.astype(np.float64).sum(-1) - 1.0).max() <= 1e-6
    mask = c["mask"]
    real = mask.any(1)
    assert (a[:, real][:, mask[real] == 0] == 0).all()                         # padding of a question with a real token
    if B > 1:
        assert not real[-1] and real[0] and mask[0].all()
        assert np.abs(a[:, -1] - np.float32(1.0) / np.float32(T)).max() <= 1e-7    # padding only: uniform


@pytest.mark.parametrize("B,T,D,I", [(3, 13, 200, 3), (2, 5, 52, 3)])
def test_chained_single_steps_give_the_bits_of_the_one_call(dev, B, T, D, I):
    from gnnrag_amd import ops
    c = io.random_case(B, T, D, I, seed=7)
    args = {k: _to(dev, c[k]) for k in io.ARGS}

    def steps(lo, hi, r_in):
        a = dict(args, W_q=args["W_q"][lo:hi], b_q=args["b_q"][lo:hi])
        return ops.instructions(*[a[k] for k in io.ARGS], r_in=r_in)

    ins, attn = steps(0, I, None)
    for zero in (None, torch.zeros(B, D, device=dev)):
        ins0, attn0 = steps(0, 1, zero)
        assert torch.equal(ins0[0], ins[0]) and torch.equal(attn0[0], attn[0])
        # steps 1 .. I-1 in one call, then one by one
        rest_i, rest_a = steps(1, I, ins0[0])
        assert torch.equal(rest_i, ins[1:]) and torch.equal(rest_a, attn[1:])
        r = ins0[0]
        for s in range(1, I):
            one_i, one_a = steps(s, s + 1, r)
            assert torch.equal(one_i[0], ins[s]) and torch.equal(one_a[0], attn[s])
            r = one_i[0]


def test_call_is_safe_under_stream_capture(dev):
    """No allocation, no host read, no stream wait inside the call: captured into a graph (after one eager call, which also
    raises the kernel's LDS cap for this shape) and replayed on new input values it gives the eager call's bits."""
    from gnnrag_amd import ops
    c = io.random_case(2, 64, 256, 2, seed=9)
    t = [_to(dev, c[k]) for k in io.ARGS]
    ops.instructions(*t)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ins, attn = ops.instructions(*t)
    t[0].copy_(torch.tanh(torch.randn_like(t[0])))                  # new token states in the captured buffers
    graph.replay()
    want_ins, want_attn = ops.instructions(*t)
    assert torch.equal(ins, want_ins) and torch.equal(attn, want_attn)


def test_unsupported_shapes_raise_the_bindings_error(dev):
    from gnnrag_amd import _lib, ops
    c = io.random_case(1, 2, 8, 9, seed=0)
    with pytest.raises(_lib.GnnragError, match=r"\(-2\)"):
        _run(dev, c)
    assert not ops.instructions_supported(2, 8, 9)


# -- the module layer --------------------------------------------------------------------------------------------------

def _reference_module(dev, tag="d50"):
    """The reference's own LSTMInstruction (staged under oracle/_ref/gnn) with the fixture's parameters."""
    import tempfile
    ref = os.path.join(REPO, "oracle", "_ref", "gnn")
    if not os.path.isfile(os.path.join(ref, "modules", "question_encoding", "lstm_encoder.py")):
        pytest.skip("oracle/_ref not staged")
    sys.path.insert(0, ref)
    try:
        from modules.question_encoding import base_encoder, lstm_encoder
    finally:
        sys.path.remove(ref)
    g = np.load(GOLDEN)
    P = {k.split(".param.")[1]: torch.from_numpy(g[k]) for k in g.files if k.startswith(tag + ".param.")}
    text = g[tag + ".query_text"]
    vocab = int(text.max())
    word_dim, entity_dim = P["node_encoder.weight_ih_l0"].shape[1], P["node_encoder.weight_hh_l0"].shape[1]
    folder = tempfile.mkdtemp() + "/"
    with open(folder + "vocab.txt", "w") as f:
        f.write("\n".join("w%d" % i for i in range(vocab)) + "\n")
    args = dict(use_cuda=True, q_type="seq", num_step=3, lm_dropout=0.0, linear_dropout=0.0, lm_frozen=0, word_dim=word_dim,
                entity_dim=entity_dim, data_folder=folder, word2id="vocab.txt")
    init = base_encoder.BaseInstruction.__init__
    base_encoder.BaseInstruction.__init__ = lambda self, a, constraint=False: init(self, a, constraint)
    try:
        enc = lstm_encoder.LSTMInstruction(args, nn.Embedding(vocab + 1, word_dim, padding_idx=vocab), vocab)
    finally:
        base_encoder.BaseInstruction.__init__ = init
    enc.load_state_dict(P, strict=True)
    return enc.to(dev).eval(), torch.from_numpy(text).long().to(dev), g, vocab


def _standin_module(dev):
    torch.manual_seed(11)
    mod = io.make_standin(20, 52, 3, num_word=30, device=dev).eval()
    rng = np.random.default_rng(5)
    text = rng.integers(0, 30, (4, 6))
    text[1, 2:] = 30
    text[3, :] = 30                             # a question of padding only
    return mod, torch.from_numpy(text).long().to(dev), None, 30


@pytest.fixture(params=["reference", "standin"])
def patched(request, dev, monkeypatch):
    """(module, question tensor, pad id, counters): the encoder after install.swap_lstm and patch_instruction, the switch
    on, ops.instructions and ops.lstm_forward counted."""
    from gnnrag_amd import install, ops
    from gnnrag_amd.modules.question_encoding.instruction import patch_instruction
    from gnnrag_amd.modules.question_encoding.lstm import HipLSTM
    mod, q, _, pad = (_reference_module if request.param == "reference" else _standin_module)(dev)
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION", "1")
    assert install.swap_lstm(mod) == 1 and isinstance(mod.node_encoder, HipLSTM)
    assert patch_instruction(mod) is mod
    count = {"instructions": 0, "lstm_forward": 0, "n_steps": []}
    ins_fn, lstm_fn = ops.instructions, ops.lstm_forward

    def instructions(*a, **k):
        count["instructions"] += 1
        count["n_steps"].append(len(a[3]))
        return ins_fn(*a, **k)

    def lstm_forward(*a, **k):
        count["lstm_forward"] += 1
        return lstm_fn(*a, **k)

    monkeypatch.setattr(ops, "instructions", instructions)
    monkeypatch.setattr(ops, "lstm_forward", lstm_forward)
    return mod, q, pad, count


@pytest.mark.parametrize("tag", ["d50", "d128"])
def test_reference_module_patched_reproduces_the_fixture(dev, monkeypatch, tag):
    from gnnrag_amd import install
    from gnnrag_amd.modules.question_encoding.instruction import patch_instruction
    enc, q, g, _ = _reference_module(dev, tag)
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION", "1")
    assert install.swap_lstm(enc) == 1
    patch_instruction(enc)
    with torch.no_grad():
        instructions, attn = enc(q)
    assert len(instructions) == 3 and instructions[0].shape == g[tag + ".instructions"].shape[1:]
    assert attn[0].shape == g[tag + ".attn"].shape[1:]                              # [B, T, 1]
    assert enc.instructions is instructions and enc.attn_list is attn and enc.relational_ins is instructions[-1]
    assert _err(torch.stack(instructions), g[tag + ".instructions"]) <= TOL
    assert _err(torch.stack(attn), g[tag + ".attn"]) <= TOL


def _rearev_sequence(mod, q):
    ins, attn = mod(q)
    first = list(ins)
    mod.init_reason(q)
    assert mod.instructions == [] and mod.attn_list == []
    assert tuple(mod.relational_ins.shape) == tuple(first[0].shape) and not mod.relational_ins.any()
    steps = []
    for i in range(mod.num_ins):                                    # rearev.py:192-196
        r, a = mod.get_instruction(mod.relational_ins, step=i)
        mod.instructions.append(r.unsqueeze(1))
        mod.relational_ins = r
        steps.append((r, a))
    return first, list(attn), steps


def test_rearev_sequence_is_one_encode_and_one_instruction_launch(patched):
    mod, q, _, count = patched
    with torch.no_grad():
        first, attn, steps = _rearev_sequence(mod, q)
    assert (count["lstm_forward"], count["instructions"], count["n_steps"]) == (1, 1, [mod.num_ins])
    for i, (r, a) in enumerate(steps):
        assert r is first[i] and a is attn[i]
    want_ins, want_attn = io.standin_oracle(mod)
    assert _err(torch.stack(first), want_ins) <= TOL and _err(torch.stack(attn)[..., 0], want_attn) <= TOL
    B, T, D = mod.query_hidden_emb.shape
    assert tuple(first[0].shape) == (B, D) and tuple(attn[0].shape) == (B, T, 1)
    # the same tensor again: nothing is launched at all; the results are the cached ones
    with torch.no_grad():
        again, _, _ = _rearev_sequence(mod, q)
    assert (count["lstm_forward"], count["instructions"]) == (1, 1) and again[0] is first[0]


def test_invalidation(patched):
    mod, q, pad, count = patched
    seen = lambda: (count["lstm_forward"], count["instructions"])       # noqa: E731
    with torch.no_grad():
        first, _, _ = _rearev_sequence(mod, q)
        assert seen() == (1, 1)
        # a new tensor with equal content
        q2 = q.clone()
        second, _, _ = _rearev_sequence(mod, q2)
        assert seen() == (2, 2) and second[0] is not first[0] and torch.equal(torch.stack(second), torch.stack(first))
        # the same tensor edited in place
        q2[0, 0] = (q2[0, 0] + 1) % pad                                  # another word, computed on the device
        third, _, _ = _rearev_sequence(mod, q2)
        assert seen() == (3, 3)
        # a relational_ins the cache did not produce: one single-step launch
        B, D = first[0].shape
        foreign = torch.tanh(torch.randn(B, D, device=q.device))
        r, a = mod.get_instruction(foreign, step=1)
        assert seen() == (3, 4) and count["n_steps"][-1] == 1
        want_r, want_a = io.standin_oracle(mod, steps=[1], r_in=foreign)
        assert _err(r, want_r[0]) <= TOL and _err(a[..., 0], want_a[0]) <= TOL
        # an equal copy of a cached step is not the cached step either
        mod.get_instruction(third[0].clone(), step=1)
        assert seen() == (3, 5)
        # a node embedding handed in: a single step on it
        node = torch.tanh(torch.randn(B, 1, D, device=q.device))
        r, _ = mod.get_instruction(third[0], step=1, query_node_emb=node)
        assert seen() == (3, 6) and not torch.equal(r, third[1])
        # a parameter edited in place
        mod.cq_linear.weight.add_(0.5)
        fourth, _, _ = _rearev_sequence(mod, q2)
        assert seen() == (4, 7)
        assert not torch.equal(torch.stack(fourth), torch.stack(third))


def test_autograd_and_dropout_run_the_original_methods(patched):
    mod, q, _, count = patched
    mod.train()                      # a training step (both dropout probabilities are 0): the LSTM's backward needs the mode
    with torch.enable_grad():
        assert all(p.requires_grad for p in mod.cq_linear.parameters())
        ins, _ = mod(q)
        mod.init_reason(q)
        r, _ = mod.get_instruction(mod.relational_ins, step=0)
        (ins[-1].sum() + r.sum()).backward()
    assert count["instructions"] == 0
    assert float(mod.cq_linear.weight.grad.abs().sum()) > 0 and float(mod.question_linear0.weight.grad.abs().sum()) > 0
    # training mode with linear dropout: the reference's own ops (and its random numbers)
    mod.linear_drop.p = 0.3
    mod.train()
    with torch.no_grad():
        mod(q)
        assert count["instructions"] == 0
        mod.eval()
        eval_ins, _ = mod(q)
        assert count["instructions"] == 1
        # training mode with both probabilities 0: the fast path again
        mod.linear_drop.p = 0.0
        mod.train()
        train_ins, _ = mod(q)
        assert count["instructions"] == 2 and torch.equal(torch.stack(train_ins), torch.stack(eval_ins))


def test_switch_off_runs_the_reference_ops(patched, monkeypatch):
    mod, q, _, count = patched
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION", "0")
    with torch.no_grad():
        off, _, _ = _rearev_sequence(mod, q)
    assert (count["lstm_forward"], count["instructions"]) == (2, 0)
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION", "1")
    with torch.no_grad():
        on, _, _ = _rearev_sequence(mod, q)
    assert (count["lstm_forward"], count["instructions"]) == (3, 1)
    assert float((torch.stack(on) - torch.stack(off)).abs().max()) <= 2 * TOL        # two fp32 forms of one result
