"""The frozen BERT-class question encoder on the MI355X against transformers' own BertModel in float64 (tests/bert_oracle.py;
the oracle runs on the CPU).

Bound of every LM-state comparison: the error relative to the oracle's largest entry is at most max(4 x e_ref, 1e-6), where
e_ref is the fp32 transformers module's own error against its float64 copy on the same input, computed here on the CPU - the
bound never comes from the code under test.  The factor 4 is the margin tests/test_gpu_rel_text.py gives a kernel whose
summation order differs from the CPU's.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

import bert_oracle as bo

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "bert_encoder_ref.npz")
MATH_FP32, MATH_BF16X3 = 0, 1
TOL_INS = 2e-5                                  # tests/test_gpu_instruction.py: the same arrays


@pytest.fixture(scope="module")
def dev():
    pytest.importorskip("transformers")
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


_cases = {}


def _case(shape, L, B, T, seed=11, max_pos=32):
    """(fp32 model, float64 model, ids, float64 states, e_ref) - computed once per case on the CPU and shared."""
    key = (tuple(sorted(shape.items())), L, B, T, seed, max_pos)
    if key not in _cases:
        m32, m64 = bo.make_model(bo.config(L=L, vocab=64, max_pos=max_pos, **shape), seed)
        ids = np.random.RandomState(seed + 1).randint(0, 64, (B, T))
        want = bo.states(m64, ids)
        _cases[key] = (m32, m64, ids, want, bo.rel_err(bo.states(m32, ids), want))
    return _cases[key]


def _encode(dev, model, ids, math=None, L=None):
    from gnnrag_amd import ops
    P = bo.layer_params(model)
    layers = P.pop("layers")
    if L is not None:
        layers = layers[:L]
    P = {k: (v.detach().to(dev) if isinstance(v, torch.Tensor) else v) for k, v in P.items()}
    layers = [{k: v.detach().to(dev) for k, v in d.items()} for d in layers]
    return ops.bert_encode(torch.from_numpy(ids).long().to(dev), P["word_emb"], P["pos_emb"], P["type_emb"], P["ln_g"],
                           P["ln_b"], P["eps"], layers, P["heads"], I=P["I"], math=math)


# -- attention alone -------------------------------------------------------------------------------------------------

# a single key; several waves; a full wave of keys; the first key in a lane's second slot; the largest T
ATT = [(2, 1, 1, 32), (3, 9, 2, 32), (1, 64, 2, 64), (1, 65, 12, 32), (1, 128, 1, 64)]


@pytest.mark.parametrize("B,T,heads,dh", ATT)
def test_attention_against_float64(dev, B, T, heads, dh):
    """fp32 against float64: a T-term dot product of q and k, exp, a T-term sum and a T-term weighted sum, each within a
    few ulp per term.  The bound is that of the LM states with the fp32 torch statement of the same step as e_ref."""
    from gnnrag_amd import ops
    rs = np.random.RandomState(100 + T)
    qkv = rs.standard_normal((B * T, 3 * heads * dh)).astype(np.float32)
    want = bo.attention64(qkv, B, T, heads, dh)
    x = torch.from_numpy(qkv).view(B, T, 3, heads, dh)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    ref32 = torch.nn.functional.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(B * T, heads * dh)
    e_ref = bo.rel_err(ref32.numpy(), want)
    got = ops.bert_attention(torch.from_numpy(qkv).to(dev), B, T, heads, dh)
    err = bo.rel_err(got.cpu().numpy(), want)
    print("attention B=%d T=%d heads=%d dh=%d: err %.3g, e_ref %.3g, ratio %.2f" % (B, T, heads, dh, err, e_ref,
                                                                                   err / max(e_ref, 1e-30)))
    assert got.shape == (B * T, heads * dh)
    assert err <= bo.bound(e_ref)
    again = ops.bert_attention(torch.from_numpy(qkv).to(dev), B, T, heads, dh)
    assert torch.equal(got, again)


@pytest.mark.parametrize("T,heads,dh", [(9, 2, 32), (65, 12, 32), (128, 1, 64)])
def test_attention_bits_do_not_depend_on_the_batch(dev, T, heads, dh):
    from gnnrag_amd import ops
    qkv = torch.from_numpy(np.random.RandomState(7).standard_normal((3 * T, 3 * heads * dh)).astype(np.float32)).to(dev)
    batch = ops.bert_attention(qkv, 3, T, heads, dh).view(3, T, heads * dh)
    for b in range(3):
        alone = ops.bert_attention(qkv[b * T:(b + 1) * T].contiguous(), 1, T, heads, dh)
        assert torch.equal(alone, batch[b])


# -- the whole encode -------------------------------------------------------------------------------------------------

def test_embedding_layernorm_at_the_last_position(dev):
    """L = 0 at T = max_pos: the embedding LayerNorm alone, the last row of the position table included."""
    m32, m64, ids, _, _ = _case(bo.MINILM, 1, 2, 32)
    with torch.no_grad():
        want = m64.embeddings(input_ids=torch.from_numpy(ids)).numpy()
        e_ref = bo.rel_err(m32.embeddings(input_ids=torch.from_numpy(ids)).numpy(), want)
    got = _encode(dev, m32, ids, L=0)
    err = bo.rel_err(got.cpu().numpy(), want)
    print("L=0 T=max_pos=32: err %.3g, e_ref %.3g" % (err, e_ref))
    assert got.shape == (2, 32, 384)
    assert err <= bo.bound(e_ref)


ENCODE = [(bo.MINILM, 1, 1, 1), (bo.MINILM, 1, 3, 9), (bo.MINILM, 2, 5, 20), (bo.BERT_BASE, 1, 2, 7), (bo.MINILM, 6, 4, 12)]


@pytest.mark.parametrize("math", [MATH_FP32, MATH_BF16X3], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("shape,L,B,T", ENCODE, ids=["minilm-L1-1x1", "minilm-L1-3x9", "minilm-L2-5x20", "base-L1-2x7",
                                                      "minilm-L6-4x12"])
def test_encode_against_float64(dev, shape, L, B, T, math):
    m32, _, ids, want, e_ref = _case(shape, L, B, T)
    got = _encode(dev, m32, ids, math=math)
    err = bo.rel_err(got.cpu().numpy(), want)
    print("encode H=%d L=%d B=%d T=%d math=%d: err %.3g, e_ref %.3g, ratio %.2f, bound %.3g"
          % (shape["H"], L, B, T, math, err, e_ref, err / max(e_ref, 1e-30), bo.bound(e_ref)))
    assert got.shape == want.shape
    assert err <= bo.bound(e_ref)
    assert torch.equal(got, _encode(dev, m32, ids, math=math))                   # the same call twice: equal bits


def test_a_question_does_not_depend_on_the_batch(dev):
    m32, _, ids, _, _ = _case(bo.MINILM, 2, 5, 20)
    batch = _encode(dev, m32, ids)
    for b in (0, 4):
        assert torch.equal(_encode(dev, m32, ids[b:b + 1]), batch[b:b + 1])


# -- the module ---------------------------------------------------------------------------------------------------------

def _fixture_module(dev):
    g = np.load(GOLDEN)
    cfg = bo.config(H=int(g["cfg.H"]), heads=int(g["cfg.heads"]), I=int(g["cfg.I"]), L=int(g["cfg.L"]),
                    vocab=int(g["cfg.vocab"]), max_pos=int(g["cfg.max_pos"]))
    m32, m64 = bo.make_model(cfg, int(g["cfg.seed"]))
    for p in m32.parameters():
        p.requires_grad_(False)                 # lm_frozen = 1 (bert_encoder.py:80-83)
    mod = bo.make_instruction_standin(m32, int(g["cfg.entity_dim"]), int(g["cfg.num_step"]), int(g["cfg.pad_val"]))
    own = {k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param.")}
    missing, unexpected = mod.load_state_dict(own, strict=False)
    assert not unexpected and all(k.startswith("node_encoder.") for k in missing)
    return mod.to(dev).eval(), m64, g


class _Model:
    """What ``install.patch_lm_encoder`` / ``patch_instruction`` are given: an object with an ``instruction``."""

    def __init__(self, instruction):
        self.instruction = instruction


def _count_original(mod):
    p = mod.node_encoder._gnnrag_lm_patch
    calls, orig = [], p.orig_forward

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    p.orig_forward = counted
    return p, calls


@pytest.mark.parametrize("hip_instruction", ["0", "1"])
def test_patched_module_reproduces_the_reference_fixture(dev, monkeypatch, hip_instruction):
    from gnnrag_amd import install
    mod, m64, g = _fixture_module(dev)
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION", hip_instruction)
    install.patch_lm_encoder(_Model(mod))
    install.patch_instruction(_Model(mod))
    p, calls = _count_original(mod)
    q = torch.from_numpy(g["q_input"]).long().to(dev)
    with torch.no_grad():
        instructions, attn = mod(q)
    assert p.hip_calls == 1 and not calls
    want = bo.states(m64, g["q_input"])
    e_ref = float(g["lm.e_ref"])
    err = bo.rel_err(mod.lm_states.cpu().numpy(), want)
    print("fixture LM states: err %.3g, e_ref %.3g (recorded by the reference's fp32 run), bound %.3g"
          % (err, e_ref, bo.bound(e_ref)))
    assert err <= bo.bound(e_ref)
    figs = {"query_hidden_emb": np.abs(mod.query_hidden_emb.cpu().numpy() - g["query_hidden_emb"]).max(),
            "instructions": np.abs(torch.stack(instructions).cpu().numpy() - g["instructions"]).max(),
            "attn": np.abs(torch.stack(attn).cpu().numpy() - g["attn"]).max()}
    print("fixture, GNNRAG_HIP_INSTRUCTION=%s: %s" % (hip_instruction, figs))
    assert all(v <= TOL_INS for v in figs.values()), figs


def test_training_mode_with_dropout_falls_through(dev, monkeypatch):
    """Trainer_KBQA runs the frozen LM in training mode (dropout 0.1): transformers' own forward, counted."""
    from gnnrag_amd import install
    mod, _, g = _fixture_module(dev)
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    install.patch_lm_encoder(_Model(mod))
    p, calls = _count_original(mod)
    q = torch.from_numpy(g["q_input"]).long().to(dev)
    mod.train()
    assert mod.node_encoder.config.hidden_dropout_prob == 0.1
    with torch.no_grad():
        out = mod.node_encoder(q)
    assert len(calls) == 1 and p.hip_calls == 0 and hasattr(out, "pooler_output")
    mod.eval()
    with torch.no_grad():
        out = mod.node_encoder(q)
        assert len(calls) == 1 and p.hip_calls == 1 and not hasattr(out, "pooler_output")
        mod.node_encoder(q, attention_mask=torch.ones_like(q))
    assert len(calls) == 2 and p.hip_calls == 1


def test_lstm_model_is_untouched_by_the_lm_patch(dev):
    """A model whose encoder is the LSTM (HipLSTM after swap_lstm) goes through install.patch_lm_encoder unchanged."""
    import instruction_oracle as io
    from gnnrag_amd import install
    from gnnrag_amd.modules.question_encoding.lstm import HipLSTM
    mod = io.make_standin(20, 52, 3, num_word=30, device=dev).eval()
    model = _Model(mod)
    assert install.swap_lstm(mod) == 1 and isinstance(mod.node_encoder, HipLSTM)
    enc, fwd, keys = mod.node_encoder, mod.node_encoder.forward, list(mod.state_dict().keys())
    assert install.patch_lm_encoder(model) is model
    assert mod.node_encoder is enc and enc.forward == fwd and not hasattr(enc, "_gnnrag_lm_patch")
    assert list(mod.state_dict().keys()) == keys
