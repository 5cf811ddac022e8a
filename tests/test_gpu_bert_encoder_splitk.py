"""The inference encode on the split-K linear (``ops.bert_encode(..., splitk=True)`` = gnnrag_bert_encode_splitk, and the
patched module under ``GNNRAG_HIP_LM_SPLITK``) against transformers' own models in float64 (tests/bert_oracle.py,
tests/lm_variants_oracle.py; the oracle runs on the CPU).  Bound: ``bert_oracle.bound(e_ref)`` with e_ref the fp32
transformers module's own error against its float64 copy on the same input - never taken from the code under test.  Every
figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

import bert_oracle as bo
import lm_variants_oracle as lo

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "bert_encoder_ref.npz")


@pytest.fixture(scope="module")
def dev():
    pytest.importorskip("transformers")
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


_cases = {}


def _case(shape, L, B, T, seed=11):
    """(fp32 model, ids, float64 states, e_ref) - computed once per case on the CPU and shared."""
    key = (tuple(sorted(shape.items())), L, B, T, seed)
    if key not in _cases:
        m32, m64 = bo.make_model(bo.config(L=L, vocab=64, max_pos=32, **shape), seed)
        ids = np.random.RandomState(seed + 1).randint(0, 64, (B, T))
        want = bo.states(m64, ids)
        _cases[key] = (m32, ids, want, bo.rel_err(bo.states(m32, ids), want))
    return _cases[key]


def _encode(dev, model, ids, splitk=True):
    from gnnrag_amd import ops
    P = bo.layer_params(model)
    layers = [{k: v.detach().to(dev) for k, v in d.items()} for d in P.pop("layers")]
    P = {k: (v.detach().to(dev) if isinstance(v, torch.Tensor) else v) for k, v in P.items()}
    return ops.bert_encode(torch.from_numpy(ids).long().to(dev), P["word_emb"], P["pos_emb"], P["type_emb"], P["ln_g"],
                           P["ln_b"], P["eps"], layers, P["heads"], I=P["I"], splitk=splitk)


ENCODE = [(bo.MINILM, 1, 1, 1), (bo.MINILM, 2, 5, 20), (bo.BERT_BASE, 1, 2, 7)]


@pytest.mark.parametrize("shape,L,B,T", ENCODE, ids=["minilm-L1-1x1", "minilm-L2-5x20", "base-L1-2x7"])
def test_encode_against_float64(dev, shape, L, B, T):
    m32, ids, want, e_ref = _case(shape, L, B, T)
    got = _encode(dev, m32, ids)
    err = bo.rel_err(got.cpu().numpy(), want)
    print("split-K encode H=%d L=%d B=%d T=%d: err %.3g, e_ref %.3g, ratio %.2f, bound %.3g"
          % (shape["H"], L, B, T, err, e_ref, err / max(e_ref, 1e-30), bo.bound(e_ref)))
    assert got.shape == want.shape
    assert err <= bo.bound(e_ref)
    assert torch.equal(got, _encode(dev, m32, ids))                              # the same call twice: equal bits


@pytest.mark.parametrize("arch,dh", [("roberta", 64), ("mpnet", 32)])
def test_variants_against_float64(dev, arch, dh):
    """RoBERTa's positions from ids with pads in them; MPNet without a token-type term and with its attention bias."""
    from gnnrag_amd import ops
    B, T = 4, 9
    m32, m64 = lo.make_model(arch, lo.config(arch, L=2, **lo.SMALL[dh]), seed=41)
    ids = lo.ids_with_pads(B, T)
    want = lo.states(m64, ids)
    e_ref = bo.rel_err(lo.states(m32, ids), want)
    P = lo.layer_params(m32, T)
    layers = [{k: v.detach().to(dev) for k, v in d.items()} for d in P["layers"]]
    top = {k: (None if P[k] is None else P[k].detach().to(dev)) for k in ("word_emb", "pos_emb", "type_emb", "ln_g", "ln_b",
                                                                          "rel_bias")}
    got = ops.bert_encode(torch.from_numpy(ids).long().to(dev), top["word_emb"], top["pos_emb"], top["type_emb"],
                          top["ln_g"], top["ln_b"], P["eps"], layers, P["heads"], I=P["I"], pad_id=P["pad_id"],
                          rel_bias=top["rel_bias"], splitk=True)
    err = bo.rel_err(got.cpu().numpy(), want)
    print("split-K %s: err %.3g, e_ref %.3g, bound %.3g" % (arch, err, e_ref, bo.bound(e_ref)))
    assert (arch == "mpnet") == (top["rel_bias"] is not None) == (top["type_emb"] is None) and P["pad_id"] == lo.PAD
    assert err <= bo.bound(e_ref)


def test_a_question_does_not_depend_on_the_batch(dev):
    m32, ids, _, _ = _case(bo.MINILM, 2, 5, 20)
    batch = _encode(dev, m32, ids)
    for b in (0, 4):
        assert torch.equal(_encode(dev, m32, ids[b:b + 1]), batch[b:b + 1])


# -- the module -------------------------------------------------------------------------------------------------------------

def _fixture_module(dev):
    g = np.load(GOLDEN)
    cfg = bo.config(H=int(g["cfg.H"]), heads=int(g["cfg.heads"]), I=int(g["cfg.I"]), L=int(g["cfg.L"]),
                    vocab=int(g["cfg.vocab"]), max_pos=int(g["cfg.max_pos"]))
    m32, m64 = bo.make_model(cfg, int(g["cfg.seed"]))
    for p in m32.parameters():
        p.requires_grad_(False)
    mod = bo.make_instruction_standin(m32, int(g["cfg.entity_dim"]), int(g["cfg.num_step"]), int(g["cfg.pad_val"]))
    own = {k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param.")}
    missing, unexpected = mod.load_state_dict(own, strict=False)
    assert not unexpected and all(k.startswith("node_encoder.") for k in missing)
    return mod.to(dev).eval(), m64, g


class _Model:
    def __init__(self, instruction):
        self.instruction = instruction


def _patched(dev, monkeypatch):
    from gnnrag_amd import install
    mod, m64, g = _fixture_module(dev)
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    install.patch_lm_encoder(_Model(mod))
    p = mod.node_encoder._gnnrag_lm_patch
    calls, orig = [], p.orig_forward

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    p.orig_forward = counted
    return mod, m64, g, p, calls


def test_patched_module_with_the_switch_reproduces_the_fixture(dev, monkeypatch):
    mod, m64, g, p, calls = _patched(dev, monkeypatch)
    monkeypatch.setenv("GNNRAG_HIP_LM_SPLITK", "1")
    q = torch.from_numpy(g["q_input"]).long().to(dev)
    with torch.no_grad():
        got = mod.node_encoder(q)[0]
    assert (p.hip_calls, p.hip_splitk_calls, p.hip_train_calls) == (1, 1, 0) and not calls
    want = bo.states(m64, g["q_input"])
    e_ref = float(g["lm.e_ref"])
    err = bo.rel_err(got.cpu().numpy(), want)
    print("fixture LM states, split-K: err %.3g, e_ref %.3g (recorded by the reference's fp32 run), bound %.3g"
          % (err, e_ref, bo.bound(e_ref)))
    assert err <= bo.bound(e_ref)
    # the switch is read at every call, and the row bound with it
    monkeypatch.setenv("GNNRAG_HIP_LM_SPLITK", "0")
    with torch.no_grad():
        mod.node_encoder(q)
    assert (p.hip_calls, p.hip_splitk_calls) == (2, 1)
    monkeypatch.setenv("GNNRAG_HIP_LM_SPLITK", "1")
    from gnnrag_amd.modules.question_encoding import lm_encoder as lm
    monkeypatch.setattr(lm, "SPLITK_MAX_ROWS", q.numel() - 1)
    with torch.no_grad():
        mod.node_encoder(q)
    assert (p.hip_calls, p.hip_splitk_calls) == (3, 1) and not calls


def test_patched_module_without_the_switch_is_the_default_call(dev, monkeypatch):
    mod, _, g, p, calls = _patched(dev, monkeypatch)
    monkeypatch.delenv("GNNRAG_HIP_LM_SPLITK", raising=False)
    q = torch.from_numpy(g["q_input"]).long().to(dev)
    with torch.no_grad():
        got = mod.node_encoder(q)[0]
    assert (p.hip_calls, p.hip_splitk_calls) == (1, 0) and not calls
    assert torch.equal(got, _encode(dev, mod.node_encoder, g["q_input"], splitk=False))


def test_training_mode_never_takes_the_split_k_path(dev, monkeypatch):
    """Active dropout with the training forward on: ``bert_encode_train`` serves the call; with it off: transformers."""
    mod, _, g, p, calls = _patched(dev, monkeypatch)
    monkeypatch.setenv("GNNRAG_HIP_LM_SPLITK", "1")
    q = torch.from_numpy(g["q_input"]).long().to(dev)
    mod.train()
    assert mod.node_encoder.config.hidden_dropout_prob == 0.1
    monkeypatch.setenv("GNNRAG_HIP_LM_TRAIN", "1")
    with torch.no_grad():
        mod.node_encoder(q)
    assert (p.hip_calls, p.hip_train_calls, p.hip_splitk_calls) == (1, 1, 0) and not calls
    monkeypatch.setenv("GNNRAG_HIP_LM_TRAIN", "0")
    with torch.no_grad():
        mod.node_encoder(q)
    assert (p.hip_calls, p.hip_train_calls, p.hip_splitk_calls) == (1, 1, 0) and len(calls) == 1
    mod.eval()
    with torch.no_grad():
        mod.node_encoder(q)
    assert (p.hip_calls, p.hip_splitk_calls) == (2, 1)
