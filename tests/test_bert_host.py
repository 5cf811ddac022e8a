"""Host side of the BERT question encoder (CPU, no GPU): the float64 oracle against the live reference's fixture, the rules
of ``patch_lm_encoder`` one by one, and the argument rules of the new entry points (answered before a device is touched)."""
import copy
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import bert_oracle as bo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "bert_encoder_ref.npz")
E_UNSUPPORTED, E_BADARG = -2, -1


@pytest.fixture(scope="module")
def lib():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def small():
    """A small BERT (H=64, 2 heads of 32, 1 layer) and its float64 copy."""
    pytest.importorskip("transformers")
    return bo.make_model(bo.config(H=64, heads=2, I=128, L=1, vocab=50, max_pos=16), seed=5)


def _ids(B=2, T=5, vocab=50, seed=0):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, vocab, (B, T))).long()


class _Holder:
    """What ``patch_lm_encoder`` is given: an object with a ``node_encoder``."""

    def __init__(self, enc):
        self.node_encoder = enc


def _patched(model, count=True):
    """A private copy of ``model``, patched, its original forward counted."""
    from gnnrag_amd.modules.question_encoding.lm_encoder import patch_lm_encoder
    enc = copy.deepcopy(model)
    h = _Holder(enc)
    assert patch_lm_encoder(h) is h
    p = enc._gnnrag_lm_patch
    if not count:
        return enc, p, None
    calls, orig = [], p.orig_forward

    def counted(*a, **k):
        calls.append((a, k))
        return orig(*a, **k)

    p.orig_forward = counted
    return enc, p, calls


# -- the oracle and the fixture ---------------------------------------------------------------------------------------

def test_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(GOLDEN) < 200 * 1024
    g = np.load(GOLDEN, allow_pickle=False)
    assert not any(k.startswith("param.node_encoder") for k in g.files)
    q = g["q_input"]
    pad = int(g["cfg.pad_val"])
    assert q.shape == (3, 9) and (q[0] != pad).all() and (q[1, :5] != pad).all() and (q[1, 5:] == pad).all()
    assert q[2, 0] != pad and (q[2, 1:] == pad).all()


def test_oracle_reproduces_the_reference_lm_states():
    """The float64 module built from the fixture's seed against the LM states of the live reference's fp32 run: their
    distance is the reference's own fp32 error, which the fixture recorded against ITS float64 run (same weights)."""
    pytest.importorskip("transformers")
    g = np.load(GOLDEN)
    cfg = bo.config(H=int(g["cfg.H"]), heads=int(g["cfg.heads"]), I=int(g["cfg.I"]), L=int(g["cfg.L"]),
                    vocab=int(g["cfg.vocab"]), max_pos=int(g["cfg.max_pos"]))
    _, m64 = bo.make_model(cfg, int(g["cfg.seed"]))
    err, e_ref = bo.rel_err(g["lm.states"], bo.states(m64, g["q_input"])), float(g["lm.e_ref"])
    print("oracle vs fixture %.3g, recorded e_ref %.3g" % (err, e_ref))
    assert 0.0 < e_ref < 1e-5
    assert err <= e_ref * 1.001          # float64 on another host moves the figure by parts in 1e9, not more


# -- the patch ---------------------------------------------------------------------------------------------------------

def test_rules_one_by_one(small, monkeypatch):
    """Each rule refuses on its own (everything else as an eligible call has it, up to the device rules, which on this
    host refuse last), every refused call is the unpatched forward bit for bit, and the original runs exactly once."""
    model = small[0]
    ids = _ids()
    with torch.no_grad():
        want = model(ids)[0]
        want_mask = model(ids, attention_mask=torch.ones_like(ids))[0]

    def run(enc, calls, *a, **k):
        n = len(calls)
        out = enc(*a, **k)
        assert len(calls) == n + 1
        return out[0]

    enc, p, calls = _patched(model)
    for q in p.enc.parameters():
        q.requires_grad_(False)
    monkeypatch.setenv("GNNRAG_HIP_LM", "0")
    assert p.refusal((ids,), {}) == "GNNRAG_HIP_LM is off"
    with torch.no_grad():
        assert torch.equal(run(enc, calls, ids), want)
    monkeypatch.delenv("GNNRAG_HIP_LM", raising=False)                           # unset: on
    assert p.refusal((ids,), {}) == "input_ids is not a CUDA tensor"
    monkeypatch.setenv("GNNRAG_HIP_LM", "0")
    assert p.refusal((ids,), {}) == "GNNRAG_HIP_LM is off"                       # read at every call
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    # with the switch on and a frozen eval-mode model only the device is in the way on this host
    assert p.refusal((ids,), {}) == "input_ids is not a CUDA tensor"
    assert p.refusal((), {"input_ids": ids}) == "input_ids is not a CUDA tensor"
    with torch.no_grad():
        assert torch.equal(run(enc, calls, ids), want)
        assert torch.equal(run(enc, calls, input_ids=ids), want)
    # an attention mask, token types, embeddings instead of ids
    assert p.refusal((ids,), {"attention_mask": torch.ones_like(ids)}) == "arguments other than input_ids"
    assert p.refusal((ids, torch.ones_like(ids)), {}) == "arguments other than input_ids"
    assert p.refusal((), {"inputs_embeds": torch.zeros(2, 5, 64)}) == "arguments other than input_ids"
    assert p.refusal((), {}) == "arguments other than input_ids"
    with torch.no_grad():
        assert torch.equal(run(enc, calls, ids, attention_mask=torch.ones_like(ids)), want_mask)
    # ids of another type or rank
    assert p.refusal((ids.int(),), {}) == "input_ids is not a 2-D int64 tensor"
    assert p.refusal((ids[0],), {}) == "input_ids is not a 2-D int64 tensor"
    # a gradient is needed: grad mode on AND a parameter that requires one
    assert p.refusal((ids,), {}) == "input_ids is not a CUDA tensor"            # grad mode on, frozen: no objection
    next(p.enc.parameters()).requires_grad_(True)
    assert p.refusal((ids,), {}) == "a gradient is needed"
    assert torch.equal(run(enc, calls, ids).detach(), want)
    with torch.no_grad():
        assert p.refusal((ids,), {}) == "input_ids is not a CUDA tensor"
    next(p.enc.parameters()).requires_grad_(False)
    # dropout: training mode with the configuration's 0.1 refuses, with both probabilities 0 it does not
    enc.train()
    assert p.refusal((ids,), {}) == "dropout is active"
    torch.manual_seed(3)
    got = run(enc, calls, ids)
    ref = copy.deepcopy(model).train()
    torch.manual_seed(3)
    assert torch.equal(got.detach(), ref(ids)[0].detach()) and not torch.equal(got.detach(), want)
    monkeypatch.setattr(enc.config, "hidden_dropout_prob", 0.0)
    assert p.refusal((ids,), {}) == "dropout is active"                          # the attention's 0.1 is still there
    monkeypatch.setattr(enc.config, "attention_probs_dropout_prob", 0.0)
    assert p.refusal((ids,), {}) == "input_ids is not a CUDA tensor"
    enc.eval()
    # the configuration: another activation, relative positions, a decoder
    for name, value in (("hidden_act", "relu"), ("position_embedding_type", "relative_key"), ("is_decoder", True)):
        with monkeypatch.context() as m:
            m.setattr(enc.config, name, value, raising=False)
            assert p.refusal((ids,), {}) == "not an absolute-position, gelu, encoder-only configuration"
    # a shape outside the kernels' set: T above 128 (the positions allow it here), head width 16
    with monkeypatch.context() as m:
        m.setattr(enc.config, "max_position_embeddings", 256)
        assert p.refusal((_ids(1, 129),), {}) == "a shape the kernels do not take"
        assert p.refusal((_ids(1, 128),), {}) == "input_ids is not a CUDA tensor"
    assert p.refusal((_ids(1, 17),), {}) == "a shape the kernels do not take"    # T > max_pos = 16
    with monkeypatch.context() as m:
        m.setattr(enc.config, "num_attention_heads", 4)
        assert p.refusal((ids,), {}) == "a shape the kernels do not take"
    assert p.hip_calls == 0


def test_other_encoders_are_not_patched(small):
    from gnnrag_amd.modules.question_encoding.lm_encoder import patch_lm_encoder
    from transformers import BertModel

    class Sub(BertModel):                       # "exactly BertModel": a subclass may override anything
        pass

    for enc in (torch.nn.LSTM(4, 4), Sub(small[0].config), None):
        h = _Holder(enc)
        fwd = None if enc is None else enc.forward
        assert patch_lm_encoder(h) is h
        assert enc is None or (enc.forward == fwd and not hasattr(enc, "_gnnrag_lm_patch"))
    assert patch_lm_encoder(object()) is not None


def test_state_dict_parameters_and_idempotence(small):
    from gnnrag_amd.modules.question_encoding.lm_encoder import patch_lm_encoder
    model = small[0]
    enc, p, _ = _patched(model)
    assert list(enc.state_dict().keys()) == list(model.state_dict().keys())
    assert [n for n, _ in enc.named_parameters()] == [n for n, _ in model.named_parameters()]
    assert [n for n, _ in enc.named_modules()] == [n for n, _ in model.named_modules()]
    h = _Holder(enc)
    patch_lm_encoder(h)
    assert enc._gnnrag_lm_patch is p and enc.forward == p.forward            # a second patch changes nothing
    enc.to(torch.float64)                                                        # .to() still reaches every parameter
    assert all(q.dtype == torch.float64 for q in enc.parameters())


def test_deep_copy_is_patched_for_itself(small):
    enc, p, _ = _patched(small[0], count=False)
    twin = copy.deepcopy(enc)
    q = twin._gnnrag_lm_patch
    assert q is not p and q.enc is twin and twin.forward.__self__ is q
    assert p.orig_forward.__self__ is enc and q.orig_forward.__self__ is twin
    with torch.no_grad():
        a, b = enc(_ids())[0], twin(_ids())[0]
    assert torch.equal(a, b)
    with torch.no_grad():
        twin.embeddings.word_embeddings.weight.add_(1.0)
        assert not torch.equal(twin(_ids())[0], a) and torch.equal(enc(_ids())[0], a)


def test_packed_weights_follow_an_in_place_update(small):
    enc, p, _ = _patched(small[0])
    s = enc.encoder.layer[0].attention.self
    W, b = p.packed_qkv()[0]
    assert W.shape == (192, 64) and b.shape == (192,)
    assert torch.equal(W, torch.cat([s.query.weight, s.key.weight, s.value.weight], 0))
    assert torch.equal(b, torch.cat([s.query.bias, s.key.bias, s.value.bias], 0))
    assert p.packed_qkv()[0][0] is W                                            # kept while nothing changes
    with torch.no_grad():
        s.key.weight.mul_(2.0)
    W2 = p.packed_qkv()[0][0]
    assert W2 is not W and torch.equal(W2[64:128], s.key.weight) and torch.equal(W2[:64], W[:64])
    with torch.no_grad():
        s.value.bias.add_(1.0)
    assert torch.equal(p.packed_qkv()[0][1][128:], s.value.bias)
    assert [sorted(d) for d in p.layers()] == [sorted(__import__("gnnrag_amd").ops.BERT_LAYER_FIELDS)]


def test_package_imports_without_transformers(monkeypatch):
    """``transformers`` hidden from sys.modules and from every finder: the package, the install module and the encoder
    module still import, and the patch leaves a module alone."""
    class Hidden:
        @staticmethod
        def find_spec(name, path=None, target=None):
            if name == "transformers" or name.startswith("transformers."):
                raise ImportError("transformers is hidden")
            return None

    for name in [n for n in sys.modules if n == "transformers" or n.startswith("transformers.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setattr(sys, "meta_path", [Hidden] + list(sys.meta_path))
    with pytest.raises(ImportError):
        importlib.import_module("transformers")
    name = "gnnrag_amd.modules.question_encoding.lm_encoder"
    monkeypatch.delitem(sys.modules, name, raising=False)
    mod = importlib.import_module(name)
    import gnnrag_amd.install as install
    importlib.import_module("gnnrag_amd.ops")

    class BertModel(torch.nn.Module):           # the name alone must not be enough either
        pass

    BertModel.__module__ = "transformers.models.bert.modeling_bert"
    h = _Holder(BertModel())
    assert mod.patch_lm_encoder(h) is h and not hasattr(h.node_encoder, "_gnnrag_lm_patch")

    class Model:
        instruction = h

    assert install.patch_lm_encoder(Model) is Model
    assert "transformers" not in sys.modules


# -- the C ABI ---------------------------------------------------------------------------------------------------------

def test_exports_and_binding(lib):
    import gnnrag_amd
    from gnnrag_amd import _lib, install, ops
    for n in ("gnnrag_bert_workspace_bytes", "gnnrag_bert_attention", "gnnrag_bert_encode"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.gnnrag_abi_version() == 16
    assert C.sizeof(_lib.BertLayer) == 12 * C.sizeof(C.c_void_p)
    for n in ("bert_attention", "bert_encode", "bert_encode_supported"):
        assert callable(getattr(ops, n))
    assert callable(install.patch_lm_encoder)
    assert ops.bert_encode_supported(20, 384, 12, 1536, 512) and ops.bert_encode_supported(128, 768, 12, 3072, 512)
    assert not ops.bert_encode_supported(129, 384, 12, 1536, 512) and not ops.bert_encode_supported(20, 384, 12, 1536, 16)
    assert not ops.bert_encode_supported(20, 384, 5, 1536, 512) and not ops.bert_encode_supported(20, 96, 2, 384, 512)
    assert not ops.bert_encode_supported(20, 66, 2, 264, 512)
    assert gnnrag_amd.ops is ops


def _encode(lib, B=2, T=9, H=384, heads=12, I=1536, L=1, vocab=64, max_pos=16, ws_bytes=None, ptr=None, layer_ptr=None,
            ids=None, ws=None):
    """gnnrag_bert_encode with stand-in pointers (nothing is launched in any of these calls)."""
    from gnnrag_amd import _lib
    layers = (_lib.BertLayer * max(L, 1))()
    for l in range(L):
        for n, _ in _lib.BertLayer._fields_:
            setattr(layers[l], n, layer_ptr)
    if ws_bytes is None:
        ws_bytes = lib.gnnrag_bert_workspace_bytes(B, T, H, I)
    return lib.gnnrag_bert_encode(ptr if ids is None else ids, ptr, vocab, ptr, max_pos, ptr, ptr, ptr, 1e-12, L, layers,
                                  B, T, H, heads, I, ptr, ptr if ws is None else ws, ws_bytes, 0, None)


def test_unsupported_rules_with_null_pointers(lib):
    """Every shape rule is answered before a pointer is looked at: with NULL everywhere the answer is still
    GNNRAG_E_UNSUPPORTED, and the same call with a legal shape is GNNRAG_E_BADARG (the pointers' turn)."""
    assert _encode(lib) == E_BADARG
    assert _encode(lib, H=380, heads=12) == E_UNSUPPORTED            # H % heads != 0
    assert _encode(lib, H=192, heads=12) == E_UNSUPPORTED            # dh = 16
    assert _encode(lib, H=1536, heads=12) == E_UNSUPPORTED           # dh = 128
    assert _encode(lib, H=384, heads=6) == E_BADARG                  # dh = 64 is taken
    assert _encode(lib, T=129, max_pos=512) == E_UNSUPPORTED         # T > 128
    assert _encode(lib, T=128, max_pos=512) == E_BADARG
    assert _encode(lib, T=17, max_pos=16) == E_UNSUPPORTED           # T > max_pos
    assert _encode(lib, T=16, max_pos=16) == E_BADARG
    assert _encode(lib, H=66, heads=2) == E_UNSUPPORTED              # H % 4 != 0 (dh = 33)
    need = lib.gnnrag_bert_workspace_bytes(2, 9, 384, 1536)
    assert _encode(lib, ws_bytes=need - 1) == E_UNSUPPORTED          # a workspace that is too small
    assert _encode(lib, ws_bytes=0) == E_UNSUPPORTED
    assert _encode(lib, L=0, ws_bytes=0) == E_BADARG                 # L = 0 needs none
    # misaligned pointers (stand-in addresses; nothing is dereferenced on the device before the answer)
    ok, odd = 0x10000, 0x10004
    assert _encode(lib, L=0, ptr=odd) == E_UNSUPPORTED
    assert _encode(lib, L=1, ptr=ok, layer_ptr=odd) == E_UNSUPPORTED
    assert _encode(lib, L=1, ptr=ok, layer_ptr=ok, ws=odd) == E_UNSUPPORTED
    assert _encode(lib, L=1, ptr=ok, layer_ptr=None) == E_BADARG
    # the attention entry point alone
    att = lib.gnnrag_bert_attention
    assert att(None, 1, 9, 2, 32, None, None) == E_BADARG
    assert att(None, 1, 9, 2, 16, None, None) == E_UNSUPPORTED
    assert att(None, 1, 9, 2, 48, None, None) == E_UNSUPPORTED
    assert att(None, 1, 129, 2, 64, None, None) == E_UNSUPPORTED
    assert att(odd, 1, 9, 2, 64, ok, None) == E_UNSUPPORTED and att(ok, 1, 9, 2, 64, odd, None) == E_UNSUPPORTED
    assert att(None, 0, 9, 2, 32, None, None) == E_BADARG


def test_workspace_bytes_is_monotone(lib):
    f = lib.gnnrag_bert_workspace_bytes
    base = (3, 9, 384, 1536)
    assert f(*base) >= 4 * 27 * (5 * 384 + 1536)
    for i in range(4):
        prev = f(*base)
        for step in (1, 2, 7, 64):
            a = list(base)
            a[i] += step
            cur = f(*a)
            assert cur >= prev
            prev = cur
        bigger = list(base)
        bigger[i] *= 2
        assert f(*bigger) > f(*base)
        zero = list(base)
        zero[i] = 0
        assert f(*zero) == 0
