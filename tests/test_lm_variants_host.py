"""Host side of the RoBERTa / MPNet question encoders (CPU, no GPU): the position rule and the bias table against
transformers' own functions, the rules of ``patch_lm_encoder`` for the two classes and the switch per class, the argument
rules of ``gnnrag_bert_encode_ex`` / ``gnnrag_bert_attention_bias`` (answered before a device is touched), and the float64
oracle against the live reference's fixture."""
import copy
import os

import numpy as np
import pytest
import torch

import bert_oracle as bo
import lm_variants_oracle as lo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "lm_variants_ref.npz")
E_UNSUPPORTED, E_BADARG = -2, -1
PAD = lo.PAD
NOT_CUDA = "input_ids is not a CUDA tensor"        # the rule that refuses last on a host without a GPU


@pytest.fixture(scope="module")
def lib():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def small():
    """arch -> (fp32 model, float64 copy): H = 64, 2 heads of 32, one layer, 16 positions."""
    pytest.importorskip("transformers")
    return {arch: lo.make_model(arch, lo.config(arch, L=1, max_pos=16, **lo.SMALL[32]), seed=5 + i)
            for i, arch in enumerate(("bert",) + lo.ARCHS)}


class _Holder:
    def __init__(self, enc):
        self.node_encoder = enc


def _patched(model):
    """A private, frozen copy of ``model``, patched, its original forward counted."""
    from gnnrag_amd.modules.question_encoding.lm_encoder import patch_lm_encoder
    enc = copy.deepcopy(model)
    for q in enc.parameters():
        q.requires_grad_(False)
    h = _Holder(enc)
    assert patch_lm_encoder(h) is h
    p = enc._gnnrag_lm_patch
    calls, orig = [], p.orig_forward

    def counted(*a, **k):
        calls.append((a, k))
        return orig(*a, **k)

    p.orig_forward = counted
    return enc, p, calls


# -- positions and the bias table ---------------------------------------------------------------------------------------

def test_position_rule_equals_transformers():
    """The plain-Python rule (what k_bert_embed_ln counts: pad -> pad, the n-th non-pad token -> pad + n) against
    ``create_position_ids_from_input_ids`` of both classes."""
    pytest.importorskip("transformers")
    from transformers.models.mpnet.modeling_mpnet import create_position_ids_from_input_ids as mpnet_rule
    from transformers.models.roberta.modeling_roberta import RobertaEmbeddings
    for T in (1, 2, 9, 65, 128):
        for pad in (1, 0, 3):
            rows = lo.pad_rows(T, pad=pad, vocab=lo.VOCAB + pad)
            want = lo.positions(rows, pad)
            ids = torch.from_numpy(rows)
            assert np.array_equal(RobertaEmbeddings.create_position_ids_from_input_ids(ids, pad).numpy(), want)
            assert np.array_equal(mpnet_rule(ids, pad).numpy(), want)
    rows = lo.pad_rows(9)
    want = lo.positions(rows, PAD)
    assert want[0].tolist() == list(range(2, 11))                                   # no pad: pad + 1 .. pad + T
    assert want[1].tolist() == [2, 3, 4, 5, 6, 1, 1, 1, 1]                          # trailing pads
    assert want[2].tolist() == [2, 3, 4, 5, 1, 6, 7, 8, 9]                          # a pad in the middle
    assert want[3].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9]                          # a pad first
    assert want[4].tolist() == [2] + [1] * 8                                        # pads only after the first token
    assert lo.positions([[7]], PAD).tolist() == [[2]] and lo.positions([[PAD]], PAD).tolist() == [[PAD]]


@pytest.mark.parametrize("T", [1, 2, 9, 64, 65, 128])
def test_bias_table_equals_compute_position_bias(small, T):
    """Every (i, j): table[h, j - i + T - 1] is the entry of transformers' ``compute_position_bias`` (distances 8, 11,
    16, 32, 64 and 127 are where buckets change or the clamp engages; T = 128 holds them all)."""
    from gnnrag_amd.modules.question_encoding.lm_encoder import rel_bias_table
    model = small["mpnet"][0]
    table = rel_bias_table(model.encoder, T)
    heads = model.config.num_attention_heads
    assert table.shape == (heads, 2 * T - 1) and table.is_contiguous() and table.dtype == torch.float32
    with torch.no_grad():
        want = model.encoder.compute_position_bias(torch.zeros(2, T, 1))
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    assert torch.equal(table[:, j - i + T - 1], want[0]) and torch.equal(want[0], want[1])
    assert torch.equal(table, lo.bias_table(model, T))                              # the tests' own reading of it
    if T == 128:
        # not symmetric: keys behind the query (j > i) use the buckets 16 .. 31, keys in front of it 0 .. 15
        assert not torch.equal(table, torch.flip(table, dims=(1,)))
        w = model.encoder.relative_attention_bias.weight.detach()
        assert torch.equal(table[:, T - 1 + 127], w[31]) and torch.equal(table[:, T - 1 - 127], w[15])
        assert torch.equal(table[:, T - 1 + 7], w[16 + 7]) and torch.equal(table[:, T - 1 - 8], w[8])


def test_bias_table_is_kept_until_the_weight_changes(small):
    enc, p, _ = _patched(small["mpnet"][0])
    a = p.rel_bias(9)
    assert p.rel_bias(9) is a and p.rel_bias(5).shape == (2, 9) and p.rel_bias(9) is a
    with torch.no_grad():
        enc.encoder.relative_attention_bias.weight.mul_(2.0)
    b = p.rel_bias(9)
    assert b is not a and torch.equal(b, 2.0 * a)
    assert _patched(small["roberta"][0])[1].rel_bias(9) is None


# -- the patch ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arch", lo.ARCHS)
def test_the_two_classes_are_patched_and_read_by_name(small, arch):
    model = small[arch][0]
    enc, p, _ = _patched(model)
    assert enc.forward == p.forward and p.pad_id() == PAD
    assert list(enc.state_dict().keys()) == list(model.state_dict().keys())
    L = p.layers()
    from gnnrag_amd import ops
    assert [sorted(d) for d in L] == [sorted(ops.BERT_LAYER_FIELDS)]
    want = lo.layer_params(enc, 9)["layers"][0]
    for k in ops.BERT_LAYER_FIELDS:
        assert torch.equal(L[0][k], want[k]), k
    twin = copy.deepcopy(enc)
    assert twin._gnnrag_lm_patch is not p and twin._gnnrag_lm_patch.enc is twin


def test_subclasses_and_t5_are_not_patched(small):
    from gnnrag_amd.modules.question_encoding.lm_encoder import patch_lm_encoder
    from transformers import MPNetModel, RobertaModel, T5Config, T5EncoderModel, T5Model

    class SubR(RobertaModel):
        pass

    class SubM(MPNetModel):
        pass

    t5 = T5Config(vocab_size=50, d_model=64, d_kv=32, d_ff=128, num_layers=1, num_heads=2)
    for enc in (SubR(small["roberta"][0].config), SubM(small["mpnet"][0].config), T5Model(t5), T5EncoderModel(t5),
                T5Model(t5).encoder):
        h = _Holder(enc)
        fwd = enc.forward
        assert patch_lm_encoder(h) is h
        assert enc.forward == fwd and not hasattr(enc, "_gnnrag_lm_patch")


def test_switch_per_class(small, monkeypatch):
    """Unset: on for the classes of ``DEFAULT_ON`` only; ``0``: off for every class; ``1``: on for every class.  Read at
    every call.  Nothing changes for ``BertModel``."""
    from gnnrag_amd.modules.question_encoding import lm_encoder
    assert "BertModel" in lm_encoder.DEFAULT_ON
    ids = torch.from_numpy(lo.ids_with_pads(2, 5))
    for arch in ("bert",) + lo.ARCHS:
        model = small[arch][0]
        enc, p, calls = _patched(model)
        with torch.no_grad():
            want = model(ids)[0]
        default_on = type(model).__name__ in lm_encoder.DEFAULT_ON
        assert (arch != "bert") or default_on
        monkeypatch.delenv("GNNRAG_HIP_LM", raising=False)
        assert p.refusal((ids,), {}) == (NOT_CUDA if default_on else "GNNRAG_HIP_LM is off")
        assert lm_encoder.enabled(type(model).__name__) == default_on
        monkeypatch.setenv("GNNRAG_HIP_LM", "0")
        assert p.refusal((ids,), {}) == "GNNRAG_HIP_LM is off" and not lm_encoder.enabled(type(model).__name__)
        monkeypatch.setenv("GNNRAG_HIP_LM", "1")
        assert p.refusal((ids,), {}) == NOT_CUDA and lm_encoder.enabled(type(model).__name__)
        with torch.no_grad():                       # a refused call is the unpatched forward, bit for bit, run once
            assert torch.equal(enc(ids)[0], want) and len(calls) == 1
        monkeypatch.delenv("GNNRAG_HIP_LM", raising=False)
    assert lm_encoder.enabled() and lm_encoder.enabled("BertModel")


@pytest.mark.parametrize("arch", lo.ARCHS)
def test_refusals(small, arch, monkeypatch):
    model = small[arch][0]
    enc, p, calls = _patched(model)
    ids = torch.from_numpy(lo.ids_with_pads(2, 5))
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    assert p.refusal((ids,), {}) == NOT_CUDA and p.refusal((), {"input_ids": ids}) == NOT_CUDA
    # the reference's call and the same call with a mask of ones are one result: pads are attended
    with torch.no_grad():
        assert torch.equal(model(ids)[0], model(ids, attention_mask=torch.ones_like(ids))[0])
    assert p.refusal((ids,), {"attention_mask": torch.ones_like(ids)}) == "arguments other than input_ids"
    assert p.refusal((ids,), {"position_ids": torch.ones_like(ids)}) == "arguments other than input_ids"
    assert p.refusal((ids.int(),), {}) == "input_ids is not a 2-D int64 tensor"
    # positions from the ids: max_pos = 16, pad = 1 takes T = 14 (a full row reaches position 15) and not T = 15
    assert p.refusal((torch.from_numpy(lo.ids_with_pads(1, 14)),), {}) == NOT_CUDA
    assert p.refusal((torch.from_numpy(lo.ids_with_pads(1, 15)),), {}) == "a shape the kernels do not take"
    with pytest.raises((IndexError, RuntimeError)):     # transformers itself raises there (a full row)
        model(torch.from_numpy(lo.ids_with_pads(1, 15)))
    # training mode with the configuration's dropout 0.1 falls through; a needed gradient too
    assert float(enc.config.hidden_dropout_prob) == 0.1
    enc.train()
    assert p.refusal((ids,), {}) == "dropout is active"
    torch.manual_seed(3)
    got = enc(ids)[0]
    ref = copy.deepcopy(model).train()
    torch.manual_seed(3)
    assert len(calls) == 1 and torch.equal(got.detach(), ref(ids)[0].detach())
    enc.eval()
    next(enc.parameters()).requires_grad_(True)
    assert p.refusal((ids,), {}) == "a gradient is needed"
    with torch.no_grad():
        assert p.refusal((ids,), {}) == NOT_CUDA
    next(enc.parameters()).requires_grad_(False)
    # the configuration
    with monkeypatch.context() as m:
        m.setattr(enc.config, "hidden_act", "relu")
        assert p.refusal((ids,), {}) == "not an absolute-position, gelu, encoder-only configuration"
    with monkeypatch.context() as m:
        m.setattr(enc.embeddings, "padding_idx", None)
        assert p.refusal((ids,), {}) == "no padding_idx to count positions from"
    with monkeypatch.context() as m:
        m.setattr(enc.config, "num_attention_heads", 4)
        assert p.refusal((ids,), {}) == "a shape the kernels do not take"
    assert p.hip_calls == 0


def test_sixteen_buckets_are_refused(small, monkeypatch):
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    cfg = lo.config("mpnet", L=1, max_pos=16, relative_attention_num_buckets=16, **lo.SMALL[32])
    model, _ = lo.make_model("mpnet", cfg, seed=9)
    _, p, _ = _patched(model)
    ids = torch.from_numpy(lo.ids_with_pads(2, 5))
    assert p.refusal((ids,), {}) == "a relative attention bias of other than 32 buckets"
    _, q, _ = _patched(small["mpnet"][0])
    assert q.refusal((ids,), {}) == NOT_CUDA


def test_roberta_without_a_pad_token_is_refused(monkeypatch):
    pytest.importorskip("transformers")
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    cfg = lo.config("roberta", L=1, max_pos=16, pad=None, **lo.SMALL[32])
    model, _ = lo.make_model("roberta", cfg, seed=3)
    _, p, _ = _patched(model)
    assert p.refusal((torch.from_numpy(lo.ids_with_pads(2, 5)),), {}) == "no padding_idx to count positions from"


# -- the C ABI ---------------------------------------------------------------------------------------------------------

def test_exports_and_binding(lib):
    import inspect
    from gnnrag_amd import _lib, ops
    for n in ("gnnrag_bert_encode_ex", "gnnrag_bert_attention_bias", "gnnrag_bert_encode", "gnnrag_bert_attention"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.gnnrag_abi_version() == 16
    sig = inspect.signature(ops.bert_encode).parameters
    assert sig["pad_id"].default is None and sig["rel_bias"].default is None
    assert inspect.signature(ops.bert_attention).parameters["rel_bias"].default is None
    assert inspect.signature(ops.bert_encode_supported).parameters["pad_id"].default is None
    assert ops.bert_encode_supported(10, 64, 2, 128, 12, pad_id=1) and not ops.bert_encode_supported(11, 64, 2, 128, 12, pad_id=1)
    assert ops.bert_encode_supported(11, 64, 2, 128, 12) and ops.bert_encode_supported(12, 64, 2, 128, 12)
    assert ops.bert_encode_supported(11, 64, 2, 128, 12, pad_id=0) and not ops.bert_encode_supported(12, 64, 2, 128, 12, pad_id=0)
    assert ops.bert_encode_supported(126, 768, 12, 3072, 514, pad_id=1) and ops.bert_encode_supported(128, 768, 12, 3072, 514, pad_id=1)


def _encode_ex(lib, B=2, T=9, H=64, heads=2, I=128, L=1, vocab=50, max_pos=16, pad=1, ptr=None, type_emb="ptr",
               rel_bias=None, layer_ptr=None, old=False):
    """gnnrag_bert_encode_ex with stand-in pointers (nothing is launched in any of these calls)."""
    from gnnrag_amd import _lib
    layers = (_lib.BertLayer * max(L, 1))()
    for l in range(L):
        for n, _ in _lib.BertLayer._fields_:
            setattr(layers[l], n, layer_ptr)
    ws_bytes = lib.gnnrag_bert_workspace_bytes(B, T, H, I)
    ty = ptr if type_emb == "ptr" else type_emb
    if old:
        return lib.gnnrag_bert_encode(ptr, ptr, vocab, ptr, max_pos, ty, ptr, ptr, 1e-5, L, layers, B, T, H, heads, I, ptr,
                                      ptr, ws_bytes, 0, None)
    return lib.gnnrag_bert_encode_ex(ptr, ptr, vocab, ptr, max_pos, ty, pad, rel_bias, ptr, ptr, 1e-5, L, layers, B, T, H,
                                     heads, I, ptr, ptr, ws_bytes, 0, None)


def test_new_argument_rules_without_a_device(lib):
    """The shape rules are answered before a pointer is looked at (NULL everywhere: UNSUPPORTED for a refused shape,
    BADARG - the pointers' turn - for a legal one); the pointer rules with stand-in addresses, NULL layers stop the call."""
    # T + pad > max_pos - 1
    assert _encode_ex(lib, T=11, pad=1, max_pos=12) == E_UNSUPPORTED
    assert _encode_ex(lib, T=10, pad=1, max_pos=12) == E_BADARG
    assert _encode_ex(lib, T=11, pad=0, max_pos=12) == E_BADARG and _encode_ex(lib, T=12, pad=0, max_pos=12) == E_UNSUPPORTED
    assert _encode_ex(lib, T=12, pad=-1, max_pos=12) == E_BADARG                 # absolute positions: T <= max_pos as before
    assert _encode_ex(lib, T=13, pad=-1, max_pos=12) == E_UNSUPPORTED
    assert _encode_ex(lib, T=12, max_pos=12, old=True) == E_BADARG
    assert _encode_ex(lib, T=128, pad=1, max_pos=130) == E_BADARG and _encode_ex(lib, T=128, pad=1, max_pos=129) == E_UNSUPPORTED
    assert _encode_ex(lib, T=129, pad=1, max_pos=514) == E_UNSUPPORTED
    assert _encode_ex(lib, T=9, pad=2**31 - 1, max_pos=2**31 - 1) == E_UNSUPPORTED      # no overflow in T + pad
    # pointers: a NULL type_emb is accepted by the new entry point (the call gets as far as the NULL layers), not by the old
    ok, odd = 0x10000, 0x10004
    assert _encode_ex(lib, ptr=ok, type_emb=None, layer_ptr=None) == E_BADARG
    assert _encode_ex(lib, ptr=ok, type_emb=None, layer_ptr=odd) == E_UNSUPPORTED        # ... and on to the layers' alignment
    assert _encode_ex(lib, ptr=ok, type_emb=None, layer_ptr=odd, old=True) == E_BADARG
    assert _encode_ex(lib, ptr=ok, type_emb=odd, layer_ptr=None) == E_UNSUPPORTED
    # a misaligned rel_bias
    assert _encode_ex(lib, ptr=ok, rel_bias=odd, layer_ptr=None) == E_UNSUPPORTED
    assert _encode_ex(lib, ptr=ok, rel_bias=ok, layer_ptr=None) == E_BADARG
    assert _encode_ex(lib, ptr=ok, rel_bias=ok, layer_ptr=odd) == E_UNSUPPORTED
    att = lib.gnnrag_bert_attention_bias
    assert att(None, 1, 9, 2, 32, None, None, None) == E_BADARG
    assert att(None, 1, 9, 2, 16, ok, None, None) == E_UNSUPPORTED and att(None, 1, 129, 2, 64, ok, None, None) == E_UNSUPPORTED
    assert att(ok, 1, 9, 2, 64, odd, ok, None) == E_UNSUPPORTED
    assert att(odd, 1, 9, 2, 64, ok, ok, None) == E_UNSUPPORTED and att(ok, 1, 9, 2, 64, ok, odd, None) == E_UNSUPPORTED
    assert att(None, 1, 9, 2, 64, ok, None, None) == E_BADARG and att(None, 0, 9, 2, 32, ok, None, None) == E_BADARG


def test_ops_refuse_a_negative_pad_id():
    from gnnrag_amd import ops
    with pytest.raises(ValueError):
        ops._bert_pad_id(-1)
    assert ops._bert_pad_id(None) == -1 and ops._bert_pad_id(1) == 1


# -- the oracle and the fixture ---------------------------------------------------------------------------------------

def test_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(GOLDEN) < 512 * 1024
    g = np.load(GOLDEN, allow_pickle=False)
    assert not any(".param.node_encoder" in k for k in g.files)
    for tag in ("roberta", "sbert2"):
        q, pad = g[tag + ".q_input"], int(g[tag + ".cfg.pad_val"])
        assert pad == 1 and q.shape == (3, 9) and (q[0] != pad).all() and (q[1, :5] != pad).all() and (q[1, 5:] == pad).all()
        assert q[2, 0] != pad and (q[2, 1:] == pad).all()


@pytest.mark.parametrize("tag,arch", [("roberta", "roberta"), ("sbert2", "mpnet")])
def test_oracle_reproduces_the_reference_lm_states(tag, arch):
    """The float64 module built from the fixture's seed against the LM states of the live reference's fp32 run: their
    distance is the reference's own fp32 error, recorded against ITS float64 run (same weights), so well inside the
    bound."""
    pytest.importorskip("transformers")
    g = np.load(GOLDEN)
    c = lambda k: int(g["%s.cfg.%s" % (tag, k)])    # noqa: E731
    cfg = lo.config(arch, H=c("H"), heads=c("heads"), I=c("I"), L=c("L"), vocab=c("vocab"), max_pos=c("max_pos"),
                    pad=c("pad_val"))
    _, m64 = lo.make_model(arch, cfg, c("seed"))
    err, e_ref = bo.rel_err(g[tag + ".lm.states"], lo.states(m64, g[tag + ".q_input"])), float(g[tag + ".lm.e_ref"])
    print("%s: oracle vs fixture %.3g, recorded e_ref %.3g, bound %.3g" % (tag, err, e_ref, bo.bound(e_ref)))
    assert 0.0 < e_ref < 1e-5
    assert err <= bo.bound(e_ref)
