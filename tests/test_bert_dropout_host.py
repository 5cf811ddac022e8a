"""Host side of the training-mode question encoder (CPU, no GPU): the exports and argument rules of
``gnnrag_bert_encode_train`` / ``gnnrag_bert_attention_drop`` (answered before a device is touched), the mask-injecting
oracle of tests/bert_dropout_oracle.py against the plain one, the switch ``GNNRAG_HIP_LM_TRAIN`` and ``draw_keep``."""
import copy
import math

import numpy as np
import pytest
import torch

import bert_dropout_oracle as do
import bert_oracle as bo
import lm_variants_oracle as lo

E_UNSUPPORTED, E_BADARG = -2, -1
OK, ODD = 0x10000, 0x10004                      # stand-in addresses: 16-byte aligned / 4-byte aligned only


@pytest.fixture(scope="module")
def lib():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    return _lib.load()


# -- the C ABI ---------------------------------------------------------------------------------------------------------

def test_exports_and_binding(lib):
    from gnnrag_amd import _lib, ops
    for n in ("gnnrag_bert_keep_hidden_bytes", "gnnrag_bert_keep_att_bytes", "gnnrag_bert_attention_drop",
              "gnnrag_bert_encode_train"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.gnnrag_abi_version() == 16 and _lib.ABI_VERSION == 16
    for n in ("bert_attention_drop", "bert_encode_train", "bert_keep_shapes", "bert_encode", "bert_attention"):
        assert callable(getattr(ops, n))
    assert ops.bert_keep_shapes(2, 3, 9, 384, 12) == ((5, 27, 384), (2, 3, 12, 9, 9))


def test_keep_sizes(lib):
    from gnnrag_amd import ops
    fh, fa = lib.gnnrag_bert_keep_hidden_bytes, lib.gnnrag_bert_keep_att_bytes
    for L, B, T, H, heads in ((1, 1, 1, 32, 1), (2, 3, 9, 384, 12), (6, 64, 20, 384, 12), (12, 64, 128, 768, 12)):
        assert fh(L, B, T, H) == (1 + 2 * L) * B * T * H
        assert fa(L, B, T, heads) == L * B * heads * T * T
        sh, sa = ops.bert_keep_shapes(L, B, T, H, heads)
        assert math.prod(sh) == fh(L, B, T, H) and math.prod(sa) == fa(L, B, T, heads)
    assert fh(0, 3, 9, 384) == 3 * 9 * 384 and fa(0, 3, 9, 12) == 0      # L = 0: plane 0 alone, no attention
    base = (2, 3, 9, 12)
    for i in range(4):
        for bad in (0, -1):
            a = list(base)
            a[i] = bad
            assert fa(*a) == 0
            if not (i == 0 and bad == 0):
                assert fh(*a) == 0


def _train(lib, B=2, T=9, H=384, heads=12, I=1536, L=1, vocab=64, max_pos=16, ws_bytes=None, ptr=None, layer_ptr=None,
           ws=None, pad_id=-1, keep_hidden=None, scale_hidden=1.0, keep_att=None, scale_att=1.0):
    """gnnrag_bert_encode_train with stand-in pointers (nothing is launched in any of these calls)."""
    from gnnrag_amd import _lib
    layers = (_lib.BertLayer * max(L, 1))()
    for l in range(L):
        for n, _ in _lib.BertLayer._fields_:
            setattr(layers[l], n, layer_ptr)
    if ws_bytes is None:
        ws_bytes = lib.gnnrag_bert_workspace_bytes(B, T, H, I)
    return lib.gnnrag_bert_encode_train(ptr, ptr, vocab, ptr, max_pos, ptr, pad_id, None, ptr, ptr, 1e-12, L, layers, B, T, H,
                                        heads, I, keep_hidden, scale_hidden, keep_att, scale_att, ptr,
                                        ptr if ws is None else ws, ws_bytes, 0, None)


@pytest.mark.parametrize("masks", [{}, dict(keep_hidden=OK, scale_hidden=1.25, keep_att=OK + 1, scale_att=2.0)],
                         ids=["no-masks", "masks"])
def test_shape_rules_are_those_of_the_inference_entry(lib, masks):
    """Every case of tests/test_bert_host.py::test_unsupported_rules_with_null_pointers, answered the same way - with and
    without masks (the shape rules come first, whatever the pointers are)."""
    t = lambda **k: _train(lib, **k, **masks)   # noqa: E731
    assert t() == E_BADARG
    assert t(H=380, heads=12) == E_UNSUPPORTED
    assert t(H=192, heads=12) == E_UNSUPPORTED
    assert t(H=1536, heads=12) == E_UNSUPPORTED
    assert t(H=384, heads=6) == E_BADARG
    assert t(T=129, max_pos=512) == E_UNSUPPORTED
    assert t(T=128, max_pos=512) == E_BADARG
    assert t(T=17, max_pos=16) == E_UNSUPPORTED
    assert t(T=16, max_pos=16) == E_BADARG
    assert t(H=66, heads=2) == E_UNSUPPORTED
    need = lib.gnnrag_bert_workspace_bytes(2, 9, 384, 1536)
    assert t(ws_bytes=need - 1) == E_UNSUPPORTED
    assert t(ws_bytes=0) == E_UNSUPPORTED
    assert t(L=0, ws_bytes=0) == E_BADARG
    assert t(L=0, ptr=ODD) == E_UNSUPPORTED
    assert t(L=1, ptr=OK, layer_ptr=ODD) == E_UNSUPPORTED
    assert t(L=1, ptr=OK, layer_ptr=OK, ws=ODD) == E_UNSUPPORTED
    assert t(L=1, ptr=OK, layer_ptr=None) == E_BADARG
    assert t(T=15, max_pos=16, pad_id=1) == E_UNSUPPORTED           # positions from the ids: T + pad_id > max_pos - 1
    assert t(T=14, max_pos=16, pad_id=1) == E_BADARG
    assert t(B=0) == E_BADARG and t(L=-1) == E_BADARG


def test_scale_and_alignment_rules(lib):
    """A scale is judged only when its mask is given, with the NULL-pointer rules (BADARG, before the alignment rules:
    every other pointer here is misaligned, so a scale that passes is answered UNSUPPORTED)."""
    bad = (float("nan"), float("inf"), -float("inf"), 0.0, -1.0)
    assert _train(lib, L=0, ptr=ODD, keep_hidden=OK, scale_hidden=1.25, keep_att=OK, scale_att=2.0) == E_UNSUPPORTED
    for s in bad:
        assert _train(lib, L=0, ptr=ODD, keep_hidden=OK, scale_hidden=s) == E_BADARG
        assert _train(lib, L=0, ptr=ODD, keep_att=OK, scale_att=s) == E_BADARG
        assert _train(lib, L=0, ptr=ODD, scale_hidden=s, scale_att=s) == E_UNSUPPORTED      # no mask: not read
        assert _train(lib, H=380, keep_hidden=OK, scale_hidden=s) == E_UNSUPPORTED          # the shape rules are first
    # keep_hidden: 4-byte aligned (the layer pointers are NULL: a call that passes the alignment rules ends BADARG there)
    assert _train(lib, ptr=OK, layer_ptr=None, keep_hidden=ODD) == E_BADARG
    for off in (1, 2, 3):
        assert _train(lib, ptr=OK, layer_ptr=None, keep_hidden=OK + off) == E_UNSUPPORTED
    # keep_att: any alignment
    for off in (0, 1, 2, 3):
        assert _train(lib, ptr=OK, layer_ptr=None, keep_att=OK + off) == E_BADARG


def test_attention_drop_rules(lib):
    att = lib.gnnrag_bert_attention_drop
    assert att(None, 1, 9, 2, 32, None, None, 1.0, None, None) == E_BADARG
    assert att(None, 1, 9, 2, 16, None, OK, 1.0, None, None) == E_UNSUPPORTED
    assert att(None, 1, 9, 2, 48, None, OK, 1.0, None, None) == E_UNSUPPORTED
    assert att(None, 1, 129, 2, 64, None, OK, 1.0, None, None) == E_UNSUPPORTED
    assert att(None, 0, 9, 2, 32, None, OK, 1.0, None, None) == E_BADARG
    assert att(ODD, 1, 9, 2, 64, None, OK + 1, 1.0, OK, None) == E_UNSUPPORTED        # qkv misaligned, keep at any address
    assert att(OK, 1, 9, 2, 64, None, OK + 1, 1.0, ODD, None) == E_UNSUPPORTED
    assert att(OK, 1, 9, 2, 64, ODD, OK + 1, 1.0, OK, None) == E_UNSUPPORTED          # rel_bias misaligned
    for s in (float("nan"), float("inf"), 0.0, -2.0):
        assert att(ODD, 1, 9, 2, 64, None, OK, s, OK, None) == E_BADARG               # before the alignment rules
        assert att(ODD, 1, 9, 2, 64, None, None, s, OK, None) == E_UNSUPPORTED        # no mask: the scale is not read
        assert att(ODD, 1, 9, 2, 16, None, OK, s, OK, None) == E_UNSUPPORTED          # the shape rules are first


# -- the oracle --------------------------------------------------------------------------------------------------------

def _variant(arch, L=2):
    if arch == "bert":
        return do.make_bert(dict(H=64, heads=2, I=128), L, seed=5, vocab=50), np.random.RandomState(1).randint(0, 50, (3, 9))
    return do.make_variant(arch, lo.SMALL[32], L, seed=5), lo.ids_with_pads(3, 9)


@pytest.mark.parametrize("arch", ["bert", "roberta", "mpnet"])
def test_oracle_call_order_and_all_ones(arch):
    """transformers calls F.dropout in the order of ``call_order``; with all-ones masks and scale 1 the injected run is
    the eval-mode run of the default attention implementation (float64: 1e-12 of the largest entry); and the fp32
    module with the same masks is a small e_ref away from the float64 one."""
    pytest.importorskip("transformers")
    (m32, m64), ids = _variant(arch)
    L, B, T, H, heads = 2, 3, 9, 64, 2
    seen = []
    got = do.run(m64, ids, do.ones(L, B, T, H, heads), record=seen)
    assert seen == do.call_order(L, B, T, H, heads)
    assert not m64.training
    if arch == "bert":
        plain = bo.make_model(bo.config(H=64, heads=2, I=128, L=L, vocab=50), seed=5)[1]
    else:
        plain = lo.make_model(arch, lo.config(arch, L=L, **lo.SMALL[32]), seed=5)[1]
    err = bo.rel_err(got, bo.states(plain, ids))
    print("%s: eager all-ones vs default attention %.3g" % (arch, err))
    assert err <= 1e-12
    masks = do.draw(7, L, B, T, H, heads, 0.1, 0.1)
    want = do.run(m64, ids, masks, do.scale(0.1), do.scale(0.1))
    e_ref = bo.rel_err(do.run(m32, ids, masks, do.scale(0.1), do.scale(0.1)), want)
    print("%s: e_ref with injected masks %.3g" % (arch, e_ref))
    assert 0.0 < e_ref < 1e-5
    assert bo.rel_err(want, got) > 1e-3                             # the masks do something
    with pytest.raises(AssertionError):
        do.run(m64, ids, masks + [masks[0]])                        # a mask too many is noticed
    kh, ka = do.pack(masks, L)
    assert kh.shape == (5, 27, 64) and ka.shape == (2, 3, 2, 9, 9) and kh.dtype == np.uint8
    assert np.array_equal(kh[3].reshape(3, 9, 64), masks[5]) and np.array_equal(ka[1], masks[4])
    assert do.pack(do.draw(7, L, B, T, H, heads, None, 0.1), L)[0] is None


# -- the module --------------------------------------------------------------------------------------------------------

class _Holder:
    def __init__(self, enc):
        self.node_encoder = enc


def test_switch_and_module_rules(monkeypatch):
    pytest.importorskip("transformers")
    from gnnrag_amd.modules.question_encoding import lm_encoder as le
    model = bo.make_model(bo.config(H=64, heads=2, I=128, L=1, vocab=50, max_pos=16), seed=5)[0]
    enc = copy.deepcopy(model)
    for q in enc.parameters():
        q.requires_grad_(False)
    le.patch_lm_encoder(_Holder(enc))
    p = enc._gnnrag_lm_patch
    ids = torch.from_numpy(np.random.RandomState(0).randint(0, 50, (2, 5))).long()
    enc.train()
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    monkeypatch.delenv("GNNRAG_HIP_LM_TRAIN", raising=False)
    assert not le.train_enabled() and p.refusal((ids,), {}) == "dropout is active"          # unset: off
    monkeypatch.setenv("GNNRAG_HIP_LM_TRAIN", "0")
    assert p.refusal((ids,), {}) == "dropout is active"
    monkeypatch.setenv("GNNRAG_HIP_LM_TRAIN", "1")                                          # read at every call
    assert le.train_enabled() and p.refusal((ids,), {}) == "input_ids is not a CUDA tensor"
    for name in ("hidden_dropout_prob", "attention_probs_dropout_prob"):
        with monkeypatch.context() as m:
            m.setattr(enc.config, name, 1.0)
            assert p.refusal((ids,), {}) == "a dropout probability of 1"
    monkeypatch.setenv("GNNRAG_HIP_LM", "0")                                                # the class's own switch rules
    assert p.refusal((ids,), {}) == "GNNRAG_HIP_LM is off"
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    next(enc.parameters()).requires_grad_(True)                                             # every other rule is unchanged
    assert p.refusal((ids,), {}) == "a gradient is needed"
    next(enc.parameters()).requires_grad_(False)
    assert p.refusal((ids,), {"attention_mask": torch.ones_like(ids)}) == "arguments other than input_ids"
    # a refused training-mode call is transformers' own forward with its own draws
    torch.manual_seed(3)
    got = enc(ids)[0]
    ref = copy.deepcopy(model).train()
    torch.manual_seed(3)
    assert torch.equal(got.detach(), ref(ids)[0].detach())
    assert p.hip_calls == 0 and p.hip_train_calls == 0


def test_draw_keep():
    from gnnrag_amd import ops
    from gnnrag_amd.modules.question_encoding.lm_encoder import draw_keep
    L, B, T, H, heads = 3, 3, 9, 384, 12
    p_h, p_a = 0.1, 0.3
    torch.manual_seed(11)
    kh, ka = draw_keep(L, B, T, H, heads, p_h, p_a, "cpu")
    sh, sa = ops.bert_keep_shapes(L, B, T, H, heads)
    assert tuple(kh.shape) == sh and tuple(ka.shape) == sa and kh.dtype == ka.dtype == torch.uint8
    assert kh.is_contiguous() and ka.is_contiguous() and kh.data_ptr() % 4 == 0
    assert set(kh.unique().tolist()) <= {0, 1} and set(ka.unique().tolist()) <= {0, 1}
    torch.manual_seed(11)
    kh2, ka2 = draw_keep(L, B, T, H, heads, p_h, p_a, "cpu")
    assert torch.equal(kh, kh2) and torch.equal(ka, ka2)
    # the share of ones: a binomial mean, 5 standard deviations (1 in 1.7 million per buffer for a correct draw)
    for name, k, p in (("hidden", kh, p_h), ("att", ka, p_a)):
        n = k.numel()
        share, sigma = float(k.double().mean()), math.sqrt(p * (1 - p) / n)
        print("%s: n %d, share of ones %.5f, expected %.2f, %.2f sigma" % (name, n, share, 1 - p, (share - (1 - p)) / sigma))
        assert abs(share - (1 - p)) <= 5 * sigma
    # not swapped: each buffer is far from the other's probability (0.2 apart, sigma < 0.009)
    assert abs(float(kh.double().mean()) - (1 - p_a)) > 0.1 and abs(float(ka.double().mean()) - (1 - p_h)) > 0.1
    # None for p = 0, and for the attention site of an encoder without layers
    assert draw_keep(L, B, T, H, heads, 0.0, p_a, "cpu")[0] is None
    assert draw_keep(L, B, T, H, heads, p_h, 0.0, "cpu")[1] is None
    assert draw_keep(L, B, T, H, heads, 0.0, 0.0, "cpu") == (None, None)
    kh0, ka0 = draw_keep(0, B, T, H, heads, p_h, p_h, "cpu")
    assert tuple(kh0.shape) == (1, B * T, H) and ka0 is None
    # equal probabilities: one draw, two views of it, the hidden planes first (4-byte aligned)
    torch.manual_seed(5)
    kh, ka = draw_keep(L, B, T, H, heads, p_h, p_h, "cpu")
    assert tuple(kh.shape) == sh and tuple(ka.shape) == sa
    assert ka.data_ptr() == kh.data_ptr() + kh.numel() and kh.data_ptr() % 4 == 0
    torch.manual_seed(5)
    one = torch.empty(kh.numel() + ka.numel(), dtype=torch.uint8).bernoulli_(1 - p_h)
    assert torch.equal(one[:kh.numel()].view(sh), kh) and torch.equal(one[kh.numel():].view(sa), ka)
