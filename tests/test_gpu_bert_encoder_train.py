"""The training-mode forward of the frozen question encoder on the MI355X (``ops.bert_encode_train``,
``ops.bert_attention_drop``, ``GNNRAG_HIP_LM_TRAIN``) against transformers' own modules in float64 with the SAME dropout
masks injected (tests/bert_dropout_oracle.py; the oracle runs on the CPU).

Bound of every comparison: ``bert_oracle.bound(e_ref) = max(4 e_ref, 1e-6)`` of the error relative to the oracle's largest
entry, where e_ref is the fp32 transformers module's (for the attention step: the fp32 torch statement's) own distance from
float64 on the same ids and the same masks.  Error, e_ref and their ratio are printed before they are asserted."""
import numpy as np
import pytest
import torch

import bert_dropout_oracle as do
import bert_oracle as bo
import lm_variants_oracle as lo

pytestmark = pytest.mark.gpu
MATH_FP32, MATH_BF16X3 = 0, 1
PROBS = [(0.1, 0.1), (0.5, 0.3)]


@pytest.fixture(scope="module")
def dev():
    pytest.importorskip("transformers")
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


# -- attention alone -------------------------------------------------------------------------------------------------

# a single key; several waves; a full wave of keys; the first key in a lane's second slot; the largest T.  B and heads
# >= 2 wherever T allows a cheap case: a wrong stride of the mask shows
ATT = [(2, 1, 1, 32), (3, 9, 2, 32), (2, 64, 2, 64), (2, 65, 2, 32), (1, 128, 1, 64)]


def _att_inputs(B, T, heads, dh, p, bias):
    rs = np.random.RandomState(200 + T + int(100 * p))
    qkv = rs.standard_normal((B * T, 3 * heads * dh)).astype(np.float32)
    keep = (rs.random_sample((B, heads, T, T)) >= p).astype(np.uint8)
    keep[0, 0, 0, 0] = 1                                                    # T = 1: not every row may be dropped
    keep[B - 1, heads - 1, T // 2, :] = 0                                   # one query row fully dropped
    rel = rs.standard_normal((heads, 2 * T - 1)).astype(np.float32) if bias else None
    return qkv, keep, rel


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,T,heads,dh", ATT)
def test_attention_drop_against_float64(dev, B, T, heads, dh, p, bias):
    from gnnrag_amd import ops
    qkv, keep, rel = _att_inputs(B, T, heads, dh, p, bias)
    s = do.scale(p)
    want = do.attention64(qkv, B, T, heads, dh, keep, s, rel)
    e_ref = bo.rel_err(do.attention32(qkv, B, T, heads, dh, keep, s, rel), want)
    args = (torch.from_numpy(qkv).to(dev), B, T, heads, dh, torch.from_numpy(keep).to(dev), s)
    rel_d = None if rel is None else torch.from_numpy(rel).to(dev)
    got = ops.bert_attention_drop(*args, rel_bias=rel_d)
    err = bo.rel_err(got.cpu().numpy(), want)
    print("attention_drop B=%d T=%d heads=%d dh=%d p=%.1f bias=%d: err %.3g, e_ref %.3g, ratio %.2f"
          % (B, T, heads, dh, p, bias, err, e_ref, err / max(e_ref, 1e-30)))
    assert got.shape == (B * T, heads * dh)
    assert err <= bo.bound(e_ref)
    row = got.view(B, T, heads, dh)[B - 1, T // 2, heads - 1]
    assert torch.equal(row, torch.zeros_like(row))                          # the fully dropped row: exactly 0
    assert torch.equal(got, ops.bert_attention_drop(*args, rel_bias=rel_d))


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("B,T,heads,dh", ATT)
def test_attention_all_ones_is_the_inference_kernel(dev, B, T, heads, dh, bias):
    from gnnrag_amd import ops
    qkv, keep, rel = _att_inputs(B, T, heads, dh, 0.5, bias)
    qkv_d = torch.from_numpy(qkv).to(dev)
    rel_d = None if rel is None else torch.from_numpy(rel).to(dev)
    plain = ops.bert_attention(qkv_d, B, T, heads, dh, rel_bias=rel_d)
    ones = torch.ones(B, heads, T, T, dtype=torch.uint8, device=dev)
    assert torch.equal(ops.bert_attention_drop(qkv_d, B, T, heads, dh, ones, 1.0, rel_bias=rel_d), plain)
    # any byte != 0 keeps; a mask at an odd address (a view one byte into a buffer) is read byte by byte
    odd = torch.empty(ones.numel() + 1, dtype=torch.uint8, device=dev)[1:].view(B, heads, T, T)
    odd.copy_(torch.from_numpy(keep).to(dev) * 255)
    assert odd.data_ptr() % 2 == 1
    want = ops.bert_attention_drop(qkv_d, B, T, heads, dh, torch.from_numpy(keep).to(dev), 2.0, rel_bias=rel_d)
    assert torch.equal(ops.bert_attention_drop(qkv_d, B, T, heads, dh, odd, 2.0, rel_bias=rel_d), want)


# -- the whole encode -------------------------------------------------------------------------------------------------

CASES = {
    "minilm-L1-1x1": ("bert", bo.MINILM, 1, 1, 1),
    "minilm-L2-3x9": ("bert", bo.MINILM, 2, 3, 9),                  # plane indexing across layers needs L >= 2
    "base-L1-2x7": ("bert", bo.BERT_BASE, 1, 2, 7),
    "roberta32-L2-3x9": ("roberta", lo.SMALL[32], 2, 3, 9),
    "roberta64-L2-3x9": ("roberta", lo.SMALL[64], 2, 3, 9),
    "mpnet32-L2-3x9": ("mpnet", lo.SMALL[32], 2, 3, 9),
    "mpnet64-L2-3x9": ("mpnet", lo.SMALL[64], 2, 3, 9),
    "minilm-L0-2x32": ("bert", bo.MINILM, 0, 2, 32),                # L = 0 at T = max_pos: plane 0 alone
}
_models, _refs = {}, {}


def _model(name):
    if name not in _models:
        arch, shape, L, B, T = CASES[name]
        if arch == "bert":
            pair = do.make_bert(shape, L, seed=41)
            ids = np.random.RandomState(42).randint(0, 64, (B, T))
        else:
            pair = do.make_variant(arch, shape, L, seed=41)
            ids = lo.ids_with_pads(B, T)                            # pad ids present
        _models[name] = (pair[0], pair[1], ids)
    return _models[name]


def _ref(name, p_hidden, p_att):
    """(fp32 model, ids, packed masks, scales, float64 states, e_ref): computed once on the CPU, shared, not modified.
    A probability of None leaves that site alone (its mask is NULL)."""
    key = (name, p_hidden, p_att)
    if key not in _refs:
        _, shape, L, B, T = CASES[name]
        m32, m64, ids = _model(name)
        masks = do.draw(43, L, B, T, shape["H"], shape["heads"], p_hidden, p_att)
        sh, sa = (1.0 if p_hidden is None else do.scale(p_hidden)), (1.0 if p_att is None else do.scale(p_att))
        want = do.run(m64, ids, masks, sh, sa)
        e_ref = bo.rel_err(do.run(m32, ids, masks, sh, sa), want)
        _refs[key] = (m32, ids, do.pack(masks, L), (sh, sa), want, e_ref)
    return _refs[key]


def _check(dev, name, p_hidden, p_att, math):
    m32, ids, (kh, ka), (sh, sa), want, e_ref = _ref(name, p_hidden, p_att)
    got = do.encode_train(dev, m32, ids, kh, ka, sh, sa, math=math)
    err = bo.rel_err(got.cpu().numpy(), want)
    print("encode_train %s p=(%s, %s) math=%d: err %.3g, e_ref %.3g, ratio %.2f, bound %.3g"
          % (name, p_hidden, p_att, math, err, e_ref, err / max(e_ref, 1e-30), bo.bound(e_ref)))
    assert got.shape == want.shape
    assert err <= bo.bound(e_ref)
    return got


@pytest.mark.parametrize("math", [MATH_FP32, MATH_BF16X3], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("p_hidden,p_att", PROBS)
@pytest.mark.parametrize("name", list(CASES))
def test_encode_train_against_the_oracle(dev, name, p_hidden, p_att, math):
    got = _check(dev, name, p_hidden, p_att, math)
    m32, ids, (kh, ka), (sh, sa), _, _ = _ref(name, p_hidden, p_att)
    assert torch.equal(got, do.encode_train(dev, m32, ids, kh, ka, sh, sa, math=math))      # the same call twice


@pytest.mark.parametrize("math", [MATH_FP32, MATH_BF16X3], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("p_hidden,p_att", [(0.5, None), (None, 0.3)], ids=["hidden-only", "attention-only"])
@pytest.mark.parametrize("name", ["minilm-L2-3x9", "mpnet32-L2-3x9"])
def test_one_site_alone(dev, name, p_hidden, p_att, math):
    _check(dev, name, p_hidden, p_att, math)


@pytest.mark.parametrize("name", ["minilm-L2-3x9", "roberta32-L2-3x9", "mpnet64-L2-3x9", "minilm-L0-2x32"])
def test_null_masks_are_the_inference_call(dev, name):
    m32, _, ids = _model(name)
    for math in (MATH_FP32, MATH_BF16X3):
        plain = do.encode_train(dev, m32, ids, None, None, math=math, plain=True)
        assert torch.equal(do.encode_train(dev, m32, ids, None, None, math=math), plain)
        # scales of masks that are not given are not read
        assert torch.equal(do.encode_train(dev, m32, ids, None, None, float("nan"), -1.0, math=math), plain)


@pytest.mark.parametrize("name", ["minilm-L2-3x9", "mpnet32-L2-3x9"])
def test_a_question_depends_on_its_own_slices_only(dev, name):
    _, shape, L, B, T = CASES[name]
    m32, ids, (kh, ka), (sh, sa), _, _ = _ref(name, 0.5, 0.3)
    batch = do.encode_train(dev, m32, ids, kh, ka, sh, sa)
    for b in range(B):
        kh_b = np.ascontiguousarray(kh.reshape(1 + 2 * L, B, T, -1)[:, b]).reshape(1 + 2 * L, T, -1)
        alone = do.encode_train(dev, m32, ids[b:b + 1], kh_b, np.ascontiguousarray(ka[:, b:b + 1]), sh, sa)
        assert torch.equal(alone, batch[b:b + 1])


# -- the module ---------------------------------------------------------------------------------------------------------

class _Holder:
    def __init__(self, enc):
        self.node_encoder = enc


def _count_original(enc):
    p = enc._gnnrag_lm_patch
    calls, orig = [], p.orig_forward

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    p.orig_forward = counted
    return p, calls


def _module_checks(dev, monkeypatch, enc, m32, m64, ids):
    """``enc``: the patched encoder on the device (training mode, frozen); ``m32`` / ``m64``: eager CPU copies of it."""
    from gnnrag_amd.modules.question_encoding import lm_encoder as le
    cfg = enc.config
    L, H, heads = int(cfg.num_hidden_layers), int(cfg.hidden_size), int(cfg.num_attention_heads)
    B, T = ids.shape
    assert cfg.hidden_dropout_prob == 0.1 and cfg.attention_probs_dropout_prob == 0.1
    p, calls = _count_original(enc)
    q = torch.from_numpy(ids).long().to(dev)
    masks = do.draw(51, L, B, T, H, heads, 0.1, 0.1)
    kh, ka = do.pack(masks, L)
    s = do.scale(0.1)
    want = do.run(m64, ids, masks, s, s)
    e_ref = bo.rel_err(do.run(m32, ids, masks, s, s), want)
    asked = []

    def known(*a):
        asked.append(a)
        return torch.from_numpy(kh).to(dev), torch.from_numpy(ka).to(dev)

    enc.train()
    with monkeypatch.context() as m:
        m.setattr(le, "draw_keep", known)
        out = enc(q)                                        # grad mode on: a frozen LM needs no gradient
    err = bo.rel_err(out[0].cpu().numpy(), want)
    print("%s in training mode, known masks: err %.3g, e_ref %.3g, ratio %.2f" % (type(enc).__name__, err, e_ref,
                                                                                  err / max(e_ref, 1e-30)))
    assert asked == [(L, B, T, H, heads, 0.1, 0.1, q.device)]
    assert not calls and p.hip_calls == 1 and p.hip_train_calls == 1 and not hasattr(out, "pooler_output")
    assert not out[0].requires_grad and err <= bo.bound(e_ref)
    # the module's own draws: two calls differ, equal seeds give equal states
    torch.manual_seed(77)
    a = enc(q)[0]
    b = enc(q)[0]
    torch.manual_seed(77)
    c = enc(q)[0]
    assert not torch.equal(a, b) and torch.equal(a, c) and not calls and p.hip_train_calls == 4
    # back in eval mode: the inference call's bits
    enc.eval()
    with torch.no_grad():
        e = enc(q)[0]
    assert p.hip_calls == 5 and p.hip_train_calls == 4 and not calls
    assert torch.equal(e, do.encode_train(dev, m32, ids, None, None, plain=True))
    assert not torch.equal(e, a)
    # the switch off again: transformers' own forward
    enc.train()
    monkeypatch.setenv("GNNRAG_HIP_LM_TRAIN", "0")
    enc(q)
    assert len(calls) == 1 and p.hip_calls == 5


def test_bert_module_in_training_mode(dev, monkeypatch):
    import test_gpu_bert_encoder as base
    from gnnrag_amd import install
    mod, _, g = base._fixture_module(dev)
    shape = dict(H=int(g["cfg.H"]), heads=int(g["cfg.heads"]), I=int(g["cfg.I"]))
    m32, m64 = do.make_bert(shape, int(g["cfg.L"]), int(g["cfg.seed"]), vocab=int(g["cfg.vocab"]),
                            max_pos=int(g["cfg.max_pos"]))
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    monkeypatch.setenv("GNNRAG_HIP_LM_TRAIN", "1")
    install.patch_lm_encoder(base._Model(mod))
    mod.train()
    _module_checks(dev, monkeypatch, mod.node_encoder, m32, m64, np.asarray(g["q_input"]))


@pytest.mark.parametrize("arch", lo.ARCHS)
def test_variant_module_in_training_mode(dev, monkeypatch, arch):
    from gnnrag_amd.modules.question_encoding.lm_encoder import patch_lm_encoder
    m32, m64 = do.make_variant(arch, lo.SMALL[32], 2, seed=61)
    enc = do.make_variant(arch, lo.SMALL[32], 2, seed=61)[0].to(dev)
    for q in enc.parameters():
        q.requires_grad_(False)
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")                 # these classes are off when the switch is unset
    monkeypatch.setenv("GNNRAG_HIP_LM_TRAIN", "1")
    patch_lm_encoder(_Holder(enc))
    _module_checks(dev, monkeypatch, enc, m32, m64, lo.ids_with_pads(3, 9))
