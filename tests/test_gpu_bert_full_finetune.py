"""Fine-tuning the whole LM question encoder on the MI355X, composed: the embedding stage, the layers (with MPNet's relative
bias) and their backwards from the ids to every parameter gradient, at the ops level and through the patched module with
``GNNRAG_HIP_LM_FINETUNE_FULL=1``, for ``BertModel``, ``RobertaModel`` and ``MPNetModel`` - against transformers' float64
module under autograd with injected masks (tests/bert_grad_oracle.py).

Bound (the issue's): per gradient tensor ``bert_oracle.bound(e_ref) = max(4 e_ref, 1e-6)``, errors relative to the tensor's
largest float64 entry, ``e_ref`` the fp32 transformers module's own distance from the float64 one on the same ids, masks and
upstream gradient.  The key projections' bias is outside the relative bound: the library writes exactly 0."""
import copy

import numpy as np
import pytest
import torch

import bert_dropout_oracle as do
import bert_full_oracle as fo
import bert_grad_oracle as go
import lm_variants_oracle as lo

pytestmark = pytest.mark.gpu
ARCHS = ("bert", "roberta", "mpnet")


@pytest.fixture(scope="module")
def dev():
    pytest.importorskip("transformers")
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev)


def _models(arch, shape, L, seed):
    if arch == "bert":
        return do.make_bert(shape, L, seed=seed, max_pos=16)
    return do.make_variant(arch, shape, L, seed=seed)


def _ids(arch, B, T, seed):
    """Pads and repeated tokens: the pad patterns of lm_variants_oracle for RoBERTa / MPNet; for BERT random ids with its
    pad id 0 (whose table row gets no gradient) and a repeated token in every question."""
    if arch != "bert":
        return lo.ids_with_pads(B, T, seed=seed)
    ids = np.random.RandomState(seed).randint(0, 64, (B, T))
    ids[:, T - 1] = ids[:, 0]
    ids[0, T // 2:] = 0
    return ids


def _pads(arch):
    """(word_pad, pos_pad): transformers' padding_idx of the two tables."""
    return (0, None) if arch == "bert" else (lo.PAD, lo.PAD)


def _emb_names(arch):
    names = {"d_word": "embeddings.word_embeddings.weight", "d_pos": "embeddings.position_embeddings.weight",
             "d_ln_g": "embeddings.LayerNorm.weight", "d_ln_b": "embeddings.LayerNorm.bias"}
    if arch != "mpnet":
        names["d_type"] = "embeddings.token_type_embeddings.weight"
    return names


def _bias_weight_grad(model, d_table, T):
    """The gradient of ``relative_attention_bias.weight`` [32, heads] from the table's [heads, 2T-1]: the transpose of the
    gather ``table = weight[bucket].t()`` with transformers' own buckets, in float64 on the library's fp32 numbers."""
    d = torch.arange(-(T - 1), T, dtype=torch.long)
    bucket = type(model.encoder).relative_position_bucket(d, num_buckets=32).numpy()
    out = np.zeros((32, d_table.shape[0]))
    np.add.at(out, bucket, np.asarray(d_table, dtype=np.float64).T)
    return out


CASES = [(arch, w, L) for arch in ARCHS for w in (32, 64) for L in (1, 2)]


@pytest.mark.parametrize("arch,width,L", CASES)
@pytest.mark.parametrize("drops", [(0.1, 0.1), (None, None)])
def test_whole_encoder_backward_against_the_oracle(dev, arch, width, L, drops):
    """ids -> x0 -> out and back on the ops: equal bits with bert_encode_train forward, every parameter gradient within the
    bound backward."""
    from gnnrag_amd import ops
    shape, B, T = lo.SMALL[width], 3, 9
    H, heads = shape["H"], shape["heads"]
    m32, m64 = _models(arch, shape, L, seed=81)
    rs = np.random.RandomState(82)
    ids = _ids(arch, B, T, 83)
    p_h, p_a = drops
    masks = do.draw(84, L, B, T, H, heads, p_h, p_a)
    scales = (do.scale(p_h) if p_h is not None else 1.0, do.scale(p_a) if p_a is not None else 1.0)
    g_out = rs.standard_normal((B, T, H)).astype(np.float32)
    G64 = go.grads(m64, [(ids, masks, *scales)], [g_out])
    G32 = go.grads(m32, [(ids, masks, *scales)], [g_out])
    kh, ka = do.pack(masks, L)

    P = lo.layer_params(m32, T)
    layers = [{k: v.detach().to(dev) for k, v in d.items()} for d in P["layers"]]
    top = {k: (None if P[k] is None else P[k].detach().to(dev)) for k in ("word_emb", "pos_emb", "type_emb", "ln_g", "ln_b",
                                                                           "rel_bias")}
    ids_d = _t(ids, dev, np.int64)
    kh_d, ka_d = (None if k is None else _t(k, dev, np.uint8) for k in (kh, ka))
    x0, e_res = ops.bert_embed_forward_save(ids_d, top["word_emb"], top["pos_emb"], top["type_emb"], top["ln_g"], top["ln_b"],
                                            P["eps"], pad_id=P["pad_id"], keep=None if kh_d is None else kh_d[0],
                                            scale=scales[0])
    kw = dict(keep_hidden=kh_d, scale_hidden=scales[0], keep_att=ka_d, scale_att=scales[1], rel_bias=top["rel_bias"])
    out, reserve = ops.bert_layers_forward_save(x0, layers, heads, P["eps"], B, T, **kw)
    assert torch.equal(out, do.encode_train(dev, m32, ids, kh, ka, scales[0], scales[1]))
    res = ops.bert_layers_backward(_t(g_out, dev), layers, heads, P["eps"], B, T, reserve,
                                   want_rel_bias_grad=arch == "mpnet", **kw)
    g_x0, grads = res[0], res[1]
    word_pad, pos_pad = _pads(arch)
    eg = ops.bert_embed_backward(g_x0, ids_d, e_res, top["ln_g"], P["eps"], int(top["word_emb"].shape[0]),
                                 int(top["pos_emb"].shape[0]), 0 if top["type_emb"] is None else int(top["type_emb"].shape[0]),
                                 word_pad=word_pad, pos_pad=pos_pad, keep=None if kh_d is None else kh_d[0], scale=scales[0])
    worst, seen = [0.0], set()
    for field, name in _emb_names(arch).items():
        go.compare(eg[field].cpu().numpy(), G64, G32, name, worst)
        seen.add(name)
    assert np.all(eg["d_word"][word_pad].cpu().numpy() == 0) and np.all(G64["embeddings.word_embeddings.weight"][word_pad] == 0)
    if arch == "mpnet":
        assert eg["d_type"] is None
        name = "encoder.relative_attention_bias.weight"
        go.compare(_bias_weight_grad(m32, res[2].cpu().numpy(), T), G64, G32, name, worst)
        seen.add(name)
    keys = fo.key_bias_names(m32)
    for l in range(L):
        for field, name in fo.layer_names(m32, l).items():
            got = grads[l][field].cpu().numpy()
            for k, nm in enumerate(name if isinstance(name, list) else [name]):
                part = got[H * k: H * (k + 1)] if isinstance(name, list) else got
                seen.add(nm)
                if nm in keys:
                    assert np.all(part == 0.0) and not np.signbit(part).any()
                    assert np.abs(G64[nm]).max() <= 1e-12 * np.abs(G64[name[0]]).max()
                else:
                    go.compare(part, G64, G32, nm, worst)
    # every parameter of the model that has a gradient was compared
    assert seen == {n for n, v in G64.items() if n not in ("x0", "g_x0") and v is not None}
    print("whole encoder %s width %d L=%d %s: largest err / e_ref %.2f" % (arch, width, L, drops, worst[0]))


class _Holder:
    def __init__(self, enc):
        self.node_encoder = enc


def _module_grads(dev, monkeypatch, m32, calls, g_outs, L, full):
    """The patched module on the GPU: one encode per call with ``draw_keep`` given the call's masks, then one backward of
    ``sum (out * g_out).sum()``.  With ``full`` nothing may reach ``F.dropout`` (the embedding stage runs on the library);
    without it the embedding site's ``F.dropout`` gets the call's mask.  Returns ({name: grad}, the patch state)."""
    import torch.nn.functional as F
    from gnnrag_amd.modules.question_encoding import lm_encoder as le
    enc = copy.deepcopy(m32).to(dev).train()
    le.patch_lm_encoder(_Holder(enc))
    p = enc._gnnrag_lm_patch
    total = None
    for (ids, masks, sh, sa), g in zip(calls, g_outs):
        kh, ka = do.pack(masks, L)
        monkeypatch.setattr(le, "draw_keep", lambda *a, kh=kh, ka=ka: (
            None if kh is None else _t(kh, dev, np.uint8), None if ka is None else _t(ka, dev, np.uint8)))
        emb = masks[0]

        def dropout(x, p=0.5, training=True, inplace=False, emb=emb, sh=sh):
            assert not full, "F.dropout was reached with the whole encoder on the library"
            assert tuple(x.shape) == tuple(emb.shape)
            return x * _t(emb, dev) * sh

        monkeypatch.setattr(F, "dropout", dropout)
        out = enc(torch.from_numpy(np.asarray(ids)).long().to(dev))[0]
        term = (out * _t(g, dev)).sum()
        total = term if total is None else total + term
    total.backward()
    return {n: (None if q.grad is None else q.grad.cpu().numpy()) for n, q in enc.named_parameters()}, p


def _module_case(arch, drop):
    shape, L, B, T = lo.SMALL[32], 2, 3, 9
    H, heads = shape["H"], shape["heads"]
    m32, m64 = _models(arch, shape, L, seed=91)
    rs = np.random.RandomState(92)
    sc = do.scale(drop) if drop else 1.0
    calls = [(_ids(arch, B, T, 93 + s), do.draw(95 + s, L, B, T, H, heads, drop, drop), sc, sc) for s in range(2)]
    g_outs = [rs.standard_normal((B, T, H)).astype(np.float32) for _ in range(2)]
    return m32, m64, calls, g_outs, L


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("drop", [0.1, None])
def test_module_finetune_full(dev, monkeypatch, arch, drop):
    """Two encodes and one backward (the ReaRev sequence) with the new switch on: every ``.grad`` - the three embedding
    tables, the embedding LayerNorm and MPNet's ``relative_attention_bias.weight`` included - within the bound."""
    m32, m64, calls, g_outs, L = _module_case(arch, drop)
    G64, G32 = go.grads(m64, calls, g_outs), go.grads(m32, calls, g_outs)
    if drop is None:                            # the patch reads the probabilities of the configuration: dropout inert
        m32.config.hidden_dropout_prob = m32.config.attention_probs_dropout_prob = 0.0
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    monkeypatch.setenv("GNNRAG_HIP_LM_FINETUNE", "1")
    monkeypatch.setenv("GNNRAG_HIP_LM_FINETUNE_FULL", "1")
    got, p = _module_grads(dev, monkeypatch, m32, calls, g_outs, L, full=True)
    assert p.hip_finetune_full_calls == 2 and p.hip_finetune_calls == 2 and p.hip_calls == 2 and p.hip_train_calls == 0
    worst, keys = [0.0], fo.key_bias_names(m32)
    for name, want in G64.items():
        if name in ("x0", "g_x0"):
            continue
        if want is None:
            assert name.startswith("pooler.") and got[name] is None
        elif name in keys:
            assert np.all(got[name] == 0.0)
        else:
            go.compare(got[name], G64, G32, name, worst)
    print("module %s dropout %s, whole encoder: largest err / e_ref %.2f" % (arch, drop, worst[0]))


def test_module_switch_off_is_the_layers_path(dev, monkeypatch):
    """With the new switch unset, "0" or empty a fine-tuning call is the call of GNNRAG_HIP_LM_FINETUNE alone: the embedding
    stage is transformers' (``F.dropout`` is reached), the counters are those of that path and the gradients have its
    bits; MPNet stays refused."""
    from gnnrag_amd.modules.question_encoding import lm_encoder as le
    m32, _, calls, g_outs, L = _module_case("roberta", 0.1)
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    monkeypatch.setenv("GNNRAG_HIP_LM_FINETUNE", "1")
    runs = []
    for value in (None, "0", ""):
        if value is None:
            monkeypatch.delenv("GNNRAG_HIP_LM_FINETUNE_FULL", raising=False)
        else:
            monkeypatch.setenv("GNNRAG_HIP_LM_FINETUNE_FULL", value)
        got, p = _module_grads(dev, monkeypatch, m32, calls, g_outs, L, full=False)
        assert p.hip_finetune_calls == 2 and p.hip_calls == 2 and p.hip_finetune_full_calls == 0
        runs.append(got)
    for other in runs[1:]:
        for n, v in runs[0].items():
            assert (v is None and other[n] is None) or np.array_equal(v.view(np.uint32), other[n].view(np.uint32)), n
    mp, _, mcalls, _, _ = _module_case("mpnet", 0.1)
    enc = copy.deepcopy(mp).to(dev).train()
    le.patch_lm_encoder(_Holder(enc))
    ids = torch.from_numpy(mcalls[0][0]).long().to(dev)
    assert enc._gnnrag_lm_patch.refusal((ids,), {}).startswith("a gradient is needed and the relative attention bias")
    monkeypatch.setenv("GNNRAG_HIP_LM_FINETUNE_FULL", "1")
    assert enc._gnnrag_lm_patch.refusal((ids,), {}) is None
