"""Oracle of the training-mode question-encoder tests: transformers' own ``BertModel`` / ``RobertaModel`` / ``MPNetModel``
in float64, in TRAINING mode, with ``torch.nn.functional.dropout`` replaced for the duration of one call by a function
that multiplies in masks the test brings (a helper, not a test).

transformers calls ``F.dropout`` at four sites, in this order (``call_order``; recorded on the installed version with
``_attn_implementation = "eager"`` and asserted by tests/test_bert_dropout_host.py for all three classes):

    embedding output [B,T,H];  per layer: attention probabilities [B,heads,T,T], attention output projection [B,T,H],
    FFN output projection [B,T,H]

Models are built by ``bert_oracle.make_model`` / ``lm_variants_oracle.make_model`` (seeded weights, nothing downloaded) on a
configuration whose attention implementation is "eager": the fused attention of the default implementation draws its
dropout inside one call and cannot be given a mask.  The masks come from ``np.random.RandomState(seed)``; ``pack`` lays
them out as ``ops.bert_encode_train`` reads them.  The float64 module is the oracle, the fp32 module with the SAME masks
gives ``e_ref`` of ``bert_oracle.bound``."""
import numpy as np
import torch

import bert_oracle as bo
import lm_variants_oracle as lo


def eager(cfg):
    cfg._attn_implementation = "eager"
    return cfg


def make_bert(shape, L, seed, vocab=64, max_pos=32):
    """(fp32, float64) ``BertModel`` of ``bert_oracle`` with eager attention."""
    return bo.make_model(eager(bo.config(L=L, vocab=vocab, max_pos=max_pos, **shape)), seed)


def make_variant(arch, shape, L, seed, **kw):
    """(fp32, float64) model of ``lm_variants_oracle`` with eager attention."""
    return lo.make_model(arch, eager(lo.config(arch, L=L, **shape, **kw)), seed)


def call_order(L, B, T, H, heads):
    """[(site, shape)] in the order transformers calls ``F.dropout``; site is "hidden" or "att"."""
    out = [("hidden", (B, T, H))]
    for _ in range(L):
        out += [("att", (B, heads, T, T)), ("hidden", (B, T, H)), ("hidden", (B, T, H))]
    return out


def scale(p):
    """float32(1 / (1 - p)): the multiplier of a kept element, the value the library is given."""
    return float(np.float32(1.0 / (1.0 - p)))


def draw(seed, L, B, T, H, heads, p_hidden, p_att):
    """The masks of one call in call order, uint8 numpy arrays (1 keeps) from ``RandomState(seed)``; ``None`` at every
    site whose probability is ``None`` (that site is left alone: the library's NULL mask)."""
    rs = np.random.RandomState(seed)
    out = []
    for site, shape in call_order(L, B, T, H, heads):
        p = p_hidden if site == "hidden" else p_att
        out.append(None if p is None else (rs.random_sample(shape) >= p).astype(np.uint8))
    return out


def ones(L, B, T, H, heads):
    return [np.ones(shape, dtype=np.uint8) for _, shape in call_order(L, B, T, H, heads)]


def pack(masks, L):
    """(keep_hidden [1+2L, B*T, H] | None, keep_att [L, B, heads, T, T] | None) of ``ops.bert_keep_shapes`` from masks in
    call order.  All hidden sites (all attention sites) are given or none is."""
    hidden = [masks[0]] + [m for l in range(L) for m in (masks[2 + 3 * l], masks[3 + 3 * l])]
    att = [masks[1 + 3 * l] for l in range(L)]
    assert len({m is None for m in hidden}) == 1 and len({m is None for m in att}) <= 1
    keep_hidden = None if hidden[0] is None else np.stack([m.reshape(-1, m.shape[-1]) for m in hidden])
    keep_att = None if not att or att[0] is None else np.stack(att)
    return keep_hidden, keep_att


def run(model, ids, masks, scale_hidden=1.0, scale_att=1.0, record=None):
    """last_hidden_state of ``model`` in training mode on ``ids`` (numpy int64 [B,T]) with ``F.dropout`` replaced: the
    n-th call takes the n-th mask, asserts that its shape is its input's and returns ``x * keep * scale`` (``x`` itself
    for a ``None`` mask); afterwards every mask must have been consumed.  ``record`` (a list) receives the shape and rank
    of every call.  The model is returned to the mode it was in."""
    import torch.nn.functional as F
    todo = list(masks)
    orig, was_training = F.dropout, model.training
    dtype = next(model.parameters()).dtype

    def replacement(x, p=0.5, training=True, inplace=False):
        assert training and todo, "an unexpected dropout call"
        keep = todo.pop(0)
        if record is not None:
            record.append(("att" if x.dim() == 4 else "hidden", tuple(x.shape)))
        if keep is None:
            return x
        assert tuple(keep.shape) == tuple(x.shape), (keep.shape, tuple(x.shape))
        return x * torch.from_numpy(keep).to(dtype) * (scale_att if x.dim() == 4 else scale_hidden)

    F.dropout = replacement
    try:
        model.train()
        with torch.no_grad():
            out = model(torch.from_numpy(np.asarray(ids, dtype=np.int64)))[0].numpy()
    finally:
        F.dropout = orig
        model.train(was_training)
    assert not todo, "%d masks were not consumed" % len(todo)
    return out


def encode_train(dev, model, ids, keep_hidden, keep_att, scale_hidden=1.0, scale_att=1.0, math=None, L=None, wrap=None,
                 plain=False):
    """``ops.bert_encode_train`` of ``model`` (any of the three classes) on ``ids`` (numpy) on ``dev`` with the packed
    numpy masks (or None); ``wrap(tensor, role)`` may replace every device tensor (guarded copies).  ``plain``:
    ``ops.bert_encode`` on the same arguments instead."""
    from gnnrag_amd import ops
    w = (lambda t, role: t) if wrap is None else wrap
    ids = np.asarray(ids)
    P = lo.layer_params(model, ids.shape[1])
    layers = P["layers"] if L is None else P["layers"][:L]
    layers = [{k: w(v.detach().to(dev), "layers[%d].%s" % (i, k)) for k, v in d.items()} for i, d in enumerate(layers)]
    top = {k: (None if P[k] is None else w(P[k].detach().to(dev), k))
           for k in ("word_emb", "pos_emb", "type_emb", "ln_g", "ln_b", "rel_bias")}
    args = (w(torch.from_numpy(ids).long().to(dev), "ids"), top["word_emb"], top["pos_emb"], top["type_emb"], top["ln_g"],
            top["ln_b"], P["eps"], layers, P["heads"])
    kw = dict(I=P["I"], math=math, pad_id=P["pad_id"], rel_bias=top["rel_bias"])
    if plain:
        return ops.bert_encode(*args, **kw)
    kh = None if keep_hidden is None else w(torch.from_numpy(keep_hidden).to(dev), "keep_hidden")
    ka = None if keep_att is None else w(torch.from_numpy(keep_att).to(dev), "keep_att")
    return ops.bert_encode_train(*args, keep_hidden=kh, scale_hidden=scale_hidden, keep_att=ka, scale_att=scale_att, **kw)


def attention64(qkv, B, T, heads, dh, keep, scale_att, rel_bias=None):
    """numpy float64: softmax, then keep * scale, then the weighted sum; qkv [B*T, 3*heads*dh], keep [B,heads,T,T]."""
    x = np.asarray(qkv, dtype=np.float64).reshape(B, T, 3, heads, dh)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    s = np.einsum("bihd,bjhd->bhij", q, k) / np.sqrt(dh)
    if rel_bias is not None:
        i, j = np.arange(T)[:, None], np.arange(T)[None, :]
        s = s + np.asarray(rel_bias, dtype=np.float64)[:, j - i + T - 1][None]
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    p = p * np.asarray(keep, dtype=np.float64) * float(scale_att)
    return np.einsum("bhij,bjhd->bihd", p, v).reshape(B * T, heads * dh)


def attention32(qkv, B, T, heads, dh, keep, scale_att, rel_bias=None):
    """The fp32 torch statement of the same steps (the yardstick ``e_ref`` of the attention tests)."""
    x = torch.from_numpy(np.asarray(qkv, dtype=np.float32)).view(B, T, 3, heads, dh)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) / float(np.sqrt(dh))
    if rel_bias is not None:
        i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
        s = s + torch.from_numpy(np.asarray(rel_bias, dtype=np.float32))[:, j - i + T - 1][None]
    p = torch.softmax(s, dim=-1) * torch.from_numpy(np.asarray(keep)).float() * float(scale_att)
    return torch.matmul(p, v).permute(0, 2, 1, 3).reshape(B * T, heads * dh).numpy()
