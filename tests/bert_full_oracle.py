"""Oracle additions for fine-tuning the WHOLE LM question encoder (a helper, not a test): MPNet's layer parameter names
for ``bert_grad_oracle.compare``, and the numpy float64 statements of the new kernels - the embedding backward with its
dense table gradients, the attention backward with the relative bias, and the bias-table gradient.  The module-level
oracle stays ``bert_grad_oracle.grads`` (transformers in float64 under autograd with injected masks); nothing here is
derived from the code under test."""
import numpy as np

import bert_grad_oracle as go


def layer_names(model, l):
    """``bert_grad_oracle.layer_names`` for any of the three classes (MPNet names its projections attn.q / k / v / o)."""
    if not hasattr(model.encoder, "relative_attention_bias"):
        return go.layer_names(model, l)
    p = "encoder.layer.%d." % l
    a = p + "attention.attn."
    return {"dW_qkv": [a + "q.weight", a + "k.weight", a + "v.weight"],
            "db_qkv": [a + "q.bias", a + "k.bias", a + "v.bias"],
            "dW_o": a + "o.weight", "db_o": a + "o.bias", "dln1_g": p + "attention.LayerNorm.weight",
            "dln1_b": p + "attention.LayerNorm.bias", "dW_i": p + "intermediate.dense.weight",
            "db_i": p + "intermediate.dense.bias", "dW_f": p + "output.dense.weight", "db_f": p + "output.dense.bias",
            "dln2_g": p + "output.LayerNorm.weight", "dln2_b": p + "output.LayerNorm.bias"}


def key_bias_names(model):
    """The key projections' bias names: their gradient is mathematically zero and the library writes exactly 0."""
    mpnet = hasattr(model.encoder, "relative_attention_bias")
    return [n for n, _ in model.named_parameters() if n.endswith("attn.k.bias" if mpnet else "key.bias")]


def positions(ids, pad_id, vocab, max_pos):
    """The position row of every token as the embedding forward saves it: ``t`` (pad_id None) or RoBERTa's rule from the
    ids; -1 where the id or the position lies outside its table."""
    ids = np.asarray(ids)
    B, T = ids.shape
    if pad_id is None:
        pos = np.tile(np.arange(T), (B, 1))
    else:
        pos = np.where(ids != pad_id, pad_id + np.cumsum(ids != pad_id, axis=1), pad_id)
    bad = (ids < 0) | (ids >= vocab) | (pos < 0) | (pos >= max_pos)
    return np.where(bad, -1, pos).astype(np.int64)


def scatter64(dz, keys, rows, pad=None):
    """``out [rows, H]``: row k is the float64 sum of the ``dz`` rows q with ``keys[q] == k``; keys outside ``[0, rows)``
    and the key ``pad`` add nothing."""
    dz = np.asarray(dz, dtype=np.float64)
    out = np.zeros((rows, dz.shape[1]))
    for q, k in enumerate(np.asarray(keys).reshape(-1).tolist()):
        if 0 <= k < rows and k != pad:
            out[k] += dz[q]
    return out


def embed_bwd64(g_x0, ids, word_emb, pos_emb, type_emb, ln_g, eps, pad_id=None, keep=None, scale=1.0, word_pad=None,
                pos_pad=None):
    """``{d_word, d_pos, d_type, d_ln_g, d_ln_b, dz}`` of ``x0 = LN(word[id] + type[0] + pos[p]) g + b`` times the mask
    (the dropout sits BEHIND the LayerNorm), for the upstream ``g_x0``; a token with position -1 adds to no table."""
    ids = np.asarray(ids)
    word, posw = np.asarray(word_emb, dtype=np.float64), np.asarray(pos_emb, dtype=np.float64)
    H = word.shape[1]
    pos = positions(ids, pad_id, word.shape[0], posw.shape[0]).reshape(-1)
    flat = ids.reshape(-1)
    assert (pos >= 0).all(), "the float64 statement is for rows inside their tables"
    sum0 = word[flat] + posw[pos] + (0.0 if type_emb is None else np.asarray(type_emb, dtype=np.float64)[0])
    g = np.asarray(g_x0, dtype=np.float64).reshape(-1, H)
    dy = g if keep is None else g * np.asarray(keep, dtype=np.float64).reshape(-1, H) * float(scale)
    dz, _, d_ln_g, d_ln_b = go.ln_bwd64(dy, sum0, ln_g, eps)
    out = {"dz": dz, "d_ln_g": d_ln_g, "d_ln_b": d_ln_b, "d_word": scatter64(dz, flat, word.shape[0], word_pad),
           "d_pos": scatter64(dz, pos, posw.shape[0], pos_pad), "d_type": None}
    if type_emb is not None:
        out["d_type"] = np.zeros(np.asarray(type_emb).shape)
        out["d_type"][0] = dz.sum(0)
    return out


def rel_bias_reduce64(ds, B, T, heads):
    """``d_bias [heads, 2T-1]``: entry ``[h, d + T - 1]`` is the sum of ``ds[b, h, i, i + d]`` over b and i."""
    ds = np.asarray(ds, dtype=np.float64).reshape(B, heads, T, T)
    out = np.zeros((heads, 2 * T - 1))
    for d in range(-(T - 1), T):
        out[:, d + T - 1] = np.trace(ds, offset=d, axis1=2, axis2=3).sum(0)
    return out


def attention_bias_bwd64(qkv, d_ctx, B, T, heads, dh, rel_bias, keep=None, scale=1.0):
    """``(d_qkv, d_bias, dS)`` of ``ctx = (softmax(q k^T / sqrt(dh) + bias[h, j - i + T - 1]) * keep * scale) v``."""
    x = np.asarray(qkv, dtype=np.float64).reshape(B, T, 3, heads, dh)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    do = np.asarray(d_ctx, dtype=np.float64).reshape(B, T, heads, dh)
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    s = np.einsum("bihd,bjhd->bhij", q, k) / np.sqrt(dh) + np.asarray(rel_bias, dtype=np.float64)[:, j - i + T - 1][None]
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    m = np.ones_like(p) if keep is None else np.asarray(keep, dtype=np.float64) * float(scale)
    pt = p * m
    dpt = np.einsum("bihd,bjhd->bhij", do, v)
    ds = p * (dpt * m - (pt * dpt).sum(-1, keepdims=True))
    dq = np.einsum("bhij,bjhd->bihd", ds, k) / np.sqrt(dh)
    dk = np.einsum("bhij,bihd->bjhd", ds, q) / np.sqrt(dh)
    dv = np.einsum("bhij,bihd->bjhd", pt, do)
    return np.stack([dq, dk, dv], axis=2).reshape(B * T, 3 * heads * dh), rel_bias_reduce64(ds, B, T, heads), ds
