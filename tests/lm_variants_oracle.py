"""Oracle of the RoBERTa / MPNet question-encoder tests: transformers' own ``RobertaModel`` / ``MPNetModel`` / ``BertModel``
in float64, built as tests/bert_oracle.py builds its ``BertModel`` (seeded ``RandomState`` weights, nothing downloaded; the
fixture tests/golden/lm_variants_ref.npz stores config numbers and seeds, not weights).  The float64 module is the oracle,
the fp32 module's distance from it (``e_ref``) is the yardstick of ``bert_oracle.bound``.

Also here: a plain-Python statement of RoBERTa's position rule, the id patterns with pads that every test uses, the
arguments of ``ops.bert_encode`` read from a model by this file (not by the code under test), and MPNet's bias table read
off ``MPNetEncoder.compute_position_bias``."""
import copy

import numpy as np
import torch

import bert_oracle as bo

PAD = 1
VOCAB = 50
SMALL = {32: dict(H=64, heads=2, I=128), 64: dict(H=128, heads=2, I=256)}      # by head width
ARCHS = ("roberta", "mpnet")


def model_class(arch):
    import transformers
    return {"bert": transformers.BertModel, "roberta": transformers.RobertaModel, "mpnet": transformers.MPNetModel}[arch]


def config(arch, H, heads, I, L, vocab=VOCAB, max_pos=32, pad=PAD, **extra):
    import transformers
    common = dict(vocab_size=vocab, hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=I,
                  max_position_embeddings=max_pos, pad_token_id=pad)
    if arch == "bert":
        return transformers.BertConfig(type_vocab_size=2, **common, **extra)
    if arch == "roberta":
        return transformers.RobertaConfig(type_vocab_size=1, **common, **extra)
    assert pad == 1                             # MPNetEmbeddings hard-codes its padding_idx
    return transformers.MPNetConfig(**{"relative_attention_num_buckets": 32, **common, **extra})


def make_model(arch, cfg, seed):
    """(fp32 model, float64 copy), eval mode, weights from RandomState(seed) in named_parameters order: matrices x 0.05,
    vectors x 0.1, LayerNorm weights 1 + that, MPNet's relative attention bias x 1 (entries of O(1): a wrong bucket or a
    wrong sign moves the states far above any bound)."""
    model = model_class(arch)(cfg)
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            w = rs.standard_normal(tuple(p.shape)) * (0.05 if p.dim() >= 2 else 0.1)
            if name.endswith("LayerNorm.weight"):
                w = 1.0 + w
            if name.endswith("relative_attention_bias.weight"):
                w = w * 20.0
            p.copy_(torch.from_numpy(w.astype(np.float32)))
    model.eval()
    return model, copy.deepcopy(model).double().eval()


def positions(ids, pad):
    """RoBERTa's rule in plain Python: a pad sits at ``pad``, the n-th token that is not a pad (n from 1) at ``pad + n``."""
    out = []
    for row in np.asarray(ids).tolist():
        n, pos = 0, []
        for tok in row:
            if tok != pad:
                n += 1
                pos.append(pad + n)
            else:
                pos.append(pad)
        out.append(pos)
    return np.asarray(out, dtype=np.int64).reshape(np.asarray(ids).shape)


def pad_rows(T, pad=PAD, vocab=VOCAB, seed=0):
    """The six id patterns at ``T`` tokens (those that need more tokens than ``T`` has fall back to what fits): no pad,
    trailing pads, a pad in the middle, a pad first, pads only after the first token, every second token a pad."""
    rs = np.random.RandomState(1000 + 7 * T + seed)
    rows = rs.randint(2, vocab, (6, T))
    rows[1, (T + 1) // 2:] = pad
    rows[2, T // 2] = pad
    rows[3, 0] = pad
    rows[4, 1:] = pad
    rows[5, 1::2] = pad
    return rows.astype(np.int64)


def ids_with_pads(B, T, pad=PAD, vocab=VOCAB, seed=0):
    """[B, T]: the patterns of ``pad_rows`` in turn, starting with the full row."""
    rows = pad_rows(T, pad, vocab, seed)
    return np.stack([rows[b % 6] for b in range(B)])


def states(model, ids):
    return bo.states(model, ids)


def bias_table(model, T):
    """MPNet's bias as the table ``[heads, 2T-1]`` of ops.bert_encode, read off transformers' ``compute_position_bias``
    (entry d + T - 1 from (i, j) = (0, d) for d >= 0 and (-d, 0) for d < 0); None for the other classes."""
    if not hasattr(model.encoder, "relative_attention_bias"):
        return None
    with torch.no_grad():
        full = model.encoder.compute_position_bias(torch.zeros(1, T, 1))[0]           # [heads, T, T]
    left = torch.flip(full[:, 1:, 0], dims=(1,))                                      # d = -(T-1) .. -1
    return torch.cat([left, full[:, 0, :]], dim=1).contiguous()


def layer_params(model, T):
    """The arguments of ``ops.bert_encode`` for ``T`` tokens from a Bert / Roberta / MPNet model."""
    emb = model.embeddings
    mpnet = hasattr(model.encoder, "relative_attention_bias")
    layers = []
    for layer in model.encoder.layer:
        a, fo = layer.attention, layer.output
        q, k, v, o, ln1 = ((a.attn.q, a.attn.k, a.attn.v, a.attn.o, a.LayerNorm) if mpnet else
                           (a.self.query, a.self.key, a.self.value, a.output.dense, a.output.LayerNorm))
        layers.append({"W_qkv": torch.cat([q.weight, k.weight, v.weight], 0).detach().contiguous(),
                       "b_qkv": torch.cat([q.bias, k.bias, v.bias], 0).detach().contiguous(),
                       "W_o": o.weight, "b_o": o.bias, "ln1_g": ln1.weight, "ln1_b": ln1.bias,
                       "W_i": layer.intermediate.dense.weight, "b_i": layer.intermediate.dense.bias,
                       "W_f": fo.dense.weight, "b_f": fo.dense.bias, "ln2_g": fo.LayerNorm.weight,
                       "ln2_b": fo.LayerNorm.bias})
    pad = getattr(emb, "padding_idx", None) if type(model).__name__ != "BertModel" else None
    return dict(word_emb=emb.word_embeddings.weight, pos_emb=emb.position_embeddings.weight,
                type_emb=None if mpnet else emb.token_type_embeddings.weight, ln_g=emb.LayerNorm.weight,
                ln_b=emb.LayerNorm.bias, eps=float(model.config.layer_norm_eps), layers=layers,
                heads=int(model.config.num_attention_heads), I=int(model.config.intermediate_size), pad_id=pad,
                rel_bias=bias_table(model, T))


def encode(dev, model, ids, math=None, L=None, wrap=None):
    """``ops.bert_encode`` of ``model`` on ``ids`` (numpy) on ``dev``; ``wrap(tensor, role)`` may replace every device
    tensor (guarded copies)."""
    from gnnrag_amd import ops
    w = (lambda t, role: t) if wrap is None else wrap
    ids = np.asarray(ids)
    P = layer_params(model, ids.shape[1])
    layers = P["layers"] if L is None else P["layers"][:L]
    layers = [{k: w(v.detach().to(dev), "layers[%d].%s" % (i, k)) for k, v in d.items()} for i, d in enumerate(layers)]
    top = {k: (None if P[k] is None else w(P[k].detach().to(dev), k))
           for k in ("word_emb", "pos_emb", "type_emb", "ln_g", "ln_b", "rel_bias")}
    return ops.bert_encode(w(torch.from_numpy(ids).long().to(dev), "ids"), top["word_emb"], top["pos_emb"],
                           top["type_emb"], top["ln_g"], top["ln_b"], P["eps"], layers, P["heads"], I=P["I"], math=math,
                           pad_id=P["pad_id"], rel_bias=top["rel_bias"])


def attention64(qkv, B, T, heads, dh, rel_bias=None):
    """``bert_oracle.attention64`` with ``rel_bias[h, j - i + T - 1]`` added to the scaled scores."""
    H = heads * dh
    x = np.asarray(qkv, dtype=np.float64).reshape(B, T, 3, heads, dh)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    s = np.einsum("bihd,bjhd->bhij", q, k) / np.sqrt(dh)
    if rel_bias is not None:
        i, j = np.arange(T)[:, None], np.arange(T)[None, :]
        s = s + np.asarray(rel_bias, dtype=np.float64)[:, j - i + T - 1][None]
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhij,bjhd->bihd", p, v).reshape(B * T, H)
