"""Oracle of the BERT question-encoder tests: transformers' own ``BertModel`` in float64.

No weights are downloaded and no ``from_pretrained`` is called: a model is ``BertModel(BertConfig(...))`` with weights
drawn from ``np.random.RandomState(seed).standard_normal`` - the legacy generator's stream is frozen, so a seed regenerates
the weights anywhere (the fixture tests/golden/bert_encoder_ref.npz stores the seed, not the weights).  Matrices are scaled by
0.05, vectors by 0.1, LayerNorm weights are 1 + that.  ``make_model`` returns the fp32 module and its ``.double()`` copy; the
float64 module is the oracle everywhere, and the fp32 module's distance from it (``e_ref``) is the yardstick of the bounds.

Also holds the reference-shaped instruction module of the module tests (``make_instruction_standin``: the statements of
``BERTInstruction.encode_question``, bert_encoder.py:89-107, over the stand-in of tests/instruction_oracle.py)."""
import copy
import os

os.environ.setdefault("HF_HUB_OFFLINE", "1")        # before transformers is imported: nothing may reach for the hub

import numpy as np  # noqa: E402
import torch  # noqa: E402

MINILM = dict(H=384, heads=12, I=1536)              # all-MiniLM-L6-v2 (6 layers)
BERT_BASE = dict(H=768, heads=12, I=3072)


def config(H, heads, I, L, vocab=64, max_pos=32):
    from transformers import BertConfig
    return BertConfig(vocab_size=vocab, hidden_size=H, num_hidden_layers=L, num_attention_heads=heads,
                      intermediate_size=I, max_position_embeddings=max_pos, type_vocab_size=2, pad_token_id=0)


def make_model(cfg, seed):
    """(fp32 BertModel, float64 copy), both in eval mode, weights from RandomState(seed) in named_parameters order."""
    from transformers import BertModel
    model = BertModel(cfg)
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            w = rs.standard_normal(tuple(p.shape)) * (0.05 if p.dim() >= 2 else 0.1)
            if name.endswith("LayerNorm.weight"):
                w = 1.0 + w
            p.copy_(torch.from_numpy(w.astype(np.float32)))
    model.eval()
    return model, copy.deepcopy(model).double().eval()


def states(model, ids):
    """last_hidden_state of ``model`` on ``ids`` (numpy int64 [B,T]) as a numpy array of the model's dtype."""
    with torch.no_grad():
        return model(torch.from_numpy(np.asarray(ids, dtype=np.int64)))[0].numpy()


def rel_err(got, want):
    """max |got - want| relative to the oracle's largest entry."""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def bound(e_ref):
    """The issue's bound: 4 x the fp32 transformers module's own error against float64, at least 1e-6."""
    return max(4.0 * e_ref, 1e-6)


def layer_params(model):
    """The arguments of ``ops.bert_encode`` from a BertModel (the QKV weights stacked here, not by the code under test)."""
    emb = model.embeddings
    layers = []
    for layer in model.encoder.layer:
        s, ao, fo = layer.attention.self, layer.attention.output, layer.output
        layers.append({"W_qkv": torch.cat([s.query.weight, s.key.weight, s.value.weight], 0).detach().contiguous(),
                       "b_qkv": torch.cat([s.query.bias, s.key.bias, s.value.bias], 0).detach().contiguous(),
                       "W_o": ao.dense.weight, "b_o": ao.dense.bias, "ln1_g": ao.LayerNorm.weight,
                       "ln1_b": ao.LayerNorm.bias, "W_i": layer.intermediate.dense.weight,
                       "b_i": layer.intermediate.dense.bias, "W_f": fo.dense.weight, "b_f": fo.dense.bias,
                       "ln2_g": fo.LayerNorm.weight, "ln2_b": fo.LayerNorm.bias})
    return dict(word_emb=emb.word_embeddings.weight, pos_emb=emb.position_embeddings.weight,
                type_emb=emb.token_type_embeddings.weight, ln_g=emb.LayerNorm.weight, ln_b=emb.LayerNorm.bias,
                eps=float(model.config.layer_norm_eps), layers=layers, heads=int(model.config.num_attention_heads),
                I=int(model.config.intermediate_size))


def attention64(qkv, B, T, heads, dh):
    """softmax(q k^T / sqrt(dh)) v per (question, head) in float64; qkv [B*T, 3*heads*dh] -> [B*T, heads*dh]."""
    H = heads * dh
    x = np.asarray(qkv, dtype=np.float64).reshape(B, T, 3, heads, dh)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    s = np.einsum("bihd,bjhd->bhij", q, k) / np.sqrt(dh)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhij,bjhd->bihd", p, v).reshape(B * T, H)


def make_instruction_standin(lm, entity_dim, num_ins, pad_val, device="cpu"):
    """A module shaped like the reference's ``BERTInstruction``: ``node_encoder`` is ``lm``, ``question_emb`` maps its states
    to ``entity_dim``, the steps are those of the stand-in in tests/instruction_oracle.py."""
    import torch.nn as nn
    import instruction_oracle as io
    word_dim = int(lm.config.hidden_size)
    mod = io.make_standin(4, entity_dim, num_ins, num_word=pad_val)
    del mod.word_embedding
    mod.node_encoder = lm
    mod.question_emb = nn.Linear(word_dim, entity_dim)
    mod.pad_val = pad_val

    def encode_question(text):
        hidden = mod.node_encoder(text)[0]
        mod.query_hidden_emb = mod.question_emb(hidden)
        mod.query_node_emb = mod.question_emb(hidden.transpose(1, 0)[0].unsqueeze(1))
        mod.query_mask = (text != mod.pad_val).float()
        mod.lm_states = hidden
        return hidden, mod.query_node_emb

    mod.encode_question = encode_question
    return mod.to(device)
