#!/usr/bin/env python
"""Generates tests/golden/bert_encoder_ref.npz from the LIVE reference's ``BERTInstruction``
(``gnn/modules/question_encoding/bert_encoder.py``) constructed as ``--lm sbert`` constructs it: ``BERTInstruction(args, None,
64, "sbert")``.  The two names the reference's module resolves through the hub - ``AutoTokenizer`` and ``AutoModel`` - are
replaced in that module's namespace BEFORE the constructor runs: the tokenizer by an object that only knows its pad token,
the model by a MiniLM-shaped ``BertModel`` with seeded random weights (tests/bert_oracle.py: ``make_model``).  Nothing is
downloaded.

Recorded: the config numbers and the seed (the LM weights are regenerated from them, not stored), the small non-LM
parameters, ``q_input`` (3 questions x 9 tokens: one full, one padded from position 5, one of padding only after [CLS]), the
LM states of the reference's fp32 run, their error against the float64 copy of the same model (``lm.e_ref``), and what the
module's ``forward`` derives: ``query_hidden_emb``, ``instructions`` and ``attn``.

    python tests/golden/make_golden_bert_encoder.py          (build container only, CPU)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference/gnn")

import bert_oracle as bo  # noqa: E402  (sets HF_HUB_OFFLINE=1 before transformers is imported)

SEED, L, VOCAB, MAX_POS, ENTITY_DIM, NUM_STEP, PAD, CLS = 2024, 2, 64, 16, 32, 3, 0, 1


def main():
    from modules.question_encoding import bert_encoder
    cfg = bo.config(L=L, vocab=VOCAB, max_pos=MAX_POS, **bo.MINILM)
    lm, lm64 = bo.make_model(cfg, SEED)

    class Tokenizer:
        pad_token = "[PAD]"

        @staticmethod
        def from_pretrained(name):
            return Tokenizer()

        def convert_tokens_to_ids(self, token):
            assert token == self.pad_token
            return PAD

    class Model:
        @staticmethod
        def from_pretrained(name):
            return lm

    bert_encoder.AutoTokenizer, bert_encoder.AutoModel = Tokenizer, Model
    torch.manual_seed(SEED)
    args = dict(use_cuda=False, q_type="seq", num_step=NUM_STEP, lm_dropout=0.0, linear_dropout=0.0, lm_frozen=1,
                entity_dim=ENTITY_DIM, word_dim=384, data_folder="")
    enc = bert_encoder.BERTInstruction(args, None, 64, "sbert")
    enc.eval()
    assert enc.node_encoder is lm and enc.pad_val == PAD and enc.word_dim == cfg.hidden_size

    rng = np.random.RandomState(SEED + 1)
    q = rng.randint(2, VOCAB, (3, 9))
    q[:, 0] = CLS
    q[1, 5:] = PAD
    q[2, 1:] = PAD
    qt = torch.from_numpy(q).long()
    with torch.no_grad():
        states = enc.encode_question(qt, store=False)
        instructions, attn = enc(qt)
        states64 = lm64(qt)[0].numpy()
    out = {"cfg.H": cfg.hidden_size, "cfg.heads": cfg.num_attention_heads, "cfg.I": cfg.intermediate_size, "cfg.L": L,
           "cfg.vocab": VOCAB, "cfg.max_pos": MAX_POS, "cfg.seed": SEED, "cfg.entity_dim": ENTITY_DIM,
           "cfg.num_step": NUM_STEP, "cfg.pad_val": PAD,
           "q_input": q, "lm.states": states.numpy(), "lm.e_ref": np.float64(bo.rel_err(states.numpy(), states64)),
           "query_hidden_emb": enc.query_hidden_emb.numpy(), "query_node_emb": enc.query_node_emb.numpy(),
           "instructions": np.stack([i.numpy() for i in instructions]), "attn": np.stack([a.numpy() for a in attn])}
    for k, v in enc.state_dict().items():
        if not k.startswith("node_encoder."):
            out["param." + k] = v.numpy()
    path = os.path.join(HERE, "bert_encoder_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote bert_encoder_ref.npz: %d bytes, e_ref %.3g" % (os.path.getsize(path), out["lm.e_ref"]),
          {k: np.shape(v) for k, v in out.items() if not k.startswith(("param.", "cfg."))})


if __name__ == "__main__":
    main()
