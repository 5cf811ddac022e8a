#!/usr/bin/env python
"""Generates tests/golden/lm_variants_ref.npz from the LIVE reference's ``BERTInstruction``
(``gnn/modules/question_encoding/bert_encoder.py``) constructed as ``--lm roberta`` and ``--lm sbert2`` construct it:
``BERTInstruction(args, None, 64, "roberta")`` and ``(..., "sbert2")``.  As in make_golden_bert_encoder.py the two names the
reference's module resolves through the hub - ``AutoTokenizer`` and ``AutoModel`` - are replaced in that module's namespace
BEFORE the constructor runs: the tokenizer by an object that only knows its pad token (id 1, as roberta-base and
all-mpnet-base-v2 have it), the model by a ``RobertaModel`` / ``MPNetModel`` with seeded random weights
(tests/lm_variants_oracle.py: ``make_model``).  The reference hard-codes ``word_dim = 768`` for both, so the models are 768
wide (12 heads of 64, intermediate 1536, 2 layers, vocabulary 50).  Nothing is downloaded.

Recorded per encoder (keys ``roberta.*`` / ``sbert2.*``): the config numbers and the seed (the LM weights are regenerated
from them, not stored), the small non-LM parameters, ``q_input`` (3 questions x 9 tokens: one full, one padded from position
5, one of padding only after <s>), the LM states of the reference's fp32 run, their error against the float64 copy of the
same model (``lm.e_ref``), and what the module's ``forward`` derives: ``query_hidden_emb``, ``instructions`` and ``attn``.

    python tests/golden/make_golden_lm_variants.py [REFERENCE/gnn]          (CPU; default: $GNNRAG_REFERENCE_GNN)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import bert_oracle as bo  # noqa: E402  (sets HF_HUB_OFFLINE=1 before transformers is imported)
import lm_variants_oracle as lo  # noqa: E402

SEED, L, VOCAB, MAX_POS, ENTITY_DIM, NUM_STEP, PAD, CLS = 2025, 2, 50, 16, 32, 3, 1, 0
SHAPE = dict(H=768, heads=12, I=1536)
LMS = {"roberta": "roberta", "sbert2": "mpnet"}          # the reference's --lm name -> the oracle's class name


def record(bert_encoder, lm_name, arch, seed):
    cfg = lo.config(arch, L=L, vocab=VOCAB, max_pos=MAX_POS, pad=PAD, **SHAPE)
    lm, lm64 = lo.make_model(arch, cfg, seed)

    class Tokenizer:
        pad_token = "<pad>"

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
    torch.manual_seed(seed)
    args = dict(use_cuda=False, q_type="seq", num_step=NUM_STEP, lm_dropout=0.0, linear_dropout=0.0, lm_frozen=1,
                entity_dim=ENTITY_DIM, word_dim=768, data_folder="")
    enc = bert_encoder.BERTInstruction(args, None, 64, lm_name)
    enc.eval()
    assert enc.node_encoder is lm and enc.pad_val == PAD and enc.word_dim == cfg.hidden_size

    rng = np.random.RandomState(seed + 1)
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
           "cfg.vocab": VOCAB, "cfg.max_pos": MAX_POS, "cfg.seed": seed, "cfg.entity_dim": ENTITY_DIM,
           "cfg.num_step": NUM_STEP, "cfg.pad_val": PAD,
           "q_input": q, "lm.states": states.numpy(), "lm.e_ref": np.float64(bo.rel_err(states.numpy(), states64)),
           "query_hidden_emb": enc.query_hidden_emb.numpy(), "query_node_emb": enc.query_node_emb.numpy(),
           "instructions": np.stack([i.numpy() for i in instructions]), "attn": np.stack([a.numpy() for a in attn])}
    for k, v in enc.state_dict().items():
        if not k.startswith("node_encoder."):
            out["param." + k] = v.numpy()
    return {lm_name + "." + k: v for k, v in out.items()}


def main():
    sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.environ["GNNRAG_REFERENCE_GNN"])
    from modules.question_encoding import bert_encoder
    out = {}
    for n, (lm_name, arch) in enumerate(LMS.items()):
        out.update(record(bert_encoder, lm_name, arch, SEED + 10 * n))
    path = os.path.join(HERE, "lm_variants_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote lm_variants_ref.npz: %d bytes" % os.path.getsize(path),
          {k: (np.shape(v) if np.ndim(v) else float(v)) for k, v in out.items() if ".param." not in k and ".cfg." not in k})


if __name__ == "__main__":
    main()
