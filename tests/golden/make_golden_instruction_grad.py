#!/usr/bin/env python
"""Generates tests/golden/instruction_grad_ref.npz from the LIVE reference's ``LSTMInstruction``
(``gnn/modules/question_encoding/lstm_encoder.py``, ``base_encoder.py:82-122``) under autograd, fp32 as shipped, both
dropouts 0: one encode, then ``num_ins`` = 3 chained ``get_instruction`` steps from a random ``r_in``, random upstream
gradients g_ins / g_attn through ``sum(ins * g_ins) + sum(attn * g_attn)``, and what torch's autograd derives for the token
states, the node state, r_in and every parameter of the steps.  D = 20, T = 5, B = 3; the last question is padding only.

    python tests/golden/make_golden_instruction_grad.py --reference <checkout of the reference>      (CPU)
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GNNRAG_REFERENCE"),
                    help="checkout of the reference (cmavro/GNN-RAG); default: $GNNRAG_REFERENCE")
    a = ap.parse_args()
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "gnn")):
        ap.error("--reference (or GNNRAG_REFERENCE) must name a checkout of the reference")
    sys.path.insert(0, os.path.join(a.reference, "gnn"))
    from modules.question_encoding import base_encoder, lstm_encoder
    # the reference's own start-up bug: LSTMInstruction calls BaseInstruction.__init__(args)
    # without the `constraint` argument - the same shim make_golden_lstm.py applies
    _init = base_encoder.BaseInstruction.__init__
    base_encoder.BaseInstruction.__init__ = lambda self, args, constraint=False: _init(self, args, constraint)
    torch.manual_seed(91)
    rng = np.random.default_rng(91)
    B, T, word_dim, D, vocab, n = 3, 5, 12, 20, 30, 3
    folder = tempfile.mkdtemp() + "/"
    with open(folder + "vocab.txt", "w") as f:
        f.write("\n".join("w%d" % i for i in range(vocab)) + "\n")
    args = dict(use_cuda=False, q_type="seq", num_step=n, lm_dropout=0.0, linear_dropout=0.0, lm_frozen=0,
                word_dim=word_dim, entity_dim=D, data_folder=folder, word2id="vocab.txt")
    enc = lstm_encoder.LSTMInstruction(args, nn.Embedding(vocab + 1, word_dim, padding_idx=vocab), vocab)
    enc.train()
    text = rng.integers(0, vocab, (B, T))
    text[1, 3:] = vocab
    text[2, :] = vocab                                           # a question of padding only
    q = torch.from_numpy(text).long()
    enc.init_reason(q)
    # leaves in place of the encoder's results: the gradients of the steps alone
    hidden = enc.query_hidden_emb.detach().clone().requires_grad_(True)
    node = enc.query_node_emb.detach().clone().requires_grad_(True)              # [B, 1, D]
    enc.query_hidden_emb, enc.query_node_emb = hidden, node
    r_in = torch.tanh(torch.randn(B, D)).requires_grad_(True)
    g_ins, g_attn = torch.randn(n, B, D), torch.randn(n, B, T)
    r, ins, attn = r_in, [], []
    for s in range(n):
        r, at = enc.get_instruction(r, step=s)
        ins.append(r)
        attn.append(at)
    ins, attn = torch.stack(ins), torch.stack(attn).reshape(n, B, T)
    ((ins * g_ins).sum() + (attn * g_attn).sum()).backward()
    P = dict(enc.named_parameters())
    out = {"hidden": hidden.detach().numpy(), "node": node.detach().numpy().reshape(B, D),
           "mask": enc.query_mask.numpy().astype(np.float32), "r_in": r_in.detach().numpy(), "g_ins": g_ins.numpy(),
           "g_attn": g_attn.numpy(), "ins": ins.detach().numpy(), "attn": attn.detach().numpy(),
           "dhidden": hidden.grad.numpy(), "dnode": node.grad.numpy().reshape(B, D), "dr_in": r_in.grad.numpy()}
    for name, key in [("cq_linear.weight", "W_cq"), ("cq_linear.bias", "b_cq"), ("ca_linear.weight", "w_ca"),
                      ("ca_linear.bias", "b_ca")] + \
            [("question_linear%d.%s" % (s, k), "%s_q%d" % (v, s)) for s in range(n) for k, v in (("weight", "W"), ("bias", "b"))]:
        out[key] = P[name].detach().numpy()
        out["d" + key] = P[name].grad.numpy()
    np.savez_compressed(os.path.join(HERE, "instruction_grad_ref.npz"), **out)
    print("wrote instruction_grad_ref.npz:", {k: v.shape for k, v in out.items()})
    print("db_ca as torch's fp32 autograd leaves it:", out["db_ca"])


if __name__ == "__main__":
    main()
