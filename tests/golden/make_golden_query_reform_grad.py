#!/usr/bin/env python
"""Generates tests/golden/query_reform_grad_ref.npz from the LIVE reference's ``QueryReform``
(``gnn/modules/query_update.py:18-44``) under autograd, fp32 as shipped: n = 3 reforms on one node state and one seed
indicator (B, N, D = 3, 7, 20; question 1 has no seed, question 0 two seeds, one of them in slot N - 1), random upstream
gradients G through ``sum_j sum(out_j * G_j)``, and what torch's autograd derives for every instruction, every ``Fusion``
weight and - summed over the reforms - the node state.

    python tests/golden/make_golden_query_reform_grad.py --reference <checkout of the reference>      (CPU)
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GNNRAG_REFERENCE"),
                    help="checkout of the reference (cmavro/GNN-RAG); default: $GNNRAG_REFERENCE")
    a = ap.parse_args()
    if not a.reference or not os.path.isdir(os.path.join(a.reference, "gnn")):
        ap.error("--reference (or GNNRAG_REFERENCE) must name a checkout of the reference")
    sys.path.insert(0, os.path.join(a.reference, "gnn"))
    from modules.query_update import QueryReform
    torch.manual_seed(92)
    B, N, D, n = 3, 7, 20, 3
    seed = torch.zeros(B, N)
    seed[0, 2] = 1.0
    seed[0, N - 1] = 1.0
    seed[2, 4] = 1.0                                             # question 1 has no seed
    ent = torch.randn(B, N, D, requires_grad=True)
    mask = torch.ones(B, N)
    out = {"seed": seed.numpy(), "ent": ent.detach().numpy()}
    loss = 0.0
    mods, qs = [], []
    for j in range(n):
        m = QueryReform(D)
        q = torch.tanh(torch.randn(B, D)).requires_grad_(True)
        G = torch.randn(B, D)
        o = m(q, ent, seed, mask)
        loss = loss + (o * G).sum()
        mods.append(m), qs.append(q)
        out["q%d" % j], out["G%d" % j], out["out%d" % j] = q.detach().numpy(), G.numpy(), o.detach().numpy()
        out["W_r%d" % j], out["W_g%d" % j] = m.fusion.r.weight.detach().numpy(), m.fusion.g.weight.detach().numpy()
    loss.backward()
    for j, (m, q) in enumerate(zip(mods, qs)):
        assert m.q_ent_attn.weight.grad is None                  # the attention does not enter the returned value
        out["dq%d" % j], out["dW_r%d" % j] = q.grad.numpy(), m.fusion.r.weight.grad.numpy()
        out["dW_g%d" % j] = m.fusion.g.weight.grad.numpy()
    out["d_ent"] = ent.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "query_reform_grad_ref.npz"), **out)
    print("wrote query_reform_grad_ref.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
