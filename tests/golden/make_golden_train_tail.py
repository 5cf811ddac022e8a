#!/usr/bin/env python
"""Generates tests/golden/train_tail_ref.npz from the LIVE reference: ``BaseModel.get_loss`` under
``ReaRev.calc_loss_label`` (``gnn/models/ReaRev/rearev.py:156-160``, ``gnn/models/base_model.py:193-215``) with autograd's
``d_pred``, and ``BaseModel.calc_h1`` / ``calc_f1_new`` / ``f1_and_hits`` (``base_model.py:217-298``), called as plain
functions on a stand-in object that holds what they read: ``loss_type='kl'``, ``kld_loss``, ``seed_entities``,
``local_entity``, ``num_entity``, ``eps``, ``device``.

Recorded per case of ``train_tail_oracle.FIXTURE_CASES``: the inputs; the fp32 loss and ``d_pred`` (for the recorded upstream
gradient g); ``torch.max(pred, 1)[1]``, H@1 and the gated F1 of ``get_eval_metric``; and - from a second ``calc_f1_new`` call
with every question let through the H@1 gate - what ``f1_and_hits`` was given and returned per question: the lengths of its
answer and candidate lists, precision, recall and F1.  Also the reference's own fp32 error of loss and d_pred against the
float64 oracle (tests/train_tail_oracle.py), relative to |loss| and to the largest |d_pred|; the recorder insists on 2e-6.

    python tests/golden/make_golden_train_tail.py <the reference's gnn directory>        (build container only, CPU)
"""
import functools
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import train_tail_oracle as to  # noqa: E402

TOL_REFERENCE = 2e-6


def stand_in(BaseModel, c):
    m = types.SimpleNamespace(loss_type="kl", kld_loss=nn.KLDivLoss(reduction="none"), device=torch.device("cpu"),
                              seed_entities=torch.from_numpy(c["seed"]), local_entity=torch.from_numpy(c["local_entity"]),
                              num_entity=c["pad_id"], eps=c["eps"], calls=[])
    for name in ("get_loss_kl", "get_loss", "calc_h1", "calc_f1_new"):
        setattr(m, name, functools.partial(getattr(BaseModel, name), m))

    def f1_and_hits(answers, candidate2prob, eps=0.5):
        got = BaseModel.f1_and_hits(m, answers, candidate2prob, eps)
        m.calls.append((len(answers), len(candidate2prob)) + tuple(got))
        return got

    m.f1_and_hits = f1_and_hits
    return m


def main():
    sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.environ["GNNRAG_REFERENCE_GNN"])
    from models.base_model import BaseModel
    from models.ReaRev.rearev import ReaRev
    out = {}
    for tag, (B, N, seed, eps) in to.FIXTURE_CASES.items():
        c = to.case(B, N, seed, eps)
        m = stand_in(BaseModel, c)
        pred = torch.from_numpy(c["pred"]).requires_grad_(True)
        answer, valid = torch.from_numpy(c["answer"]), torch.from_numpy(c["label_valid"])
        loss = ReaRev.calc_loss_label(m, curr_dist=pred, teacher_dist=torch.from_numpy(c["teacher"]), label_valid=valid)
        (d_pred,) = torch.autograd.grad(loss * float(c["g"]), pred)
        h1, f1 = BaseModel.get_eval_metric(m, pred.detach(), answer)
        gated_calls = len(m.calls)
        assert gated_calls == int(h1.sum().item())
        BaseModel.calc_f1_new(m, pred.detach(), answer, torch.ones(B))
        raw = np.array(m.calls[gated_calls:], dtype=np.float64)          # n_ans, kept, precision, recall, f1, hits
        assert raw.shape == (B, 6)
        want_loss, want_d, _, _ = to.loss_and_grad(c["pred"], c["teacher"], c["label_valid"], c["g"])
        err_loss = abs(float(loss) - want_loss) / abs(want_loss)
        err_d = float(np.abs(d_pred.numpy() - want_d).max() / np.abs(want_d).max())
        assert err_loss <= TOL_REFERENCE and err_d <= TOL_REFERENCE, (tag, err_loss, err_d)
        rec = dict(pred=c["pred"], answer=c["answer"], teacher=c["teacher"], label_valid=c["label_valid"], seed=c["seed"],
                   local_entity=c["local_entity"], pad_id=np.int64(c["pad_id"]), eps=np.float64(c["eps"]), g=c["g"],
                   loss=loss.detach().numpy(), d_pred=d_pred.numpy(), argmax=torch.max(pred, dim=1)[1].numpy(),
                   h1=h1.numpy(), f1=f1.numpy(), n_ans=raw[:, 0].astype(np.int32), kept=raw[:, 1].astype(np.int32),
                   precision=raw[:, 2], recall=raw[:, 3], f1_raw=raw[:, 4], err_loss=np.float64(err_loss),
                   err_d_pred=np.float64(err_d))
        out.update({"%s.%s" % (tag, k): v for k, v in rec.items()})
        print(tag, (B, N, eps), "loss %.6f err %.2e, d_pred err %.2e, h1 %s, f1 %s" % (float(loss), err_loss, err_d,
                                                                                    h1.tolist(), f1.tolist()))
    path = os.path.join(HERE, "train_tail_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote train_tail_ref.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
