"""The loss and the batch metrics of a training forward on the MI355X.

What follows the last ``dist`` of ``ReaRev.forward`` (``models/ReaRev/rearev.py:227-243``) and ``NSM.forward``
(``models/NSM/nsm.py:242-250``):

* ``calc_loss_label`` -> ``get_loss`` -> ``get_loss_kl`` (``base_model.py:193-215``): about ten torch launches forward and as
  many backward;
* ``get_eval_metric`` -> ``calc_h1`` + ``calc_f1_new`` (``base_model.py:249-298``), which ``Trainer_KBQA.train_epoch`` runs on
  every training step (``train_model.py:222``): per question with a hit one ``.item()``, four ``.tolist()`` of N-vectors, a
  Python loop over the N slots and a Python sort.

``patch_loss_metrics(model)`` wraps both methods ON THE INSTANCE (the pattern of ``patch_instruction`` and
``patch_rel_feature``; the reference files are untouched).  With ``GNNRAG_HIP_LOSS_METRICS=1`` (read at every call, default
off):

* ``calc_loss_label(curr_dist, teacher_dist, label_valid)`` goes through ``autograd.KLLossFn`` (``gnnrag_kl_loss_train`` /
  ``gnnrag_kl_loss_backward``) when ``loss_type == 'kl'``, the three tensors are fp32, contiguous and on the GPU, and
  ``teacher_dist`` does not ask for a gradient (NSM's backward loss may pass one that does: that call stays on torch);
* ``get_eval_metric(pred_dist, answer_dist)`` is one ``gnnrag_train_metrics`` call over ``self.seed_entities``,
  ``self.local_entity``, ``self.num_entity`` and ``self.eps`` - what ``calc_f1_new`` reads - and returns ``(h1, f1)`` as device
  float tensors [B]; the forward's own ``.tolist()`` pair is then the only wait.

Everything else - and ``GNNRAG_E_UNSUPPORTED`` from the library (N > 16384) - runs the wrapped original unchanged.

Limitation: ``f1_and_hits`` counts a retrieved candidate as correct by its entity id (``c in answers``), the kernel by the
slot's own answer flag.  The two agree whenever a question's non-pad entity ids are distinct, which the batch builder
guarantees: ``candidate_entities[q, local] = global`` is filled from the keys of the dict ``g2l``
(``dataset_load.py:249-257``, built by ``_add_entity_to_map``, ``:562-575``).
"""
from __future__ import annotations

import os

import torch

from .. import _lib, ops

DEFAULT = "0"        # GNNRAG_HIP_LOSS_METRICS when unset (the rule and the measurement)
E_UNSUPPORTED = -2


def enabled() -> bool:
    """Whether the patched methods use the library (read at every call: the switch can change in-process)."""
    return os.environ.get("GNNRAG_HIP_LOSS_METRICS", DEFAULT) == "1"


def _f32_cuda(t) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


class _Patch:
    """State and wrappers of one patched model.  The wrappers are BOUND METHODS of this object (not closures), so a
    ``copy.deepcopy`` of a patched model gets wrappers that belong to the copy."""

    def __init__(self, model):
        self.model = model
        self.orig_loss, self.orig_metric = model.calc_loss_label, model.get_eval_metric

    def loss_eligible(self, curr_dist, teacher_dist, label_valid) -> bool:
        if getattr(self.model, "loss_type", None) != "kl":
            return False
        if not (_f32_cuda(curr_dist) and _f32_cuda(teacher_dist) and _f32_cuda(label_valid)):
            return False
        if teacher_dist.requires_grad or label_valid.requires_grad or curr_dist.dim() != 2:
            return False
        B, N = curr_dist.shape
        return B > 0 and N > 0 and tuple(teacher_dist.shape) == (B, N) and label_valid.numel() == B

    def calc_loss_label(self, curr_dist, teacher_dist, label_valid):
        if not enabled() or not self.loss_eligible(curr_dist, teacher_dist, label_valid):
            return self.orig_loss(curr_dist=curr_dist, teacher_dist=teacher_dist, label_valid=label_valid)
        if torch.is_grad_enabled() and curr_dist.requires_grad:
            from ..autograd import KLLossFn
            return KLLossFn.apply(curr_dist, teacher_dist, label_valid)
        return ops.kl_loss_train(curr_dist.detach(), teacher_dist, label_valid)[0].view(())

    def metric_operands(self, pred_dist, answer_dist):
        """(seed, local_entity, pad_id, eps) when the call can run on the library, else None."""
        m = self.model
        seed, ent = getattr(m, "seed_entities", None), getattr(m, "local_entity", None)
        if not (_f32_cuda(pred_dist) and _f32_cuda(answer_dist) and _f32_cuda(seed)) or pred_dist.dim() != 2:
            return None
        if not (isinstance(ent, torch.Tensor) and ent.is_cuda and ent.dtype == torch.int64 and ent.is_contiguous()):
            return None
        B, N = pred_dist.shape
        if any(tuple(t.shape) != (B, N) for t in (answer_dist, seed, ent)) or not ops.train_metrics_supported(B, N):
            return None
        return seed.detach(), ent, int(m.num_entity), float(m.eps)

    def get_eval_metric(self, pred_dist, answer_dist):
        args = self.metric_operands(pred_dist, answer_dist) if enabled() else None
        if args is None:
            return self.orig_metric(pred_dist, answer_dist)
        try:
            _, h1, f1, _ = ops.train_metrics(pred_dist.detach(), answer_dist.detach(), *args)
        except _lib.GnnragError as e:
            if getattr(e, "code", None) != E_UNSUPPORTED:
                raise
            return self.orig_metric(pred_dist, answer_dist)
        return h1, f1


def patch_loss_metrics(model):
    """Wraps ``calc_loss_label`` and ``get_eval_metric`` of a ReaRev- or NSM-like model (see the module docstring).
    Idempotent; a model without both methods is returned as it is."""
    if getattr(model, "_gnnrag_loss_metrics_patched", False):
        return model
    if not (hasattr(model, "calc_loss_label") and hasattr(model, "get_eval_metric")):
        return model
    p = _Patch(model)
    model.calc_loss_label, model.get_eval_metric = p.calc_loss_label, p.get_eval_metric
    model._gnnrag_loss_metrics_patched = True
    return model
