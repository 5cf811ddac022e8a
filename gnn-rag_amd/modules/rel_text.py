"""Relation-text features on the MI355X (the relation-text branch).

With ``--relation_word_emb True`` (the reference's default, and what every documented command runs) ``get_rel_feature``
(``models/ReaRev/rearev.py:101-106``, ``models/NSM/nsm.py:103-105``) re-encodes the whole relation vocabulary on every
forward: ``instruction.question_emb`` over the frozen LM token states ``rel_features [R1, T, word_dim]``, then
``self_att_r`` (``AttnEncoder``, ``modules/query_update.py:46-61``) - twice in ReaRev, once per direction.  In training
the parameters move every step, so every step pays for it, forward and backward.

``patch_rel_feature(model)`` wraps ``get_rel_feature`` ON THE INSTANCE (the pattern of ``patch_instruction``; the reference
file is untouched).  The wrapped method makes one ``gnnrag_rel_text_pool`` call for all directions - under autograd through
``autograd.RelTextPoolFn``, whose backward is one ``gnnrag_rel_text_pool_backward`` call - when

* ``rel_texts`` is not None and ``lm != 'lstm'`` (the reference itself fails on that branch),
* ``instruction.question_emb`` is an ``nn.Linear`` with a bias and ``self_att_r.attn_linear`` an ``nn.Linear(D, 1)`` without,
* ``rel_features(_inv)``, the parameters and ``rel_texts`` are CUDA tensors (fp32, contiguous), the LM states do not ask for
  a gradient, and the shape is one the library takes.

Both directions take the mask of ``rel_texts`` (``rearev.py:105-106``); it is kept between calls, keyed by the identity and
version of ``rel_texts``.  Everything else - and ``GNNRAG_E_UNSUPPORTED`` from the library - runs the wrapped original
unchanged, and so does ``GNNRAG_HIP_REL_TEXT=0`` (read at every call; the default until the path is measured).
``install.cache_rel_features`` wraps on top of this: in evaluation the one computation per parameter version takes this
path.  Nothing is read on the host.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .. import _lib, ops

DEFAULT = "0"        # GNNRAG_HIP_REL_TEXT when unset (the rule and the measurement)
E_UNSUPPORTED = -2


def enabled() -> bool:
    """Whether the patched method uses the library (read at every call: the switch can change in-process)."""
    return os.environ.get("GNNRAG_HIP_REL_TEXT", DEFAULT) != "0"


def _on_gpu(t) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda


def _f32_cuda(t) -> bool:
    return _on_gpu(t) and t.dtype == torch.float32 and t.is_contiguous()


class _Patch:
    """State and wrapper of one patched model.  The wrapper is a BOUND METHOD of this object (not a closure)."""

    def __init__(self, model, directions: int):
        self.model, self.directions = model, directions
        self.orig = model.get_rel_feature
        self.mask_key, self.mask = None, None

    def operands(self):
        """(X_fwd, X_inv or None, W, b, a) when the call can run on the library, else None."""
        m = self.model
        texts = getattr(m, "rel_texts", None)
        if texts is None or getattr(m, "lm", None) == "lstm" or not _on_gpu(texts):
            return None
        ins, att = getattr(m, "instruction", None), getattr(m, "self_att_r", None)
        emb, lin = getattr(ins, "question_emb", None), getattr(att, "attn_linear", None)
        if not (isinstance(emb, nn.Linear) and isinstance(lin, nn.Linear)) or emb.bias is None or lin.bias is not None:
            return None
        if not hasattr(ins, "pad_val"):
            return None
        Xf = getattr(m, "rel_features", None)
        Xi = getattr(m, "rel_features_inv", None) if self.directions == 2 else None
        W, b, a = emb.weight, emb.bias, lin.weight
        xs = [Xf] if self.directions == 1 else [Xf, Xi]
        if not all(_f32_cuda(t) for t in xs + [W, b, a]) or any(x.requires_grad for x in xs) or Xf.dim() != 3:
            return None
        R, T, K = Xf.shape
        D = W.shape[0]
        if (tuple(W.shape) != (D, K) or tuple(a.shape) != (1, D) or tuple(texts.shape) != (R, T) or
                any(tuple(x.shape) != (R, T, K) or x.data_ptr() % 16 for x in xs) or
                not ops.rel_text_supported(R, T, K, D)):
            return None
        return Xf, Xi, W, b, a

    def token_mask(self):
        m = self.model
        texts, pad = m.rel_texts, m.instruction.pad_val
        key = (id(texts), texts._version, texts.data_ptr(), pad)
        if self.mask_key != key:
            self.mask, self.mask_key = (texts != pad).float(), key        # rearev.py:105
        return self.mask

    def get_rel_feature(self):
        if not enabled():
            return self.orig()
        args = self.operands()
        if args is None:
            return self.orig()
        Xf, Xi, W, b, a = args
        try:
            if torch.is_grad_enabled() and any(p.requires_grad for p in (W, b, a)):
                from ..autograd import RelTextPoolFn
                out_f, out_i = RelTextPoolFn.apply(Xf, Xi, self.token_mask(), W, b, a)
            else:
                out_f, out_i, _, _ = ops.rel_text_pool(Xf, Xi, self.token_mask(), W, b, a)
        except _lib.GnnragError as e:
            if getattr(e, "code", None) != E_UNSUPPORTED:
                raise
            return self.orig()
        return out_f if self.directions == 1 else (out_f, out_i)


def patch_rel_feature(model, directions=None):
    """Wraps ``get_rel_feature`` of a ReaRev- or NSM-like model (see the module docstring).  ``directions``: 2 = forward
    and inverse relation texts, a pair is returned (ReaRev); 1 = the forward texts only (NSM); None = 1 for a class
    named ``NSM``, else 2.  Idempotent; a model without ``get_rel_feature`` is returned as it is.  Apply it BEFORE
    ``install.cache_rel_features`` (``install.swap`` does): a method that is already the caching wrapper is left alone."""
    if getattr(model, "_gnnrag_rel_text_patched", False) or not hasattr(model, "get_rel_feature"):
        return model
    if getattr(model.get_rel_feature, "_gnnrag_cached", False):
        return model
    if directions is None:
        directions = 1 if type(model).__name__ == "NSM" else 2
    if directions not in (1, 2):
        raise ValueError("directions must be 1 or 2")
    model.get_rel_feature = _Patch(model, directions).get_rel_feature
    model._gnnrag_rel_text_patched = True
    return model
