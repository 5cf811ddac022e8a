"""Drop-in for the reference's ``modules/query_update.py``: the instruction
update between two ReaRev iterations (``rearev.py:217-221``).

``QueryReform.forward`` in the reference (``query_update.py:26-44``) first computes an attention over
all N node states (``:36-38``: a [B,N,D] product, a softmax over N and a second [B,N,D] product - three
passes over the node state plus two [B,N,D] temporaries) and then does not use it: the value it returns
is ``fusion(q_node, seed_retrieve)`` (``:40,44``).  Here only that is computed, and ``seed_retrieve`` reads
just the seed rows instead of streaming the node state through a bmm - retrieval and Fusion in ONE launch
(``gnnrag_query_reform``; ``gnnrag_seed_retrieve`` + the torch Fusion for shapes it does not take).  Same
classes, constructors, parameter names (``q_ent_attn`` is kept: released checkpoints hold it) and
return values.

Under autograd the seed retrieval is the reference's ``torch.bmm`` followed by the torch ``Fusion`` - unless
``GNNRAG_HIP_QUERY_REFORM_TRAIN=1`` (read at every call, default off).  With the switch set an
eligible call goes through ``autograd.QueryReformFn`` (``gnnrag_query_reform_train`` / ``gnnrag_query_reform_backward``):
CUDA fp32 tensors, ``q_node`` [B,D], ``ent_emb`` [B,N,D] contiguous in its last dimension (read in place by its row
stride), no ``Fusion`` biases, a shape the library takes, ``seed_info`` not requiring grad.  Anything else - CPU tensors
among it - is the torch form, bit for bit.  ``q_ent_attn`` keeps receiving no gradient, as in the reference.

``bind_reforms(model)`` (called by ``install.swap``) makes the reforms of one iteration (``rearev.py:217-221``) ONE call: the
n reforms are independent of each other - they share the node state and the seeds, each has its own instruction and
``Fusion`` weights.  When reform 0 is called with the very ``model.instruction.instructions[0].squeeze(1)`` (same storage,
shape, strides, ``_version``) and every sibling is eligible, one ``QueryReformFn`` call computes all n outputs - one forward
launch, one backward, ONE dense node-state gradient instead of n.  Outputs 1..n-1 are kept under a key (identity and
``_version`` of ``ent_emb`` and ``seed_info``; storage, shape, strides and ``_version`` of ``instructions[j]``); reform j's call
hands its output out when its arguments match the key and makes a single (n = 1) call otherwise.  Kept outputs are dropped
at the next reform-0 call.  Nothing is read on the host.  An unbound module always makes single calls; the bound state
lives in a plain object per model, so a ``copy.deepcopy`` of the model binds to itself."""
from __future__ import annotations

import copy
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import autograd, ops

TRAIN_DEFAULT = "0"  # GNNRAG_HIP_QUERY_REFORM_TRAIN when unset: off until measured


def train_enabled() -> bool:
    """Whether an eligible call under autograd runs on the library (read at every call)."""
    return os.environ.get("GNNRAG_HIP_QUERY_REFORM_TRAIN", TRAIN_DEFAULT) != "0"


def _f32_cuda(t) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32


def _view_key(t):
    """What makes two tensors the same values AND the same place in the graph without reading them: storage, offset,
    shape, strides, version counter, and whether / how autograd tracks them."""
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t._version, t.requires_grad, type(t.grad_fn).__name__)


class _Bound:
    """The reforms of one model, its instruction module, and the kept outputs of the last all-reforms call.  A plain
    object (nothing in it is registered as a submodule); a deep copy refers to the COPIED modules and keeps no outputs."""

    def __init__(self, reforms, instruction):
        self.reforms, self.instruction, self.kept = list(reforms), instruction, None

    def __deepcopy__(self, memo):
        new = _Bound.__new__(_Bound)
        memo[id(self)] = new
        new.reforms = [copy.deepcopy(m, memo) for m in self.reforms]
        new.instruction = copy.deepcopy(self.instruction, memo)
        new.kept = None
        return new


def bind_reforms(model):
    """Gives every ``model.reform{j}`` (rearev.py:46-47) its index, its siblings and a handle on ``model.instruction``, so
    that an iteration's reforms can be one call (see the module docstring).  Idempotent; rebinding replaces the state."""
    reforms, j = [], 0
    while isinstance(getattr(model, "reform" + str(j), None), QueryReform):
        reforms.append(getattr(model, "reform" + str(j)))
        j += 1
    instruction = getattr(model, "instruction", None)
    if not reforms or instruction is None or getattr(model, "reform" + str(j), None) is not None:
        return model
    bound = _Bound(reforms, instruction)
    for k, m in enumerate(reforms):
        # past nn.Module.__setattr__: the siblings and the instruction module must not become submodules of a reform
        object.__setattr__(m, "_qr_bound", bound)
        object.__setattr__(m, "_qr_index", k)
    return model


class Fusion(nn.Module):
    """Gated mix of an instruction x with retrieved evidence y (reference: query_update.py:6-16)."""

    def __init__(self, d_hid):
        super().__init__()
        self.r = nn.Linear(d_hid * 3, d_hid, bias=False)
        self.g = nn.Linear(d_hid * 3, d_hid, bias=False)

    def forward(self, x, y):
        feats = torch.cat([x, y, x - y], dim=-1)
        gate = torch.sigmoid(self.g(feats))
        return gate * self.r(feats) + (1 - gate) * x


class QueryReform(nn.Module):
    """Instruction update from the seeds' node states (reference: query_update.py:18-44)."""

    def __init__(self, h_dim):
        super().__init__()
        self.fusion = Fusion(h_dim)
        self.q_ent_attn = nn.Linear(h_dim, h_dim)      # unused by the returned value; state_dict parity

    def _eligible(self, q_node, ent_emb, seed_info) -> bool:
        r, g = self.fusion.r, self.fusion.g
        if not (_f32_cuda(q_node) and _f32_cuda(ent_emb) and _f32_cuda(seed_info) and q_node.dim() == 2
                and ent_emb.dim() == 3 and seed_info.dim() == 2 and not seed_info.requires_grad):
            return False
        B, D = q_node.shape
        N = seed_info.shape[1]
        return (B > 0 and N > 0 and seed_info.shape[0] == B and tuple(ent_emb.shape) == (B, N, D) and ent_emb.stride(2) == 1
                and r.bias is None and g.bias is None and _f32_cuda(r.weight) and _f32_cuda(g.weight)
                and tuple(r.weight.shape) == (D, 3 * D) and tuple(g.weight.shape) == (D, 3 * D)
                and ops.query_reform_backward_supported(D, 1))

    def _train_forward(self, q_node, ent_emb, seed_info):
        """The call on ``QueryReformFn`` (None: not eligible).  Bound: reform 0 computes every reform of the iteration,
        reform j > 0 picks its output up when its arguments are the ones that call saw."""
        if not self._eligible(q_node, ent_emb, seed_info):
            return None
        bound, j = self.__dict__.get("_qr_bound"), self.__dict__.get("_qr_index", 0)
        if bound is not None and j == 0:
            bound.kept = None
            n = len(bound.reforms)
            ins = getattr(bound.instruction, "instructions", None)
            if n > 1 and isinstance(ins, list) and len(ins) >= n and ops.query_reform_backward_supported(q_node.shape[1], n) \
                    and all(isinstance(t, torch.Tensor) and t.dim() == 3 and t.shape[1] == 1 for t in ins[:n]):
                qs = [t.squeeze(1) for t in ins[:n]]
                if _view_key(qs[0]) == _view_key(q_node) and all(
                        m._eligible(q, ent_emb, seed_info) for m, q in zip(bound.reforms[1:], qs[1:])):
                    outs = autograd.QueryReformFn.apply(seed_info, ent_emb, *qs,
                                                        *[m.fusion.r.weight for m in bound.reforms],
                                                        *[m.fusion.g.weight for m in bound.reforms])
                    bound.kept = {"ent": ent_emb, "ent_v": ent_emb._version, "seed": seed_info,
                                  "seed_v": seed_info._version, "q": [_view_key(q) for q in qs], "out": list(outs)}
                    return outs[0]
        elif bound is not None:
            kept = bound.kept
            if (kept is not None and j < len(kept["out"]) and kept["out"][j] is not None and kept["ent"] is ent_emb
                    and kept["ent_v"] == ent_emb._version and kept["seed"] is seed_info
                    and kept["seed_v"] == seed_info._version and kept["q"][j] == _view_key(q_node)):
                out, kept["out"][j] = kept["out"][j], None
                return out
        return autograd.QueryReformFn.apply(seed_info, ent_emb, q_node, self.fusion.r.weight, self.fusion.g.weight)[0]

    def forward(self, q_node, ent_emb, seed_info, ent_mask):
        if torch.is_grad_enabled():
            if train_enabled():
                out = self._train_forward(q_node, ent_emb, seed_info)
                if out is not None:
                    return out
            seed_retrieve = torch.bmm(seed_info.unsqueeze(1), ent_emb).squeeze(1)       # :40 (autograd form)
        else:
            base = getattr(ent_emb, "_gnnrag_padded", None)        # node state kept zero-padded by ReasonGNNLayer
            D = ent_emb.shape[-1]
            r, g = self.fusion.r, self.fusion.g
            if (q_node.dim() == 2 and q_node.shape[-1] == D and D <= 4096 and r.bias is None and g.bias is None
                    and r.weight.dtype == torch.float32 and g.weight.dtype == torch.float32):
                # retrieval + Fusion (:40,44 with :6-16) in one launch: ~11 small torch launches per call otherwise
                return ops.query_reform(q_node.detach().float(), seed_info.float(), base if base is not None else ent_emb.float(),
                                        r.weight.detach(), g.weight.detach())
            if base is not None:
                seed_retrieve = ops.seed_retrieve(seed_info.float(), base)[:, : ent_emb.shape[-1]]
            else:
                seed_retrieve = ops.seed_retrieve(seed_info.float(), ent_emb.float())   # raises on CPU tensors
        return self.fusion(q_node, seed_retrieve)                                       # :44


class AttnEncoder(nn.Module):
    """Masked attention pooling over a sequence (reference: query_update.py:46-62)."""

    def __init__(self, d_hid):
        super().__init__()
        self.attn_linear = nn.Linear(d_hid, 1, bias=False)

    def forward(self, x, x_mask):
        logits = self.attn_linear(x) - (1 - x_mask.unsqueeze(2)) * 1e8
        return (x * F.softmax(logits, dim=1)).sum(1)
