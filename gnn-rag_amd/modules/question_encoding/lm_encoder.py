"""The frozen BERT-class question encoder of ``--lm sbert`` / ``bert`` / ``simcse`` on the MI355X.

The reference's ``BERTInstruction.encode_question`` (``gnn/modules/question_encoding/bert_encoder.py:94``) calls
``self.node_encoder(query_text)[0]``: a transformers ``BertModel`` on the input ids alone - no attention mask, so pad tokens
are attended like any other token - twice per forward (``rearev.py:138`` and ``:192``).  In transformers that is 13-15
launches per layer; ``ops.bert_encode`` runs it in 8 (``csrc/bert_encoder.hip``).

``patch_lm_encoder(instr)`` wraps ``instr.node_encoder.forward`` ON THE INSTANCE by a bound method of a state object (the
pattern of ``instruction.patch_instruction``: a ``copy.deepcopy`` of the model gets a wrapper of its own).  Parameters,
``state_dict`` keys and ``.to()`` are untouched.  A call is taken when ALL of these hold, else the original forward runs
unchanged:

* ``GNNRAG_HIP_LM`` is not ``0`` (read at every call; the default is on by the rule and the numbers of DESIGN.md section 8
  f-6; ``GNNRAG_HIP_LM=0`` leaves transformers' forward in charge of every call);
* the encoder's type is exactly transformers' ``BertModel``, with absolute positions, ``hidden_act == "gelu"``, not a decoder
  (RoBERTa, MPNet and T5 encoders keep their own forward);
* the only argument is a 2-D int64 CUDA ``input_ids`` (an ``attention_mask``, ``token_type_ids``, ... fall through);
* all parameters are contiguous fp32 CUDA tensors and the kernels take the shape (``ops.bert_encode_supported``);
* nothing needs a gradient: grad mode is off, or no LM parameter requires grad;
* dropout is inert: the module is in eval mode, or both dropout probabilities are 0 (``Trainer_KBQA`` runs a frozen LM in
  training mode with dropout 0.1: those calls fall through).

An eligible call returns a ``BaseModelOutput`` whose ``[0]`` is ``last_hidden_state``; the pooler is not computed (the
reference never reads it).  The packed query / key / value weight and bias of every layer are kept on the state object,
keyed by ``(data_ptr, _version)`` of their six source tensors (as ``install.cache_rel_features`` keys its cache): an
in-place parameter update or a ``.to()`` refreshes them.

``transformers`` is imported only inside :func:`patch_lm_encoder` and the eligible call: this package imports without it.
"""
from __future__ import annotations

import os

import torch

from ... import ops

DEFAULT = "1"        # GNNRAG_HIP_LM when unset (the rule and the measurement)


def enabled() -> bool:
    """Whether the patched forward uses the library (read at every call: the switch can change in-process)."""
    return os.environ.get("GNNRAG_HIP_LM", DEFAULT) != "0"


def _f32_cuda_contig(t) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


class _LmPatch:
    """State and wrapper of one patched encoder.  ``forward`` is a BOUND METHOD of this object (not a closure), so a
    ``copy.deepcopy`` of a patched model gets a wrapper that belongs to the copy."""

    def __init__(self, enc):
        self.enc = enc
        self.orig_forward = enc.forward
        self.key, self.packed = None, None      # the packed W_qkv / b_qkv of every layer and what they were made from
        self.hip_calls = 0                      # eligible calls served by the library (tests, tools)

    # -- eligibility ----------------------------------------------------------------------------------------------
    def refusal(self, args, kwargs):
        """None when the call runs on the library, else the first rule (of the module docstring) it does not meet."""
        enc, cfg = self.enc, self.enc.config
        if not enabled():
            return "GNNRAG_HIP_LM is off"
        if (getattr(cfg, "position_embedding_type", None) not in (None, "absolute") or
                getattr(cfg, "hidden_act", None) != "gelu" or getattr(cfg, "is_decoder", False) or
                getattr(cfg, "add_cross_attention", False)):
            return "not an absolute-position, gelu, encoder-only configuration"
        ids = args[0] if args else kwargs.get("input_ids")
        if len(args) + len(kwargs) != 1 or not isinstance(ids, torch.Tensor):
            return "arguments other than input_ids"
        if ids.dtype != torch.int64 or ids.dim() != 2 or ids.numel() == 0:
            return "input_ids is not a 2-D int64 tensor"
        params = list(enc.parameters())
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return "a gradient is needed"
        if enc.training and (float(cfg.hidden_dropout_prob) != 0.0 or float(cfg.attention_probs_dropout_prob) != 0.0):
            return "dropout is active"
        if not ops.bert_encode_supported(int(ids.shape[1]), int(cfg.hidden_size), int(cfg.num_attention_heads),
                                         int(cfg.intermediate_size), int(cfg.max_position_embeddings)):
            return "a shape the kernels do not take"
        if not ids.is_cuda:
            return "input_ids is not a CUDA tensor"
        if not all(_f32_cuda_contig(p) and p.device == ids.device for p in params):
            return "a parameter is not a contiguous fp32 tensor on the device of input_ids"
        return None

    # -- parameters -----------------------------------------------------------------------------------------------
    def _qkv_sources(self):
        out = []
        for layer in self.enc.encoder.layer:
            s = layer.attention.self
            out += [s.query.weight, s.key.weight, s.value.weight, s.query.bias, s.key.bias, s.value.bias]
        return out

    def packed_qkv(self):
        src = self._qkv_sources()
        key = tuple((p.data_ptr(), p._version) for p in src)
        if self.key != key:
            with torch.no_grad():
                self.packed = [(torch.cat([t.detach() for t in src[6 * l: 6 * l + 3]], 0).contiguous(),
                                torch.cat([t.detach() for t in src[6 * l + 3: 6 * l + 6]], 0).contiguous())
                               for l in range(len(src) // 6)]
            self.key = key
        return self.packed

    def layers(self):
        out = []
        for layer, (W_qkv, b_qkv) in zip(self.enc.encoder.layer, self.packed_qkv()):
            ao, it, fo = layer.attention.output, layer.intermediate.dense, layer.output
            out.append({"W_qkv": W_qkv, "b_qkv": b_qkv, "W_o": ao.dense.weight, "b_o": ao.dense.bias,
                        "ln1_g": ao.LayerNorm.weight, "ln1_b": ao.LayerNorm.bias, "W_i": it.weight, "b_i": it.bias,
                        "W_f": fo.dense.weight, "b_f": fo.dense.bias, "ln2_g": fo.LayerNorm.weight,
                        "ln2_b": fo.LayerNorm.bias})
        return out

    # -- the wrapper ----------------------------------------------------------------------------------------------
    def forward(self, *args, **kwargs):
        if self.refusal(args, kwargs) is not None:
            return self.orig_forward(*args, **kwargs)
        from transformers.modeling_outputs import BaseModelOutput
        enc = self.enc
        ids = args[0] if args else kwargs["input_ids"]
        emb, cfg = enc.embeddings, enc.config
        with torch.no_grad():
            hidden = ops.bert_encode(ids, emb.word_embeddings.weight, emb.position_embeddings.weight,
                                     emb.token_type_embeddings.weight, emb.LayerNorm.weight, emb.LayerNorm.bias,
                                     float(cfg.layer_norm_eps), self.layers(), int(cfg.num_attention_heads),
                                     I=int(cfg.intermediate_size))
        self.hip_calls += 1
        return BaseModelOutput(last_hidden_state=hidden)


def patch_lm_encoder(instr):
    """Wraps ``instr.node_encoder.forward`` when the encoder is exactly transformers' ``BertModel`` (see the module
    docstring).  Idempotent; anything else - no ``node_encoder``, another encoder class, no transformers - is returned as it
    is."""
    enc = getattr(instr, "node_encoder", None)
    if enc is None or getattr(enc, "_gnnrag_lm_patch", None) is not None:
        return instr
    if type(enc).__name__ != "BertModel" or not type(enc).__module__.startswith("transformers."):
        return instr                            # an nn.LSTM / HipLSTM encoder: transformers is not even imported
    try:
        from transformers import BertModel
    except ImportError:
        return instr
    if type(enc) is not BertModel:
        return instr
    p = _LmPatch(enc)
    # plain instance attributes (nn.Module.__setattr__ keeps non-module, non-parameter values in __dict__): no
    # parameter, buffer or state_dict key is added
    enc.forward = p.forward
    enc._gnnrag_lm_patch = p
    return instr
