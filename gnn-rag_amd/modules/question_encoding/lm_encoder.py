"""The frozen question encoder of ``--lm sbert`` / ``bert`` / ``simcse`` (transformers' ``BertModel``), ``--lm roberta`` /
``relbert`` (``RobertaModel``) and ``--lm sbert2`` (``MPNetModel``) on the MI355X.

The reference's ``BERTInstruction.encode_question`` (``gnn/modules/question_encoding/bert_encoder.py:94``) calls
``self.node_encoder(query_text)[0]``: the transformers model on the input ids alone - no attention mask, so pad tokens
are attended like any other token - twice per forward (``rearev.py:138`` and ``:192``).  In transformers that is 13-15
launches per layer; ``ops.bert_encode`` runs it in 8 (``csrc/bert_encoder.hip``).  The three classes are one post-LayerNorm,
erf-GELU block; what differs is read per class (``_ARCH``):

* ``RobertaModel`` and ``MPNetModel`` take a token's position from the ids (``pad_id = embeddings.padding_idx``: a pad sits
  at ``pad_id``, the n-th non-pad token at ``pad_id + n``), ``BertModel`` counts ``0 .. T-1``;
* ``MPNetModel`` has no token-type embedding, names its projections ``attention.attn.q/k/v/o`` and adds
  ``relative_attention_bias.weight[bucket(j - i)]`` to the scaled scores of every layer: the table ``[heads, 2T-1]`` is
  built here with transformers' own ``MPNetEncoder.relative_position_bucket`` and kept per ``T``.

``patch_lm_encoder(instr)`` wraps ``instr.node_encoder.forward`` ON THE INSTANCE by a bound method of a state object (the
pattern of ``instruction.patch_instruction``: a ``copy.deepcopy`` of the model gets a wrapper of its own).  Parameters,
``state_dict`` keys and ``.to()`` are untouched.  A call is taken when ALL of these hold, else the original forward runs
unchanged:

* the switch is on for the class (read at every call): ``GNNRAG_HIP_LM=0`` is off for every class, any other value is on
  for every class, unset is on for the classes in ``DEFAULT_ON`` - those whose measurement met the rule of DESIGN.md
  section 8 f-6;
* the encoder's type is exactly transformers' ``BertModel``, ``RobertaModel`` or ``MPNetModel`` (no subclass), with
  absolute position embeddings, ``hidden_act == "gelu"``, not a decoder; a RoBERTa / MPNet encoder has a ``padding_idx``,
  an MPNet encoder 32 relative-attention buckets (T5 encoders keep their own forward);
* the only argument is a 2-D int64 CUDA ``input_ids`` (an ``attention_mask``, ``token_type_ids``, ... fall through);
* all parameters are contiguous fp32 CUDA tensors and the kernels take the shape (``ops.bert_encode_supported``; with
  positions from the ids also ``T + pad_id <= max_position_embeddings - 1``, where transformers itself would raise);
* nothing needs a gradient: grad mode is off, or no LM parameter requires grad - or fine-tuning is switched on (below);
* dropout is inert: the module is in eval mode, or both dropout probabilities are 0 - or the training-mode forward is
  switched on (next paragraph).

``Trainer_KBQA`` calls ``model.train()``, which puts the frozen LM into training mode with transformers' dropout 0.1:
two encodes per step.  With ``GNNRAG_HIP_LM_TRAIN=1`` (read at every call; unset or ``0`` is off, and those calls fall
through with "dropout is active") such a call runs on ``ops.bert_encode_train`` when the class's ``GNNRAG_HIP_LM`` rule is
met, both probabilities are below 1 and every other rule above holds: :func:`draw_keep` draws the keep bytes of the four
dropout sites from torch's generator of the device and the kernels multiply them in as ``float32(1 / (1 - p))``.  These are
not ``F.dropout``'s draws: comparable loss curve, not equal draws.  Eval-mode calls and calls with both probabilities 0
stay on the inference path, bit for bit.

``GNNRAG_HIP_LM_SPLITK=1`` (read at every call; unset, empty or ``0`` is off, the default): an eligible INFERENCE call
with ``B T <= SPLITK_MAX_ROWS`` rows runs on ``ops.bert_encode(..., splitk=True)`` - the four dense products of a layer on
the split-K linear, which spreads a weight over the chip when a question brings 12 .. 20 rows, with the GELU and the
LayerNorms in its reduce.  Exact fp32 in another summation order: the states are within the same bound, not the same bits,
and a question's bits still do not depend on its batch.  Training-mode calls never take it.  Nothing else about
eligibility changes; ``hip_splitk_calls`` counts these calls beside ``hip_calls``.

``GNNRAG_HIP_LM_FINETUNE=1`` (read at every call; unset, empty or ``0`` is off, the default): the reference's
``--lm_frozen 0``.  A call that needs a gradient - grad mode on and an LM parameter requiring grad - otherwise ends in "a
gradient is needed".  With the switch on it runs on the library when the class's ``GNNRAG_HIP_LM`` rule is met, the class is
``BertModel`` or ``RobertaModel`` (``MPNetModel`` keeps transformers' forward, with a refusal text of its own: its
relative-bias table would need a gradient), ``ops.bert_layers_backward_supported`` takes the shape and every other rule
above holds.  ``x0 = enc.embeddings(input_ids)`` is then transformers' own module under torch autograd - its LayerNorm, its
dropout, its position rule, its lookup backward - and the layers run on ``autograd.BertLayersFn``
(``gnnrag_bert_layers_forward_save`` / ``gnnrag_bert_layers_backward``).  Active dropout does not need
``GNNRAG_HIP_LM_TRAIN`` on this path: the keep bytes of planes ``1 .. 2L`` and of the attention planes come from
:func:`draw_keep` (comparable loss curve, not equal draws).  The reserve belongs to the autograd context of the call: two
encodes followed by one backward each read their own.  ``hip_finetune_calls`` counts these calls beside ``hip_calls``.  With
the switch off or unset every call behaves as without it.

``GNNRAG_HIP_LM_FINETUNE_FULL=1`` (read at every call; unset, empty or ``0`` is off, the default; it has a meaning only
together with ``GNNRAG_HIP_LM_FINETUNE=1``): the whole encoder on the library.  ``x0`` then comes from
``autograd.BertEmbedFn`` (``gnnrag_bert_embed_forward_save`` / ``gnnrag_bert_embed_backward``: the lookups, the positions, the
LayerNorm and keep plane 0 of :func:`draw_keep` in one launch; the three table gradients dense and without atomics, the
``padding_idx`` rows zero as transformers leaves them), and an ``MPNetModel`` is taken as well: its bias table is built
differentiably per call as ``relative_attention_bias.weight[bucket].t()`` and the layers run on
``autograd.BertLayersBiasFn``, which returns the table's gradient; torch autograd carries it to the weight.  One more
refusal: "more rows than the embedding backward takes" (``ops.bert_embed_backward_supported``).
``hip_finetune_full_calls`` counts these calls beside ``hip_finetune_calls``.  With the switch off every call behaves as
without it, bit for bit.

An eligible call returns a ``BaseModelOutput`` whose ``[0]`` is ``last_hidden_state``; the pooler is not computed (the
reference never reads it).  The packed query / key / value weight and bias of every layer are kept on the state object,
keyed by ``(data_ptr, _version)`` of their six source tensors (as ``install.cache_rel_features`` keys its cache): an
in-place parameter update or a ``.to()`` refreshes them; MPNet's bias tables are keyed the same way.

``transformers`` is imported only inside :func:`patch_lm_encoder` and the eligible call: this package imports without it.
"""
from __future__ import annotations

import os

import torch

from ... import ops

DEFAULT = "1"        # GNNRAG_HIP_LM for BertModel when unset (the rule and the measurement)
# classes that are on when GNNRAG_HIP_LM is unset; the others need GNNRAG_HIP_LM=1.  RobertaModel and MPNetModel were
# measured at the 768-wide, 12-layer shape: 3-4 x less host time, but more stream time than transformers at B = 1 and
# B = 64 (DESIGN.md section 8 f-6 keeps the numbers), so by the rule they stay off
DEFAULT_ON = ("BertModel",)
TRAIN_DEFAULT = "0"  # GNNRAG_HIP_LM_TRAIN when unset: off (DESIGN.md section 8 f-6 has the rule for a later flip)
FINETUNE_DEFAULT = "0"  # GNNRAG_HIP_LM_FINETUNE when unset: off (Fine-tuning: the rule for a flip)
FINETUNE_FULL_DEFAULT = "0"  # GNNRAG_HIP_LM_FINETUNE_FULL when unset: off (Fine-tuning)
SPLITK_DEFAULT = "0"  # GNNRAG_HIP_LM_SPLITK when unset: off (DESIGN.md section 8 f-6 keeps the measurement)
# the largest B T at which an inference call with GNNRAG_HIP_LM_SPLITK set takes the split-K encode: the largest measured
# shape, (8, 20), at which its stream time is not worse than the encode without the switch; at (64, 20) it is
# (tools/time_bert_encoder.py --splitk, profiles/bert_encoder_splitk_time.jsonl)
SPLITK_MAX_ROWS = 160
REL_BUCKETS = 32                # MPNetEncoder.compute_position_bias passes its default, whatever the configuration says

# what differs between the classes: where positions come from, the token-type term, the attention bias, the names
_ARCH = {
    "BertModel": dict(id_positions=False, token_type=True, rel_bias=False),
    "RobertaModel": dict(id_positions=True, token_type=True, rel_bias=False),
    "MPNetModel": dict(id_positions=True, token_type=False, rel_bias=True),
}


def enabled(arch: str = "BertModel") -> bool:
    """Whether the patched forward of an encoder of class ``arch`` uses the library (read at every call: the switch can
    change in-process)."""
    v = os.environ.get("GNNRAG_HIP_LM")
    if v is None:
        return arch in DEFAULT_ON and DEFAULT != "0"
    return v != "0"


def train_enabled() -> bool:
    """Whether a training-mode call with active dropout may use the library (``GNNRAG_HIP_LM_TRAIN``, read at every
    call)."""
    return os.environ.get("GNNRAG_HIP_LM_TRAIN", TRAIN_DEFAULT) not in ("0", "")


def finetune_enabled() -> bool:
    """Whether a call that needs a gradient may run its layers on the library (``GNNRAG_HIP_LM_FINETUNE``, read at every
    call; unset, empty or ``0`` is off)."""
    return os.environ.get("GNNRAG_HIP_LM_FINETUNE", FINETUNE_DEFAULT) not in ("0", "")


def finetune_full_enabled() -> bool:
    """Whether a fine-tuning call also runs its embedding stage on the library, and an ``MPNetModel`` may be fine-tuned on it
    (``GNNRAG_HIP_LM_FINETUNE_FULL``, read at every call; unset, empty or ``0`` is off).  It has a meaning only together
    with ``GNNRAG_HIP_LM_FINETUNE``."""
    return os.environ.get("GNNRAG_HIP_LM_FINETUNE_FULL", FINETUNE_FULL_DEFAULT) not in ("0", "")


def splitk_enabled() -> bool:
    """Whether an eligible inference call may take the split-K encode (``GNNRAG_HIP_LM_SPLITK``, read at every call; unset,
    empty or ``0`` is off)."""
    return os.environ.get("GNNRAG_HIP_LM_SPLITK", SPLITK_DEFAULT) not in ("0", "")


def splitk_rows_ok(B: int, T: int) -> bool:
    """The split-K encode is for few rows: ``B T <= SPLITK_MAX_ROWS``."""
    return 0 < int(B) * int(T) <= SPLITK_MAX_ROWS


def draw_keep(L: int, B: int, T: int, H: int, heads: int, p_hidden: float, p_att: float, device):
    """The keep bytes of one training-mode encode: ``(keep_hidden, keep_att)`` of the shapes of ``ops.bert_keep_shapes``,
    uint8, each byte 1 with probability ``1 - p`` (``bernoulli_`` on torch's generator of ``device``); ``None`` for a site
    whose ``p`` is 0 (and for the attention site of an encoder without layers).  One draw launch when the two
    probabilities are equal - the two buffers are views of one - two otherwise.  Comparable loss curve, not equal draws:
    these are not the numbers ``F.dropout`` would have drawn."""
    shape_h, shape_a = ops.bert_keep_shapes(L, B, T, H, heads)
    n_h = shape_h[0] * shape_h[1] * shape_h[2] if p_hidden != 0.0 else 0
    n_a = shape_a[0] * shape_a[1] * shape_a[2] * shape_a[3] * shape_a[4] if p_att != 0.0 else 0

    def one(n, p):
        return torch.empty(n, dtype=torch.uint8, device=device).bernoulli_(1.0 - float(p))

    if n_h and n_a and float(p_hidden) == float(p_att):
        both = one(n_h + n_a, p_hidden)         # the hidden planes first: they stay 4-byte aligned (H % 4 == 0)
        return both[:n_h].view(shape_h), both[n_h:].view(shape_a)
    return (one(n_h, p_hidden).view(shape_h) if n_h else None), (one(n_a, p_att).view(shape_a) if n_a else None)


def _scale(p: float) -> float:
    """float32(1 / (1 - p)): what the kernels multiply a kept element by."""
    return float(torch.tensor(1.0 / (1.0 - float(p)), dtype=torch.float32))


def _f32_cuda_contig(t) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


def rel_bias_table(encoder, T: int) -> torch.Tensor:
    """``[heads, 2T-1]``: entry ``[h, d + T - 1]`` is what ``MPNetEncoder.compute_position_bias`` adds to the score of
    query i and key j = i + d of head h.  The buckets come from transformers' own function, on the CPU as it runs it."""
    d = torch.arange(-(T - 1), T, dtype=torch.long)
    bucket = type(encoder).relative_position_bucket(d, num_buckets=REL_BUCKETS)
    w = encoder.relative_attention_bias.weight.detach()
    return w[bucket.to(w.device)].t().contiguous()


class _LmPatch:
    """State and wrapper of one patched encoder.  ``forward`` is a BOUND METHOD of this object (not a closure), so a
    ``copy.deepcopy`` of a patched model gets a wrapper that belongs to the copy."""

    def __init__(self, enc):
        self.enc = enc
        self.arch = type(enc).__name__
        self.orig_forward = enc.forward
        self.key, self.packed = None, None      # the packed W_qkv / b_qkv of every layer and what they were made from
        self.bias_key, self.bias = None, {}     # MPNet: T -> the bias table, and the weight they were made from
        self.hip_calls = 0                      # eligible calls served by the library (tests, tools)
        self.hip_train_calls = 0                # those of them that ran the training-mode forward
        self.hip_splitk_calls = 0               # those of them that ran the split-K inference encode
        self.hip_finetune_calls = 0             # those of them that ran the layers under autograd (fine-tuning)
        self.hip_finetune_full_calls = 0        # those of these that ran the embedding stage on the library as well

    # -- eligibility ----------------------------------------------------------------------------------------------
    def pad_id(self):
        """The padding id positions are counted from (RoBERTa, MPNet), else None."""
        if not _ARCH[self.arch]["id_positions"]:
            return None
        pad = getattr(self.enc.embeddings, "padding_idx", None)
        return int(pad) if isinstance(pad, int) and not isinstance(pad, bool) else -1

    def dropout_active(self) -> bool:
        cfg = self.enc.config
        return bool(self.enc.training and (float(cfg.hidden_dropout_prob) != 0.0 or
                                           float(cfg.attention_probs_dropout_prob) != 0.0))

    def needs_grad(self) -> bool:
        """Whether a call now would have to be differentiated: grad mode is on and an LM parameter requires grad."""
        return bool(torch.is_grad_enabled() and any(p.requires_grad for p in self.enc.parameters()))

    def refusal(self, args, kwargs):
        """None when the call runs on the library, else the first rule (of the module docstring) it does not meet."""
        enc, cfg, arch = self.enc, self.enc.config, _ARCH[self.arch]
        if not enabled(self.arch):
            return "GNNRAG_HIP_LM is off"
        if (getattr(cfg, "position_embedding_type", None) not in (None, "absolute") or
                getattr(cfg, "hidden_act", None) != "gelu" or getattr(cfg, "is_decoder", False) or
                getattr(cfg, "add_cross_attention", False)):
            return "not an absolute-position, gelu, encoder-only configuration"
        pad = self.pad_id()
        if pad is not None and pad < 0:
            return "no padding_idx to count positions from"
        if arch["rel_bias"] and (int(getattr(cfg, "relative_attention_num_buckets", 0)) != REL_BUCKETS or
                                 enc.encoder.relative_attention_bias.weight.shape[0] != REL_BUCKETS):
            return "a relative attention bias of other than 32 buckets"
        ids = args[0] if args else kwargs.get("input_ids")
        if len(args) + len(kwargs) != 1 or not isinstance(ids, torch.Tensor):
            return "arguments other than input_ids"
        if ids.dtype != torch.int64 or ids.dim() != 2 or ids.numel() == 0:
            return "input_ids is not a 2-D int64 tensor"
        params = list(enc.parameters())
        finetune = self.needs_grad()
        if finetune:
            if not finetune_enabled():
                return "a gradient is needed"
            full = finetune_full_enabled()
            if arch["rel_bias"] and not full:
                return "a gradient is needed and the relative attention bias has no backward on the library"
            if len(enc.encoder.layer) < 1 or not ops.bert_layers_backward_supported(
                    int(ids.shape[1]), int(cfg.hidden_size), int(cfg.num_attention_heads), int(cfg.intermediate_size)):
                return "a shape the backward kernels do not take"
            if full and not ops.bert_embed_backward_supported(int(ids.numel()), int(cfg.hidden_size)):
                return "more rows than the embedding backward takes"
        if self.dropout_active():
            if not finetune and not train_enabled():
                return "dropout is active"
            if not (float(cfg.hidden_dropout_prob) < 1.0 and float(cfg.attention_probs_dropout_prob) < 1.0):
                return "a dropout probability of 1"
        if not ops.bert_encode_supported(int(ids.shape[1]), int(cfg.hidden_size), int(cfg.num_attention_heads),
                                         int(cfg.intermediate_size), int(cfg.max_position_embeddings), pad_id=pad):
            return "a shape the kernels do not take"
        if not ids.is_cuda:
            return "input_ids is not a CUDA tensor"
        if not all(_f32_cuda_contig(p) and p.device == ids.device for p in params):
            return "a parameter is not a contiguous fp32 tensor on the device of input_ids"
        return None

    # -- parameters -----------------------------------------------------------------------------------------------
    def _modules(self, layer):
        """One layer's modules: (query, key, value, output projection, the LayerNorm behind it, intermediate dense, output
        dense, the LayerNorm behind it) - the only place that knows a transformers layer's attribute names."""
        a = layer.attention
        att = ((a.attn.q, a.attn.k, a.attn.v, a.attn.o, a.LayerNorm) if self.arch == "MPNetModel" else
               (a.self.query, a.self.key, a.self.value, a.output.dense, a.output.LayerNorm))
        return att + (layer.intermediate.dense, layer.output.dense, layer.output.LayerNorm)

    def _qkv_sources(self):
        out = []
        for layer in self.enc.encoder.layer:
            q, k, v = self._modules(layer)[:3]
            out += [q.weight, k.weight, v.weight, q.bias, k.bias, v.bias]
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
            o, ln1, it, fo, ln2 = self._modules(layer)[3:]
            out.append({"W_qkv": W_qkv, "b_qkv": b_qkv, "W_o": o.weight, "b_o": o.bias,
                        "ln1_g": ln1.weight, "ln1_b": ln1.bias, "W_i": it.weight, "b_i": it.bias,
                        "W_f": fo.weight, "b_f": fo.bias, "ln2_g": ln2.weight, "ln2_b": ln2.bias})
        return out

    def _draw(self, L, ids):
        """``(p_hidden, p_att, keep_hidden, keep_att)`` of one call with active dropout: the configuration's two
        probabilities and one :func:`draw_keep` for ``L`` layers on the device of ``ids``."""
        cfg = self.enc.config
        p_h, p_a = float(cfg.hidden_dropout_prob), float(cfg.attention_probs_dropout_prob)
        keep_h, keep_a = draw_keep(L, int(ids.shape[0]), int(ids.shape[1]), int(cfg.hidden_size),
                                   int(cfg.num_attention_heads), p_h, p_a, ids.device)
        return p_h, p_a, keep_h, keep_a

    def rel_bias(self, T):
        """MPNet's bias table for ``T`` tokens (None for the other classes), kept until the weight changes."""
        if not _ARCH[self.arch]["rel_bias"]:
            return None
        w = self.enc.encoder.relative_attention_bias.weight
        key = (w.data_ptr(), w._version)
        if self.bias_key != key:
            self.bias_key, self.bias = key, {}
        if T not in self.bias:
            with torch.no_grad():
                self.bias[T] = rel_bias_table(self.enc.encoder, T)
        return self.bias[T]

    def _finetune(self, ids):
        """The unfrozen encoder: transformers' embedding stage under torch autograd (its LayerNorm, its dropout, its
        position rule), then the layers on ``autograd.BertLayersFn``."""
        from ... import autograd
        enc, cfg = self.enc, self.enc.config
        full = finetune_full_enabled()
        if not full:
            x0 = enc.embeddings(input_ids=ids)
        p_h, p_a, keep_h, keep_a = 0.0, 0.0, None, None
        if self.dropout_active():
            # without GNNRAG_HIP_LM_FINETUNE_FULL plane 0 (the embedding's) is not read
            p_h, p_a, keep_h, keep_a = self._draw(len(enc.encoder.layer), ids)
        if full:
            x0 = self._embed_full(ids, keep_h, p_h)
        params = []
        for layer in enc.encoder.layer:
            q, k, v, o, ln1, it, fo, ln2 = self._modules(layer)
            params += [q.weight, k.weight, v.weight, q.bias, k.bias, v.bias, o.weight, o.bias, ln1.weight, ln1.bias,
                       it.weight, it.bias, fo.weight, fo.bias, ln2.weight, ln2.bias]
        if _ARCH[self.arch]["rel_bias"]:        # only with GNNRAG_HIP_LM_FINETUNE_FULL (refusal)
            # the table as a function of the weight, per call: torch autograd carries its gradient back through the
            # bucket gather (rel_bias_table detaches and caches: that one is for the frozen paths)
            T = int(ids.shape[1])
            w = enc.encoder.relative_attention_bias.weight
            bucket = type(enc.encoder).relative_position_bucket(torch.arange(-(T - 1), T, dtype=torch.long),
                                                                num_buckets=REL_BUCKETS)
            table = w[bucket.to(w.device)].t()
            return autograd.BertLayersBiasFn.apply(x0, table, keep_h, _scale(p_h), keep_a, _scale(p_a),
                                                   int(cfg.num_attention_heads), float(cfg.layer_norm_eps), *params)
        return autograd.BertLayersFn.apply(x0, keep_h, _scale(p_h), keep_a, _scale(p_a), int(cfg.num_attention_heads),
                                           float(cfg.layer_norm_eps), *params)

    def _embed_full(self, ids, keep_h, p_h):
        """The embedding stage on ``autograd.BertEmbedFn``: keep plane 0 is read, the padding rows are transformers'
        ``padding_idx`` of the two tables."""
        from ... import autograd
        emb, cfg = self.enc.embeddings, self.enc.config
        type_emb = emb.token_type_embeddings.weight if _ARCH[self.arch]["token_type"] else None
        return autograd.BertEmbedFn.apply(ids, None if keep_h is None else keep_h[0], _scale(p_h), self.pad_id(),
                                          emb.word_embeddings.padding_idx, emb.position_embeddings.padding_idx,
                                          float(cfg.layer_norm_eps), emb.word_embeddings.weight,
                                          emb.position_embeddings.weight, type_emb, emb.LayerNorm.weight,
                                          emb.LayerNorm.bias)

    # -- the wrapper ----------------------------------------------------------------------------------------------
    def forward(self, *args, **kwargs):
        if self.refusal(args, kwargs) is not None:
            return self.orig_forward(*args, **kwargs)
        from transformers.modeling_outputs import BaseModelOutput
        enc = self.enc
        ids = args[0] if args else kwargs["input_ids"]
        emb, cfg = enc.embeddings, enc.config
        if self.needs_grad():
            hidden = self._finetune(ids)
            self.hip_calls += 1
            self.hip_finetune_calls += 1
            self.hip_finetune_full_calls += int(finetune_full_enabled())
            return BaseModelOutput(last_hidden_state=hidden)
        type_emb = emb.token_type_embeddings.weight if _ARCH[self.arch]["token_type"] else None
        top = (ids, emb.word_embeddings.weight, emb.position_embeddings.weight, type_emb, emb.LayerNorm.weight,
               emb.LayerNorm.bias, float(cfg.layer_norm_eps), self.layers(), int(cfg.num_attention_heads))
        rest = dict(I=int(cfg.intermediate_size), pad_id=self.pad_id(), rel_bias=self.rel_bias(int(ids.shape[1])))
        with torch.no_grad():
            if self.dropout_active():
                p_h, p_a, keep_h, keep_a = self._draw(len(top[7]), ids)
                hidden = ops.bert_encode_train(*top, keep_hidden=keep_h, scale_hidden=_scale(p_h), keep_att=keep_a,
                                               scale_att=_scale(p_a), **rest)
                self.hip_train_calls += 1
            elif splitk_enabled() and splitk_rows_ok(int(ids.shape[0]), int(ids.shape[1])):
                hidden = ops.bert_encode(*top, splitk=True, **rest)
                self.hip_splitk_calls += 1
            else:
                hidden = ops.bert_encode(*top, **rest)
        self.hip_calls += 1
        return BaseModelOutput(last_hidden_state=hidden)


def patch_lm_encoder(instr):
    """Wraps ``instr.node_encoder.forward`` when the encoder is exactly transformers' ``BertModel``, ``RobertaModel`` or
    ``MPNetModel`` (see the module docstring).  Idempotent; anything else - no ``node_encoder``, another encoder class, a
    subclass, no transformers - is returned as it is."""
    enc = getattr(instr, "node_encoder", None)
    if enc is None or getattr(enc, "_gnnrag_lm_patch", None) is not None:
        return instr
    name = type(enc).__name__
    if name not in _ARCH or not type(enc).__module__.startswith("transformers."):
        return instr                            # an nn.LSTM / HipLSTM encoder: transformers is not even imported
    try:
        import transformers
        cls = getattr(transformers, name)
    except (ImportError, AttributeError):
        return instr
    if type(enc) is not cls:
        return instr
    p = _LmPatch(enc)
    # plain instance attributes (nn.Module.__setattr__ keeps non-module, non-parameter values in __dict__): no
    # parameter, buffer or state_dict key is added
    enc.forward = p.forward
    enc._gnnrag_lm_patch = p
    return instr
