"""ctypes binding of libgnnrag_hip.so (C ABI declared in include/gnnrag.h).

There is deliberately NO fallback: if the HIP library is missing or an entry point
is absent, importing/using the product path raises.  (CPU restatements live under
``oracle/`` and are test infrastructure only.)
"""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "lib", "libgnnrag_hip.so")

c_i32p = C.POINTER(C.c_int32)
c_f32p = C.POINTER(C.c_float)


class CsrStruct(C.Structure):
    """Mirror of ``struct gnnrag_csr`` (include/gnnrag.h)."""
    _fields_ = [
        ("B", C.c_int32), ("N", C.c_int32), ("R1", C.c_int32), ("heavy_deg", C.c_int32),
        ("F", C.c_int64),
        ("row_ptr", C.c_void_p * 2), ("edge", C.c_void_p * 2), ("perm", C.c_void_p * 2),
        ("w_gnn", C.c_void_p * 2), ("w_rel", C.c_void_p * 2),
        ("heavy", C.c_void_p * 2), ("chunk_off", C.c_void_p * 2),
        ("n_heavy", C.c_void_p), ("n_chunks", C.c_void_p),
        ("heavy_cap", C.c_int32), ("max_chunks", C.c_int32),
        ("big_cnt", C.c_void_p), ("big_nodes", C.c_void_p),
        ("big_deg", C.c_int32), ("hub_sorted", C.c_int32),
        ("edge_l", C.c_void_p * 2), ("rel_off", C.c_void_p), ("rel_rows", C.c_void_p),
        ("rel_total", C.c_int32), ("rel_max", C.c_int32),
        ("edge_m", C.c_void_p), ("m_from", C.c_void_p), ("m_dst", C.c_void_p),
        ("hub_q_off", C.c_void_p * 2), ("hub_wbase", C.c_void_p * 2),
    ]


class RelorderStruct(C.Structure):
    """Mirror of ``struct gnnrag_relorder`` (include/gnnrag.h)."""
    _fields_ = [("F", C.c_int64), ("rel_total", C.c_int32), ("n_chunks", C.c_int32),
                ("ht", C.c_void_p), ("perm", C.c_void_p), ("w", C.c_void_p), ("row_ptr", C.c_void_p),
                ("chunk_ptr", C.c_void_p)]


class UGraphStruct(C.Structure):
    """Mirror of ``struct gnnrag_ugraph`` (include/gnnrag.h)."""
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("F", C.c_int64), ("cap", C.c_int64),
                ("u_ptr", C.c_void_p), ("u_adj", C.c_void_p)]


class DenseFormStruct(C.Structure):
    """Mirror of ``struct gnnrag_dense_form_t`` (include/gnnrag.h)."""
    _fields_ = [(n, C.c_int32) for n in ("family", "block_family", "launches", "epi", "nt", "mt", "v4", "math", "nw",
                                          "v4out", "n0", "nc", "has_add", "kguard")]


class LayerParams(C.Structure):
    """Mirror of ``struct gnnrag_layer_params`` (include/gnnrag.h)."""
    _fields_ = [("W_rel", C.c_void_p), ("b_rel", C.c_void_p), ("pos_fwd", C.c_void_p), ("pos_inv", C.c_void_p),
                ("W_e2e", C.c_void_p), ("b_e2e", C.c_void_p)]


class BertLayer(C.Structure):
    """Mirror of ``struct gnnrag_bert_layer`` (include/gnnrag.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("W_qkv", "b_qkv", "W_o", "b_o", "ln1_g", "ln1_b", "W_i", "b_i", "W_f", "b_f",
                                          "ln2_g", "ln2_b")]


class BertLayerGrads(C.Structure):
    """Mirror of ``struct gnnrag_bert_layer_grads`` (include/gnnrag.h); a NULL field is a gradient that is not wanted."""
    _fields_ = [(n, C.c_void_p) for n in ("dW_qkv", "db_qkv", "dW_o", "db_o", "dln1_g", "dln1_b", "dW_i", "db_i", "dW_f",
                                          "db_f", "dln2_g", "dln2_b")]


class SplitkPlanStruct(C.Structure):
    """Mirror of ``struct gnnrag_splitk_plan_t`` (include/gnnrag.h)."""
    _fields_ = [("splits", C.c_int32), ("k_chunk", C.c_int32), ("launches", C.c_int32), ("reserved", C.c_int32 * 5)]


class OptimSeg(C.Structure):
    """Mirror of ``struct gnnrag_optim_seg`` (include/gnnrag.h): 80 bytes, one entry per tensor of an optimiser step."""
    _fields_ = ([(n, C.c_void_p) for n in ("p", "g", "m", "v")] + [("n", C.c_int64), ("first_chunk", C.c_int64)] +
                [(n, C.c_float) for n in ("beta1", "beta2", "om_beta1", "om_beta2", "eps", "weight_decay", "step_size",
                                          "bc2_sqrt")])


OPTIM_CHUNK = 4096                               # GNNRAG_OPTIM_CHUNK (include/gnnrag.h)

# name -> (restype, argtypes); every symbol include/gnnrag.h declares
_VP = C.c_void_p
SIGNATURES = {
    "gnnrag_csr_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_int]),
    "gnnrag_csr_scratch_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "gnnrag_csr_build": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                   _VP, C.c_size_t, _VP, C.c_size_t, C.POINTER(CsrStruct), _VP]),
    "gnnrag_csr_build_counts": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, _VP, C.c_size_t, _VP, C.c_size_t, C.POINTER(CsrStruct), _VP]),
    "gnnrag_csr_status": (C.c_int, [C.POINTER(CsrStruct), _VP]),
    "gnnrag_csr_concat": (C.c_int, [C.POINTER(C.POINTER(CsrStruct)), C.c_int32, C.c_int32, C.c_int32, _VP, C.c_size_t,
                                    C.POINTER(CsrStruct), _VP]),
    "gnnrag_narrow_tuple": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, C.c_int32]),
    "gnnrag_csr_permute_weight": (C.c_int, [C.POINTER(CsrStruct), _VP, C.c_int, _VP, _VP, _VP]),
    "gnnrag_linear": (C.c_int, [_VP, C.c_int64, C.c_int32, _VP, _VP, _VP, C.c_int64, C.c_int, _VP,
                                C.c_int32, C.c_int32, _VP]),
    "gnnrag_linear_pair": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, _VP, _VP, _VP, _VP, C.c_int64, _VP, _VP,
                                     C.c_int32, C.c_int32, _VP]),
    "gnnrag_aggregate_workspace_bytes": (C.c_size_t, [C.POINTER(CsrStruct), C.c_int32, C.c_int32]),
    "gnnrag_aggregate": (C.c_int, [C.POINTER(CsrStruct), _VP, _VP, _VP, _VP, _VP, C.c_int32, C.c_int32,
                                   _VP, C.c_size_t, _VP]),
    "gnnrag_aggregate_fused": (C.c_int, [C.POINTER(CsrStruct), _VP, _VP, _VP, C.c_int32, _VP, C.c_size_t, _VP]),
    "gnnrag_aggregate_fused_variant": (C.c_int, [C.POINTER(CsrStruct), C.c_int32]),
    "gnnrag_aggregate_fused_hub_form": (C.c_int, [C.POINTER(CsrStruct), C.c_int32, _VP, C.c_size_t, _VP, _VP]),
    "gnnrag_relorder_bytes": (C.c_size_t, [C.POINTER(CsrStruct), C.c_int]),
    "gnnrag_relorder_scratch_bytes": (C.c_size_t, [C.POINTER(CsrStruct)]),
    "gnnrag_relorder_build": (C.c_int, [C.POINTER(CsrStruct), _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP, C.c_size_t,
                                        C.POINTER(RelorderStruct), _VP]),
    "gnnrag_backward_workspace_bytes": (C.c_size_t, [C.POINTER(CsrStruct), C.POINTER(RelorderStruct), C.c_int32,
                                                     C.c_int32]),
    "gnnrag_aggregate_fused_backward": (C.c_int, [C.POINTER(CsrStruct), C.POINTER(RelorderStruct), _VP, _VP, _VP, _VP, _VP,
                                                 C.c_int32, _VP, C.c_size_t, _VP]),
    "gnnrag_aggregate_backward": (C.c_int, [C.POINTER(CsrStruct), C.POINTER(RelorderStruct), _VP, _VP, _VP, _VP, _VP,
                                            _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, _VP, C.c_size_t, _VP]),
    "gnnrag_typelayer_backward": (C.c_int, [C.POINTER(CsrStruct), C.POINTER(RelorderStruct), _VP, _VP, C.c_int, _VP,
                                            C.c_int32, _VP, C.c_size_t, _VP]),
    "gnnrag_lstm_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gnnrag_lstm_forward": (C.c_int, [_VP] * 10 + [C.c_int32] * 4 + [_VP, C.c_size_t, _VP]),
    # training form of the LSTM (additive to ABI 16)
    "gnnrag_lstm_reserve_bytes": (C.c_size_t, [C.c_int32] * 3),
    "gnnrag_lstm_forward_train": (C.c_int, [_VP] * 10 + [C.c_int32] * 4 + [_VP, C.c_size_t, _VP, C.c_size_t, _VP]),
    "gnnrag_lstm_backward_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "gnnrag_lstm_backward": (C.c_int, [_VP] * 7 + [C.c_size_t] + [_VP] * 9 + [C.c_int32] * 4 + [_VP, C.c_size_t, _VP]),
    "gnnrag_seed_retrieve": (C.c_int, [_VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP]),
    "gnnrag_query_reform": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, _VP]),
    "gnnrag_topp_candidates": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_double, C.c_double, _VP, _VP, _VP]),
    "gnnrag_topp_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gnnrag_topp_candidates_ws": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, C.c_double, C.c_double, _VP, _VP, _VP,
                                            C.c_size_t, _VP]),
    "gnnrag_relation_tables": (C.c_int, [C.POINTER(CsrStruct), _VP, _VP, _VP, _VP, _VP, C.c_int32, C.c_int32,
                                         C.c_int32, _VP]),
    "gnnrag_update_score_fused": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_int64, C.c_int32,
                                            C.c_int32, C.c_int32, _VP]),
    "gnnrag_update_score": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_int64, C.c_int32,
                                      C.c_int32, C.c_int32, _VP]),
    # which kernel a dense call runs (host only; additive to ABI 16)
    "gnnrag_dense_form": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                    C.c_int32, C.c_int32, C.POINTER(DenseFormStruct)]),
    "gnnrag_masked_softmax": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32, _VP]),
    "gnnrag_typelayer": (C.c_int, [C.POINTER(CsrStruct), _VP, C.c_int, _VP, C.c_int32, _VP, C.c_size_t, _VP]),
    "gnnrag_layer_workspace_bytes": (C.c_size_t, [C.POINTER(CsrStruct), C.c_int32, C.c_int32]),
    "gnnrag_stack_workspace_bytes": (C.c_size_t, [C.POINTER(CsrStruct), C.c_int32, C.c_int32, C.c_int32]),
    "gnnrag_rel_transform": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.POINTER(LayerParams), C.c_int32, _VP,
                                      _VP, _VP]),
    "gnnrag_gemm_tn_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "gnnrag_gemm_tn": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, C.c_int32, _VP, _VP, C.c_size_t, _VP]),
    "gnnrag_rel_planes_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "gnnrag_relation_tables_planes": (C.c_int, [C.POINTER(CsrStruct), _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, _VP]),
    # the packed sparse operand of the relation tables (additive to ABI 16)
    "gnnrag_rel_packed_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "gnnrag_rel_transform_packed": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, C.c_int32, C.POINTER(LayerParams), C.c_int32,
                                             _VP, _VP, _VP]),
    "gnnrag_relation_tables_packed": (C.c_int, [C.POINTER(CsrStruct), _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32,
                                               _VP]),
    "gnnrag_reason_layer": (C.c_int, [C.POINTER(CsrStruct)] + [_VP] * 9 + [C.c_int32] + [_VP] * 8 +
                            [_VP, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP]),
    "gnnrag_reason_stack": (C.c_int, [C.POINTER(CsrStruct), C.c_int32, C.POINTER(LayerParams)] + [_VP] * 5 +
                            [C.c_int32] + [_VP] * 6 + [_VP, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP]),
    "gnnrag_reason_stack_capture": (C.c_int, [C.POINTER(CsrStruct), C.c_int32, C.POINTER(LayerParams)] + [_VP] * 5 +
                                    [C.c_int32] + [_VP] * 6 + [_VP, C.c_size_t, C.c_int32, C.c_int32, C.c_int32,
                                                               C.c_int32, _VP, C.POINTER(C.c_void_p)]),
    "gnnrag_graph_launch": (C.c_int, [_VP, _VP]),
    "gnnrag_graph_destroy": (C.c_int, [_VP]),
    "gnnrag_frontier_workspace_bytes": (C.c_size_t, [C.POINTER(CsrStruct)]),
    "gnnrag_frontier_supported": (C.c_int, [C.POINTER(CsrStruct), C.c_int32]),
    "gnnrag_frontier_build": (C.c_int, [C.POINTER(CsrStruct), _VP, _VP, C.c_size_t, _VP]),
    "gnnrag_relation_tables_frontier": (C.c_int, [C.POINTER(CsrStruct), _VP, _VP, _VP, _VP, _VP, _VP, C.c_int32,
                                                  C.c_int32, _VP]),
    "gnnrag_aggregate_fused_frontier": (C.c_int, [C.POINTER(CsrStruct), _VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "gnnrag_frontier_read": (C.c_int, [C.POINTER(CsrStruct), _VP, _VP, _VP, _VP]),
    # the projections and the frontier build of a seed layer in one launch (additive to ABI 16)
    "gnnrag_frontier_layout": (C.c_int, [C.POINTER(CsrStruct), C.POINTER(C.c_uint64)]),
    "gnnrag_seed_prologue": (C.c_int, [C.POINTER(CsrStruct), _VP, _VP, C.c_size_t, _VP, C.c_int64, _VP, C.c_int64, _VP, _VP,
                                      C.c_int32, C.c_int32, C.POINTER(LayerParams), C.c_int32, _VP, _VP,
                                      C.POINTER(C.c_int32), _VP]),
    # instruction generation (additive to ABI 16)
    "gnnrag_instructions": (C.c_int, [_VP] * 4 + [C.POINTER(C.c_void_p)] * 2 + [_VP] * 4 + [C.c_int32] * 4 + [_VP] * 3),
    # training form of instruction generation (additive to ABI 16)
    "gnnrag_instructions_reserve_bytes": (C.c_size_t, [C.c_int32] * 4),
    "gnnrag_instructions_train": (C.c_int, [_VP] * 4 + [C.POINTER(C.c_void_p)] * 2 + [_VP] * 7 + [C.c_int32] * 4 +
                                  [_VP] * 3 + [C.c_size_t, _VP]),
    "gnnrag_instructions_backward_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "gnnrag_instructions_backward": (C.c_int, [_VP] * 3 + [C.POINTER(C.c_void_p)] + [_VP] * 8 + [C.c_size_t] + [_VP] * 5 +
                                     [C.POINTER(C.c_void_p)] * 2 + [_VP] * 4 + [C.c_int32] * 4 + [_VP, C.c_size_t, _VP]),
    # training form of the instruction update (additive to ABI 16)
    "gnnrag_query_reform_reserve_bytes": (C.c_size_t, [C.c_int32] * 3),
    "gnnrag_query_reform_train": (C.c_int, [C.POINTER(C.c_void_p), _VP, _VP, C.c_int64] + [C.POINTER(C.c_void_p)] * 2 +
                                  [_VP, _VP, C.c_size_t] + [C.c_int32] * 4 + [_VP]),
    "gnnrag_query_reform_backward_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "gnnrag_query_reform_backward": (C.c_int, [C.POINTER(C.c_void_p), _VP] + [C.POINTER(C.c_void_p)] * 2 +
                                     [_VP, C.c_size_t] + [C.POINTER(C.c_void_p)] * 4 + [_VP] + [C.c_int32] * 4 +
                                     [_VP, C.c_size_t, _VP]),
    # the tail of the reasoning layer under autograd (additive to ABI 16)
    "gnnrag_layer_tail_train": (C.c_int, [_VP] * 3 + [C.c_float] + [_VP] * 3 + [C.c_int32] * 3 + [_VP] * 4),
    "gnnrag_layer_tail_backward_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "gnnrag_layer_tail_backward": (C.c_int, [_VP] * 3 + [C.c_float] + [_VP] * 3 + [C.c_int32] * 3 + [_VP] * 4 +
                                   [C.c_size_t, _VP]),
    # the concatenated update under dropout, forward and backward (additive to ABI 16)
    "gnnrag_update_drop_train": (C.c_int, [_VP] * 3 + [C.c_float] + [_VP] * 2 + [C.c_int64, C.c_int32, C.c_int32, _VP,
                                           C.c_int32, _VP]),
    "gnnrag_update_drop_backward_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "gnnrag_update_drop_backward": (C.c_int, [_VP] * 4 + [C.c_float, _VP, C.c_int64, C.c_int32, C.c_int32] + [_VP] * 5 +
                                    [C.c_size_t, C.c_int32, _VP]),
    # backward of the per-question relation tables (additive to ABI 16)
    "gnnrag_relation_tables_backward_workspace_bytes": (C.c_size_t, [C.POINTER(CsrStruct), C.c_int32, C.c_int32]),
    "gnnrag_relation_tables_backward": (C.c_int, [C.POINTER(CsrStruct)] + [_VP] * 9 + [C.c_int32] * 3 +
                                        [_VP, C.c_size_t, _VP]),
    # training loss and batch metrics (additive to ABI 16)
    "gnnrag_kl_loss_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "gnnrag_kl_loss_train": (C.c_int, [_VP] * 3 + [C.c_int32] * 2 + [_VP] * 3 + [C.c_size_t, _VP]),
    "gnnrag_kl_loss_backward": (C.c_int, [_VP] * 5 + [C.c_int32] * 2 + [_VP] * 2),
    "gnnrag_train_metrics": (C.c_int, [_VP] * 4 + [C.c_int64, C.c_double] + [C.c_int32] * 2 + [_VP] * 5),
    # frozen BERT-class question encoder, inference (additive to ABI 16)
    "gnnrag_bert_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "gnnrag_bert_attention": (C.c_int, [_VP] + [C.c_int32] * 4 + [_VP, _VP]),
    "gnnrag_bert_encode": (C.c_int, [_VP, _VP, C.c_int32, _VP, C.c_int32, _VP, _VP, _VP, C.c_float, C.c_int32,
                                     C.POINTER(BertLayer)] + [C.c_int32] * 5 + [_VP, _VP, C.c_size_t, C.c_int32, _VP]),
    # the same with RoBERTa / MPNet positions, no token-type term and MPNet's relative attention bias
    "gnnrag_bert_attention_bias": (C.c_int, [_VP] + [C.c_int32] * 4 + [_VP, _VP, _VP]),
    "gnnrag_bert_encode_ex": (C.c_int, [_VP, _VP, C.c_int32, _VP, C.c_int32, _VP, C.c_int32, _VP, _VP, _VP, C.c_float,
                                        C.c_int32, C.POINTER(BertLayer)] + [C.c_int32] * 5 +
                              [_VP, _VP, C.c_size_t, C.c_int32, _VP]),
    # the same encoder in training mode: the caller's dropout masks fused into the forward (additive to ABI 16)
    "gnnrag_bert_keep_hidden_bytes": (C.c_size_t, [C.c_int32] * 4),
    "gnnrag_bert_keep_att_bytes": (C.c_size_t, [C.c_int32] * 4),
    "gnnrag_bert_attention_drop": (C.c_int, [_VP] + [C.c_int32] * 4 + [_VP, _VP, C.c_float, _VP, _VP]),
    "gnnrag_bert_encode_train": (C.c_int, [_VP, _VP, C.c_int32, _VP, C.c_int32, _VP, C.c_int32, _VP, _VP, _VP, C.c_float,
                                           C.c_int32, C.POINTER(BertLayer)] + [C.c_int32] * 5 +
                                 [_VP, C.c_float, _VP, C.c_float, _VP, _VP, C.c_size_t, C.c_int32, _VP]),
    # fine-tuning the encoder: the layers' saving forward and their backward (additive to ABI 16)
    "gnnrag_bert_reserve_bytes": (C.c_size_t, [C.c_int32] * 5),
    "gnnrag_bert_layers_forward_save": (C.c_int, [_VP, C.c_int32, C.POINTER(BertLayer), C.c_float] + [C.c_int32] * 5 +
                                        [_VP, C.c_float, _VP, C.c_float, _VP, _VP, C.c_size_t, _VP, C.c_size_t, C.c_int32,
                                         _VP]),
    "gnnrag_bert_layers_backward_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "gnnrag_bert_layers_backward": (C.c_int, [_VP, C.c_int32, C.POINTER(BertLayer), C.c_float] + [C.c_int32] * 5 +
                                    [_VP, C.c_float, _VP, C.c_float, _VP, C.c_size_t, _VP, C.POINTER(BertLayerGrads), _VP,
                                     C.c_size_t, _VP]),
    "gnnrag_bert_attention_backward_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "gnnrag_bert_attention_backward": (C.c_int, [_VP, _VP] + [C.c_int32] * 4 + [_VP, C.c_float, _VP, _VP, C.c_size_t, _VP]),
    "gnnrag_bert_ln_backward": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, _VP, C.c_float, C.c_int64, C.c_int32] + [_VP] * 6),
    "gnnrag_bert_gelu_backward": (C.c_int, [_VP, _VP, C.c_int64, _VP, _VP, _VP]),
    # fine-tuning the whole encoder: the embedding stage and MPNet's relative bias (additive to ABI 16)
    "gnnrag_bert_embed_reserve_bytes": (C.c_size_t, [C.c_int32] * 3),
    "gnnrag_bert_embed_forward_save": (C.c_int, [_VP, _VP, C.c_int32, _VP, C.c_int32, _VP, C.c_int32, _VP, _VP, C.c_float] +
                                       [C.c_int32] * 3 + [_VP, C.c_float, _VP, _VP, C.c_size_t, _VP]),
    "gnnrag_bert_embed_backward_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "gnnrag_bert_embed_backward": (C.c_int, [_VP, _VP, _VP, C.c_size_t] + [C.c_int32] * 8 +
                                   [_VP, C.c_float, _VP, C.c_float] + [_VP] * 6 + [C.c_size_t, _VP]),
    "gnnrag_bert_layers_forward_save_ex": (C.c_int, [_VP, C.c_int32, C.POINTER(BertLayer), _VP, C.c_float] +
                                           [C.c_int32] * 5 + [_VP, C.c_float, _VP, C.c_float, _VP, _VP, C.c_size_t, _VP,
                                                              C.c_size_t, C.c_int32, _VP]),
    "gnnrag_bert_layers_backward_ex": (C.c_int, [_VP, C.c_int32, C.POINTER(BertLayer), _VP, C.c_float] + [C.c_int32] * 5 +
                                       [_VP, C.c_float, _VP, C.c_float, _VP, C.c_size_t, _VP, C.POINTER(BertLayerGrads),
                                        _VP, _VP, C.c_size_t, _VP]),
    "gnnrag_bert_attention_backward_bias": (C.c_int, [_VP, _VP] + [C.c_int32] * 4 +
                                            [_VP, _VP, C.c_float, _VP, _VP, C.c_size_t, _VP]),
    "gnnrag_bert_rel_bias_reduce": (C.c_int, [_VP] + [C.c_int32] * 3 + [_VP, _VP]),
    "gnnrag_bert_embed_scatter": (C.c_int, [_VP, _VP, _VP, C.c_int64] + [C.c_int32] * 5 + [_VP, _VP, _VP]),
    # split-K linear for few rows and the inference encoder on it (additive to ABI 16)
    "gnnrag_linear_splitk_plan": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(SplitkPlanStruct)]),
    "gnnrag_linear_splitk_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "gnnrag_linear_splitk": (C.c_int, [_VP, C.c_int64, C.c_int32, _VP, _VP, C.c_int32, _VP, _VP, _VP, C.c_float, _VP,
                                       C.c_int32, C.c_int32, _VP, C.c_size_t, _VP]),
    "gnnrag_bert_splitk_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "gnnrag_bert_encode_splitk": (C.c_int, [_VP, _VP, C.c_int32, _VP, C.c_int32, _VP, C.c_int32, _VP, _VP, _VP, C.c_float,
                                            C.c_int32, C.POINTER(BertLayer)] + [C.c_int32] * 5 +
                                  [_VP, _VP, C.c_size_t, C.c_int32, _VP]),
    # relation-text features (additive to ABI 16)
    "gnnrag_rel_text_workspace_bytes": (C.c_size_t, [C.c_int64] + [C.c_int32] * 4),
    "gnnrag_rel_text_pool": (C.c_int, [_VP] * 6 + [C.c_int64] + [C.c_int32] * 3 + [_VP] * 5 + [C.c_size_t, _VP]),
    "gnnrag_rel_text_backward_workspace_bytes": (C.c_size_t, [C.c_int64] + [C.c_int32] * 4),
    "gnnrag_rel_text_pool_backward": (C.c_int, [_VP] * 8 + [C.c_int64] + [C.c_int32] * 3 + [_VP] * 4 + [C.c_size_t, _VP]),
    # reasoning paths (additive to ABI 16)
    "gnnrag_ugraph_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "gnnrag_ugraph_scratch_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "gnnrag_ugraph_build": (C.c_int, [C.POINTER(CsrStruct), _VP, C.c_size_t, _VP, C.c_size_t, C.POINTER(UGraphStruct),
                                      _VP]),
    "gnnrag_paths_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "gnnrag_paths_out_bytes": (C.c_size_t, [C.c_int32] * 5),
    "gnnrag_shortest_paths": (C.c_int, [C.POINTER(UGraphStruct), _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "gnnrag_rule_paths_workspace_bytes": (C.c_size_t, [C.c_int64] + [C.c_int32] * 4),
    "gnnrag_rule_paths_out_bytes": (C.c_size_t, [C.c_int32] * 5),
    "gnnrag_rule_paths": (C.c_int, [C.POINTER(UGraphStruct), _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    # gradient-norm clip and Adam step (additive to ABI 16)
    "gnnrag_optim_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gnnrag_grad_norm": (C.c_int, [_VP, C.c_int32, C.c_int64, C.c_float, _VP, _VP, C.c_size_t, _VP]),
    "gnnrag_adam_step": (C.c_int, [_VP, C.c_int32, C.c_int64, _VP, _VP]),
    "gnnrag_stream_copy": (C.c_int, [_VP, _VP, C.c_int64, _VP]),
    "gnnrag_abi_version": (C.c_int, []),
    "gnnrag_error_string": (C.c_char_p, [C.c_int]),
}

ABI_VERSION = 16
PATH_AUTO, PATH_UNFUSED, PATH_FUSED = 0, 1, 2
PATH_ONLY_FWD, PATH_ONLY_INV = 0x10, 0x20        # OR-ed into the path: one-direction layers (NSM)
PATH_SEED_PRIOR = 0x40                           # OR-ed into the path: the (first layer's) prior is a seed distribution
PATH_REUSE_PROJ = 0x80                           # gnnrag_reason_stack: the workspace still holds the relation projections
E_TUPLE = -4
SPLITK_EPI = {"bias": 0, "gelu": 1, "add_ln": 2}   # GNNRAG_SPLITK_EPI_* (include/gnnrag.h)
SPLITK_MAX_SPLITS = 128                          # GNNRAG_SPLITK_MAX_SPLITS
_lib = None


class GnnragError(RuntimeError):
    pass


def load():
    """Loads the library once; raises if it is not built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("GNNRAG_LIB", LIB_PATH)     # experiment builds (tools/tune_variants.py)
    if not os.path.exists(path):
        raise GnnragError(
            "HIP extension %s is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)           # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.gnnrag_abi_version() != ABI_VERSION:
        raise GnnragError("ABI mismatch: library %d, binding %d" % (lib.gnnrag_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(code: int, what: str = ""):
    if code != 0:
        msg = load().gnnrag_error_string(code)
        err = GnnragError("%s failed (%d): %s" % (what or "gnnrag call", code,
                                                  msg.decode() if msg else "?"))
        err.code = code
        raise err
