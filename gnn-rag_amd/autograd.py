"""autograd bindings of the sparse operators.

Training (``Trainer_KBQA.train_epoch``, reference ``train_model.py:209-233``) differentiates
through ``reason_layer`` / ``reason_layer_inv`` (``reasongnn.py:61-116``) and ``TypeLayer``
(``layer_init.py:25-62``).  Here the typed-edge aggregation and its backward are HIP kernels
(``gnnrag_aggregate`` / ``gnnrag_aggregate_backward``, ``gnnrag_typelayer`` /
``gnnrag_typelayer_backward``); the dense projections around them run on the library's matrix-core kernels in
both directions (:class:`LinearFn`: ``gnnrag_linear`` for y and dx, ``gnnrag_gemm_tn`` for dW).  The question
encoder's LSTM trains on :class:`LstmFn` (``gnnrag_lstm_forward_train`` / ``gnnrag_lstm_backward``), the relation-text
features on :class:`RelTextPoolFn` (``gnnrag_rel_text_pool`` / ``gnnrag_rel_text_pool_backward``), instruction generation on
:class:`InstructionsFn` (``gnnrag_instructions_train`` / ``gnnrag_instructions_backward``), the instruction update between
two iterations on :class:`QueryReformFn` (``gnnrag_query_reform_train`` / ``gnnrag_query_reform_backward``), the tail of the
reasoning layer on :class:`LayerTailFn` (``gnnrag_layer_tail_train`` / ``gnnrag_layer_tail_backward``), the concatenated update under
dropout on :class:`UpdateDropFn` (``gnnrag_update_drop_train`` / ``gnnrag_update_drop_backward``), the KL loss behind
the last distribution on :class:`KLLossFn` (``gnnrag_kl_loss_train`` / ``gnnrag_kl_loss_backward``), the relation tables of
the fused training form on :class:`RelationTablesFn` (``gnnrag_relation_tables`` / ``gnnrag_relation_tables_backward``), the
layers of an unfrozen BERT-class question encoder on :class:`BertLayersFn` (``gnnrag_bert_layers_forward_save`` /
``gnnrag_bert_layers_backward``), with MPNet's relative bias on :class:`BertLayersBiasFn`, and the embedding stage in front
of them on :class:`BertEmbedFn` (``gnnrag_bert_embed_forward_save`` / ``gnnrag_bert_embed_backward``)."""
from __future__ import annotations

import torch

from torch.autograd.function import once_differentiable

from . import ops


class AggregateFn(torch.autograd.Function):
    """agg [BN, 2I*D] = typed-edge aggregation of all instructions, both directions."""

    @staticmethod
    def forward(ctx, plan, dist, ins, T_fwd, T_inv):
        dist = dist.detach().float().contiguous()
        ins = ins.detach().float().contiguous()
        T_fwd = T_fwd.detach().float().contiguous()
        T_inv = T_inv.detach().float().contiguous()
        ctx.plan = plan
        ctx.save_for_backward(dist, ins, T_fwd, T_inv)
        return ops.aggregate(plan, dist, ins, T_fwd, T_inv)

    @staticmethod
    def backward(ctx, g_agg):
        dist, ins, T_fwd, T_inv = ctx.saved_tensors
        g_dist, g_ins, g_Tf, g_Ti = ops.aggregate_backward(ctx.plan, dist, ins, T_fwd, T_inv,
                                                           g_agg.float().contiguous())
        return None, g_dist.view(ctx.plan.B, ctx.plan.N), g_ins, g_Tf, g_Ti


class FusedAggregateFn(torch.autograd.Function):
    """nbr [BN, D] = the fused walk over per-question relation tables P [2, rel_total, D] (``gnnrag_aggregate_fused``);
    backward on ``gnnrag_aggregate_fused_backward`` (gather kernels, fixed summation order)."""

    @staticmethod
    def forward(ctx, plan, dist, P):
        dist = dist.detach().float().contiguous()
        P = P.detach().float().contiguous()
        ctx.plan = plan
        ctx.save_for_backward(dist, P)
        return ops.aggregate_fused(plan, dist, P)

    @staticmethod
    def backward(ctx, g_nbr):
        dist, P = ctx.saved_tensors
        g_dist, g_P = ops.aggregate_fused_backward(ctx.plan, dist, P, g_nbr.float().contiguous())
        return None, g_dist.view(ctx.plan.B, ctx.plan.N), g_P


def relation_tables_dense(plan, T_fwd, T_inv, ins, W_e2e):
    """Differentiable per-question relation tables of the fused form in plain torch ops:
    P[d, (b, r), :] = sum_i W_e2e[:, (1 + 2 i + d) D : (2 + 2 i + d) D] . relu(T_d[r] * ins[b, i]) over the compact rows
    (question, relation in use) of the structure - a few ten thousand rows, where the per-fact form of the reference
    (reasongnn.py:71-79) has one row per fact.  [2, rel_total, D]."""
    rows = plan.rel_rows_device()
    b, r = rows[:, 0].long(), rows[:, 1].long()
    I, D = ins.shape[1], ins.shape[2]
    q = ins.index_select(0, b)                                             # [M, I, D]
    out = []
    for d, T in enumerate((T_fwd, T_inv)):
        z = torch.relu(T.index_select(0, r).unsqueeze(1) * q)             # [M, I, D]
        Wd = torch.stack([W_e2e[:, (1 + 2 * i + d) * D:(2 + 2 * i + d) * D] for i in range(I)])    # [I, D_out, D]
        out.append(torch.einsum("mik,iok->mo", z, Wd))
    return torch.stack(out)


class RelationTablesFn(torch.autograd.Function):
    """P [2, rel_total, D] = the per-question relation tables of the fused form on ``gnnrag_relation_tables`` (the bits of
    inference) / ``gnnrag_relation_tables_backward``: what :func:`relation_tables_dense` spells in torch ops, as ONE autograd
    node.  Saves T_fwd, T_inv, ins and W_e2e only - relu(T * ins) [M, I, D] is formed inside the products of both directions
    and never stored; an input that needs no gradient gets none computed."""

    @staticmethod
    def forward(ctx, plan, T_fwd, T_inv, ins, W_e2e):
        T_fwd, T_inv = T_fwd.detach().float().contiguous(), T_inv.detach().float().contiguous()
        ins, W_e2e = ins.detach().float().contiguous(), W_e2e.detach().float().contiguous()
        ctx.plan = plan
        ctx.save_for_backward(T_fwd, T_inv, ins, W_e2e)
        return ops.relation_tables(plan, T_fwd, T_inv, ins, W_e2e)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_P):
        T_fwd, T_inv, ins, W_e2e = ctx.saved_tensors
        nig = ctx.needs_input_grad
        if not any(nig[1:5]):
            return (None,) * 5
        # .contiguous() inside ops._chk also copies an expanded (stride-0) gradient, as P.sum().backward() delivers
        g = ops.relation_tables_backward(ctx.plan, T_fwd, T_inv, ins, W_e2e, g_P.float(), need_T_fwd=nig[1],
                                         need_T_inv=nig[2], need_ins=nig[3], need_W=nig[4])
        return None, g["g_T_fwd"], g["g_T_inv"], g["g_ins"], g["g_W"]


class TypeAggFn(torch.autograd.Function):
    """h0 [BN, D] = relu(sum over incident facts of v_f T[rel_f]) (both directions)."""

    @staticmethod
    def forward(ctx, plan, T, use_w_rel):
        T = T.detach().float().contiguous()
        h0 = ops.typelayer(plan, T, use_w_rel)
        ctx.plan = plan
        ctx.use_w_rel = use_w_rel
        ctx.save_for_backward(h0)
        return h0

    @staticmethod
    def backward(ctx, g_h0):
        (h0,) = ctx.saved_tensors
        g_pre = (g_h0.float() * (h0 > 0)).contiguous()
        return None, ops.typelayer_backward(ctx.plan, g_pre, ctx.use_w_rel), None


class LinearFn(torch.autograd.Function):
    """``y = act(x W^T + b)`` (``nn.Linear`` + optional ReLU) on the hand-written kernels, forward and backward:
    forward and ``dx = dy W`` are ``gnnrag_linear`` calls (the second with the transposed weight, a [K, Nout] copy of
    a few hundred KB), ``dW = dy^T x`` is ``gnnrag_gemm_tn``; ``db`` is a column sum.  x: [M, K] fp32 contiguous."""

    @staticmethod
    def forward(ctx, x, W, b, relu):
        x = x.detach().float().contiguous()
        Wd = W.detach().float().contiguous()
        y = ops.linear(x, Wd, None if b is None else b.detach().float().contiguous(), relu=relu)
        ctx.relu = relu
        ctx.has_bias = b is not None
        ctx.save_for_backward(x, Wd, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, W, y = ctx.saved_tensors
        g = gy.float()
        if ctx.relu:
            g = g * (y > 0)
        g = g.contiguous()
        gx = ops.linear(g, W.t().contiguous()) if ctx.needs_input_grad[0] else None
        gW = ops.gemm_tn(g, x) if ctx.needs_input_grad[1] else None
        gb = g.sum(dim=0) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return gx, gW, gb, None


def linear(x: torch.Tensor, W: torch.Tensor, b=None, relu: bool = False) -> torch.Tensor:
    """Differentiable ``act(x W^T + b)`` over the last dimension of x on :class:`LinearFn`."""
    shp = x.shape
    y = LinearFn.apply(x.reshape(-1, shp[-1]), W, b, relu)
    return y.view(*shp[:-1], W.shape[0])


class LstmFn(torch.autograd.Function):
    """``out, h_n, c_n = LSTM(x, (h0, c0))`` (one layer, one direction, batch_first; ``nn.LSTM`` semantics) on
    ``gnnrag_lstm_forward_train`` / ``gnnrag_lstm_backward``.  h0 / c0: [B, H] or None (zeros).  The reserve (activated
    gates and cell states) is saved in the context of THIS call - a module called twice inside one graph has two;
    ``workspaces`` is the caller's dict for the transposed-weight scratch (see :func:`ops.lstm_forward`)."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, h0, c0, workspaces):
        x = x.detach().float()
        h0 = None if h0 is None else h0.detach().float()
        c0 = None if c0 is None else c0.detach().float()
        out, h_n, c_n, reserve = ops.lstm_forward_train(x, w_ih, w_hh, b_ih, b_hh, h0, c0, workspaces=workspaces)
        ctx.set_materialize_grads(False)            # an unused output arrives as None and goes to the library as NULL
        ctx.save_for_backward(x, w_ih.detach(), w_hh.detach(), h0, c0, out, reserve)
        return out, h_n, c_n

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_hn, g_cn):
        x, w_ih, w_hh, h0, c0, out, reserve = ctx.saved_tensors
        need = ctx.needs_input_grad
        # .contiguous() inside ops._chk also copies an expanded (stride-0) gradient, as out.sum().backward() delivers
        g_out, g_hn, g_cn = (None if g is None else g.float() for g in (g_out, g_hn, g_cn))
        dx, dw_ih, dw_hh, db, dh0, dc0 = ops.lstm_backward(x, w_ih, w_hh, h0, c0, out, reserve, g_out, g_hn, g_cn,
                                                           need_dx=need[0], need_db=need[3] or need[4],
                                                           need_dh0=need[5], need_dc0=need[6])
        # b_ih and b_hh get the same values in two tensors (their .grad must not share memory)
        return (dx, dw_ih if need[1] else None, dw_hh if need[2] else None, db if need[3] else None,
                (db.clone() if need[3] else db) if need[4] else None, dh0, dc0, None)


class RelTextPoolFn(torch.autograd.Function):
    """``out_fwd, out_inv = AttnEncoder(question_emb(X), mask)`` of the relation-text branch (rearev.py:101-106; X_inv None:
    one direction, nsm.py:103-105, and ``out_inv`` is None) on ``gnnrag_rel_text_pool`` / ``gnnrag_rel_text_pool_backward``.
    W, b = ``question_emb``, a = ``attn_linear.weight``.  xbar and alpha are saved in the context of THIS call.  X (the
    frozen LM states) and the mask never receive a gradient."""

    @staticmethod
    def forward(ctx, X_fwd, X_inv, mask, W, b, a):
        X_fwd = X_fwd.detach()
        X_inv = None if X_inv is None else X_inv.detach()
        need = any(ctx.needs_input_grad[3:6])
        out_fwd, out_inv, xbar, alpha = ops.rel_text_pool(X_fwd, X_inv, mask.detach(), W, b, a, save=need)
        ctx.set_materialize_grads(False)            # an unused output arrives as None and goes to the library as NULL
        ctx.two = X_inv is not None
        ctx.a_shape = a.shape
        if need:
            ctx.save_for_backward(X_fwd, X_inv, W.detach(), a.detach(), xbar, alpha)
        return out_fwd, out_inv

    @staticmethod
    @once_differentiable
    def backward(ctx, g_fwd, g_inv):
        X_fwd, X_inv, W, a, xbar, alpha = ctx.saved_tensors
        need = ctx.needs_input_grad
        g_fwd = None if g_fwd is None else g_fwd.float()
        g_inv = None if (g_inv is None or not ctx.two) else g_inv.float()
        dW, db, da = ops.rel_text_pool_backward(X_fwd, X_inv, W, a, xbar, alpha, g_fwd, g_inv, need_dW=need[3],
                                                need_db=need[4], need_da=need[5])
        return None, None, None, dW, db, None if da is None else da.view(ctx.a_shape)


class InstructionsFn(torch.autograd.Function):
    """``ins [n,B,D], attn [n,B,T]`` = n chained ``get_instruction`` steps (base_encoder.py:82-101) on
    ``gnnrag_instructions_train`` / ``gnnrag_instructions_backward``.  r_in [B,D] or None (zeros); drop_node / drop_cat /
    drop_tok: the multipliers of ``linear_drop`` or None (see :func:`ops.instructions_train`); ``lin``: the steps'
    ``question_linear`` weights, then their biases (2 n tensors).  The reserve and the multipliers are saved in the context
    of THIS call.  The mask and the multipliers never receive a gradient."""

    @staticmethod
    def forward(ctx, hidden, node, mask, r_in, W_cq, b_cq, w_ca, b_ca, drop_node, drop_cat, drop_tok, *lin):
        n = len(lin) // 2
        W_q, b_q = list(lin[:n]), list(lin[n:])
        hidden, node = hidden.detach().float(), node.detach().float()
        r_in = None if r_in is None else r_in.detach().float()
        ins, attn, reserve = ops.instructions_train(hidden, node, mask.detach(), W_q, b_q, W_cq, b_cq, w_ca, b_ca, r_in=r_in,
                                                    drop_node=drop_node, drop_cat=drop_cat, drop_tok=drop_tok)
        ctx.set_materialize_grads(False)            # an unused output arrives as None and goes to the library as NULL
        ctx.n, ctx.w_ca_shape, ctx.b_ca_shape = n, w_ca.shape, b_ca.shape
        ctx.save_for_backward(hidden, node, r_in, W_cq.detach(), w_ca.detach(), drop_node, drop_cat, drop_tok, ins, attn,
                              reserve, *[w.detach() for w in W_q])
        return ins, attn

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ins, g_attn):
        hidden, node, r_in, W_cq, w_ca, drop_node, drop_cat, drop_tok, ins, attn, reserve = ctx.saved_tensors[:11]
        W_q = list(ctx.saved_tensors[11:])
        n, nig = ctx.n, ctx.needs_input_grad
        need = {"dhidden": nig[0], "dnode": nig[1], "dr_in": nig[3] and r_in is not None, "dW_cq": nig[4], "db_cq": nig[5],
                "dw_ca": nig[6], "db_ca": nig[7], "dW_q": list(nig[11:11 + n]), "db_q": list(nig[11 + n:11 + 2 * n])}
        # .contiguous() inside ops._chk also copies an expanded (stride-0) gradient, as ins.sum().backward() delivers
        g_ins, g_attn = (None if g is None else g.float() for g in (g_ins, g_attn))
        g = ops.instructions_backward(hidden, node, W_q, W_cq, w_ca, ins, attn, reserve, g_ins, g_attn, r_in=r_in,
                                      drop_node=drop_node, drop_cat=drop_cat, drop_tok=drop_tok, need=need)
        view = lambda t, shape: None if t is None else t.view(shape)      # noqa: E731
        return (g["dhidden"], g["dnode"], None, g["dr_in"], g["dW_cq"], g["db_cq"], view(g["dw_ca"], ctx.w_ca_shape),
                view(g["db_ca"], ctx.b_ca_shape), None, None, None, *g["dW_q"], *g["db_q"])


class QueryReformFn(torch.autograd.Function):
    """``out_0 .. out_{n-1}`` [B,D] = the n reforms of one ReaRev iteration (rearev.py:217-221; query_update.py:26-44) on
    ``gnnrag_query_reform_train`` / ``gnnrag_query_reform_backward``.  ``rest``: the reforms' instructions [B,D], then their
    ``fusion.r.weight``, then their ``fusion.g.weight`` (3 n tensors).  ent_emb [B,N,D] is the shared node state: it gets ONE
    dense gradient (the reforms' seed-row gradients added inside the kernel), and none is computed when it needs none.  The
    reserve is saved in the context of THIS call.  ``seed_info`` never receives a gradient."""

    @staticmethod
    def forward(ctx, seed_info, ent_emb, *rest):
        n = len(rest) // 3
        qs = [q.detach().float() for q in rest[:n]]
        W_rs, W_gs = [w.detach() for w in rest[n:2 * n]], [w.detach() for w in rest[2 * n:]]
        seed_info = seed_info.detach()
        out, reserve = ops.query_reform_train(qs, seed_info, ent_emb.detach(), W_rs, W_gs)
        ctx.set_materialize_grads(False)            # an unused output arrives as None and goes to the library as NULL
        ctx.n, ctx.ent_width = n, ent_emb.shape[2]
        ctx.save_for_backward(seed_info, reserve, *qs, *W_rs, *W_gs)
        return tuple(out.unbind(0))

    @staticmethod
    @once_differentiable
    def backward(ctx, *g_outs):
        n, nig = ctx.n, ctx.needs_input_grad
        seed_info, reserve = ctx.saved_tensors[:2]
        qs, W_rs, W_gs = (list(ctx.saved_tensors[2 + k * n:2 + (k + 1) * n]) for k in range(3))
        need = {"d_ent": nig[1], "dq": list(nig[2:2 + n]), "dW_r": list(nig[2 + n:2 + 2 * n]),
                "dW_g": list(nig[2 + 2 * n:2 + 3 * n])}
        # .contiguous() inside ops._chk also copies an expanded (stride-0) gradient, as out.sum().backward() delivers
        g_outs = [None if g is None else g.float() for g in g_outs]
        if all(g is None for g in g_outs):
            return (None,) * (2 + 3 * n)
        g = ops.query_reform_backward(qs, seed_info, W_rs, W_gs, reserve, g_outs, need=need)
        d_ent = g["d_ent"]
        if d_ent is not None and ctx.ent_width != d_ent.shape[2]:       # a node state wider than the instructions
            d_ent = torch.nn.functional.pad(d_ent, (0, ctx.ent_width - d_ent.shape[2]))
        return (None, d_ent, *g["dq"], *g["dW_r"], *g["dW_g"])


class LayerTailFn(torch.autograd.Function):
    """``(h, score, dist)`` = the tail of the reasoning layer (reasongnn.py:163-169) on ``gnnrag_layer_tail_train`` /
    ``gnnrag_layer_tail_backward``: pre_a, pre_b [B*N,D] (pre_b may be None) the pre-activations, keep [B*N,D] uint8 / scale
    the dropout in front of the score function (keep None: none), w = ``score_func.weight`` [1,D], b = ``score_func.bias``
    [1], mask [B,N].  ``score`` is not differentiable (the reference hands it out with ``return_score`` only, and the module
    keeps that case on torch); pre_a and pre_b receive the one gradient buffer the library writes."""

    @staticmethod
    def forward(ctx, pre_a, pre_b, keep, scale, w, b, mask):
        wd = w.detach().float().reshape(-1)
        h, score, dist = ops.layer_tail_train(pre_a.detach(), None if pre_b is None else pre_b.detach(), keep, scale, wd,
                                              b.detach().float(), mask.detach())
        ctx.mark_non_differentiable(score)
        ctx.set_materialize_grads(False)            # an unused h or dist arrives as None and goes to the library as NULL
        ctx.scale, ctx.has_keep, ctx.has_b = float(scale), keep is not None, pre_b is not None
        ctx.w_shape, ctx.b_shape = w.shape, b.shape
        ctx.save_for_backward(h, dist, wd, *([keep] if keep is not None else []))
        return h, score, dist

    @staticmethod
    @once_differentiable
    def backward(ctx, g_h, _g_score, g_dist):
        if g_h is None and g_dist is None:
            return (None,) * 7
        h, dist, wd = ctx.saved_tensors[:3]
        keep = ctx.saved_tensors[3] if ctx.has_keep else None
        nig = ctx.needs_input_grad
        # .contiguous() inside ops._chk also copies an expanded (stride-0) gradient, as h.sum().backward() delivers
        g = ops.layer_tail_backward(h, dist, keep, ctx.scale, wd, None if g_h is None else g_h.float(),
                                    None if g_dist is None else g_dist.float(), need_dw=nig[4], need_db=nig[5])
        g_pre = g["g_pre"]
        return (g_pre if nig[0] else None, g_pre if (ctx.has_b and nig[1]) else None, None, None,
                None if g["dw"] is None else g["dw"].view(ctx.w_shape), None if g["db"] is None else g["db"].view(ctx.b_shape),
                None)


class UpdateDropFn(torch.autograd.Function):
    """``pre = e2e_linear(linear_drop(cat(h, agg)))`` (reasongnn.py:161-163 in training) on ``gnnrag_update_drop_train`` /
    ``gnnrag_update_drop_backward``: h [B*N,D], agg [B*N,2*I*D], keep [B*N,(2I+1)D] uint8 / scale the dropout (keep None: none),
    W [D,(2I+1)D], b [D].  Saves h, agg, keep and W - not the dropped operand, which neither direction ever stores; h, agg,
    W and b receive the gradients ``needs_input_grad`` asks for, an output nobody asks for is not computed."""

    @staticmethod
    def forward(ctx, h, agg, keep, scale, W, b):
        h, agg = h.detach().float().contiguous(), agg.detach().float().contiguous()
        Wd = W.detach().float().contiguous()
        pre = ops.update_drop_train(h, agg, keep, scale, Wd, b.detach().float().contiguous())
        ctx.scale, ctx.has_keep = float(scale), keep is not None
        ctx.save_for_backward(h, agg, Wd, *([keep] if keep is not None else []))
        return pre

    @staticmethod
    @once_differentiable
    def backward(ctx, g_pre):
        h, agg, Wd = ctx.saved_tensors[:3]
        keep = ctx.saved_tensors[3] if ctx.has_keep else None
        nig = ctx.needs_input_grad
        if not (nig[0] or nig[1] or nig[4] or nig[5]):
            return (None,) * 6
        # .contiguous() inside ops._chk also copies an expanded (stride-0) gradient, as pre.sum().backward() delivers
        g = ops.update_drop_backward(g_pre.float(), h, agg, keep, ctx.scale, Wd, need_h=nig[0], need_agg=nig[1],
                                     need_dW=nig[4], need_db=nig[5])
        return g["g_h"], g["g_agg"], None, None, g["dW"], g["db"]


class KLLossFn(torch.autograd.Function):
    """``loss`` = ``calc_loss_label`` with ``loss_type='kl'`` (rearev.py:156-160 over base_model.py:193-215) on
    ``gnnrag_kl_loss_train`` / ``gnnrag_kl_loss_backward``: pred, teacher [B,N], label_valid [B] or [B,1].  Returns the 0-dim
    batch-mean loss; saves pred, teacher, label_valid and the reserve (the answer counts).  Only pred receives a gradient:
    the module keeps a teacher that asks for one on torch.  The upstream gradient stays on the device."""

    @staticmethod
    def forward(ctx, pred, teacher, label_valid):
        pred, teacher, label_valid = pred.detach(), teacher.detach(), label_valid.detach().reshape(-1)
        loss, reserve = ops.kl_loss_train(pred, teacher, label_valid)
        ctx.save_for_backward(pred, teacher, label_valid, reserve)
        return loss.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        pred, teacher, label_valid, reserve = ctx.saved_tensors
        return ops.kl_loss_backward(g_loss.float().reshape(1), pred, teacher, label_valid, reserve), None, None


BERT_LAYER_PARAMS = 16      # per layer: query / key / value weights, their biases, then W_o, b_o, ln1_g, ln1_b, W_i .. ln2_b


class BertLayersFn(torch.autograd.Function):
    """``out [B,T,H]`` = the encoder layers of a BERT-class LM on ``x0 [B,T,H]`` (the output of the embedding stage, which
    stays transformers' module) on ``gnnrag_bert_layers_forward_save`` / ``gnnrag_bert_layers_backward``.  ``params``: per
    layer the ``BERT_LAYER_PARAMS`` tensors - the separate query / key / value weights, their biases, then W_o, b_o, ln1_g,
    ln1_b, W_i, b_i, W_f, b_f, ln2_g, ln2_b.  The packed ``W_qkv`` / ``b_qkv`` are built here and their gradients go back
    as their three row blocks (the key bias block is exactly zero, see the header).  ``keep_hidden`` / ``keep_att``: the
    keep bytes of ``ops.bert_keep_shapes`` or None; they never receive a gradient.  The reserve, the masks and the packed
    weights are saved in the context of THIS call: two encodes followed by one backward each read their own."""

    @staticmethod
    def forward(ctx, x0, keep_hidden, scale_hidden, keep_att, scale_att, heads, eps, *params):
        return _bert_layers_forward(ctx, x0, None, keep_hidden, scale_hidden, keep_att, scale_att, heads, eps, params)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        g_x0, _, per_param = _bert_layers_backward(ctx, g_out, first=7, want_bias=False)
        return (g_x0, None, None, None, None, None, None) + per_param


class BertLayersBiasFn(torch.autograd.Function):
    """:class:`BertLayersFn` with MPNet's relative attention bias: ``rel_bias [heads, 2T-1]`` (entry ``[h, j - i + T - 1]``
    is added to the scaled score of query i and key j in every layer) is the second, differentiable input, on
    ``gnnrag_bert_layers_forward_save_ex`` / ``gnnrag_bert_layers_backward_ex``.  Its gradient is one table summed over the
    layers; it is computed only when the input needs it."""

    @staticmethod
    def forward(ctx, x0, rel_bias, keep_hidden, scale_hidden, keep_att, scale_att, heads, eps, *params):
        return _bert_layers_forward(ctx, x0, rel_bias.detach().contiguous(), keep_hidden, scale_hidden, keep_att,
                                    scale_att, heads, eps, params)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        g_x0, d_bias, per_param = _bert_layers_backward(ctx, g_out, first=8, want_bias=ctx.needs_input_grad[1])
        return (g_x0, d_bias, None, None, None, None, None, None) + per_param


def _bert_layers_forward(ctx, x0, rel_bias, keep_hidden, scale_hidden, keep_att, scale_att, heads, eps, params):
    """The forward of :class:`BertLayersFn` (``rel_bias`` None) and :class:`BertLayersBiasFn`."""
    L = len(params) // BERT_LAYER_PARAMS
    if L < 1 or L * BERT_LAYER_PARAMS != len(params):
        raise ValueError("BertLayersFn: %d tensors per layer" % BERT_LAYER_PARAMS)
    B, T, H = x0.shape
    layers = []
    for l in range(L):
        p = [t.detach() for t in params[BERT_LAYER_PARAMS * l: BERT_LAYER_PARAMS * (l + 1)]]
        layers.append(dict(zip(ops.BERT_LAYER_FIELDS, [torch.cat(p[0:3], 0).contiguous(),
                                                       torch.cat(p[3:6], 0).contiguous()] + p[6:])))
    out, reserve = ops.bert_layers_forward_save(x0.detach(), layers, int(heads), float(eps), B, T,
                                                keep_hidden=keep_hidden, scale_hidden=scale_hidden,
                                                keep_att=keep_att, scale_att=scale_att, rel_bias=rel_bias)
    ctx.meta = (B, T, H, L, int(heads), float(eps), float(scale_hidden), float(scale_att))
    ctx.save_for_backward(reserve, keep_hidden, keep_att, rel_bias,
                          *[layer[n] for layer in layers for n in ops.BERT_LAYER_FIELDS])
    return out


def _bert_layers_backward(ctx, g_out, first, want_bias):
    """``(g_x0, d_rel_bias, the per-parameter gradients)`` of the two Functions; ``first``: the index of the first layer
    parameter among the Function's inputs."""
    B, T, H, L, heads, eps, scale_hidden, scale_att = ctx.meta
    reserve, keep_hidden, keep_att, rel_bias = ctx.saved_tensors[:4]
    flat, nf = ctx.saved_tensors[4:], len(ops.BERT_LAYER_FIELDS)
    layers = [dict(zip(ops.BERT_LAYER_FIELDS, flat[nf * l: nf * (l + 1)])) for l in range(L)]
    nig = ctx.needs_input_grad
    need = []
    for l in range(L):
        n = nig[first + BERT_LAYER_PARAMS * l: first + BERT_LAYER_PARAMS * (l + 1)]
        d = {"dW_qkv": any(n[0:3]), "db_qkv": any(n[3:6])}
        d.update({"d" + name: n[4 + i] for i, name in enumerate(ops.BERT_LAYER_FIELDS) if i >= 2})
        need.append(d)
    res = ops.bert_layers_backward(g_out.float(), layers, heads, eps, B, T, reserve, keep_hidden=keep_hidden,
                                   scale_hidden=scale_hidden, keep_att=keep_att, scale_att=scale_att,
                                   need_x0=nig[0], need=need, rel_bias=rel_bias, want_rel_bias_grad=bool(want_bias))
    g_x0, grads, d_bias = res if want_bias else res + (None,)
    ret = []
    for l in range(L):
        g, n = grads[l], nig[first + BERT_LAYER_PARAMS * l: first + BERT_LAYER_PARAMS * (l + 1)]
        for packed, lo in ((g["dW_qkv"], 0), (g["db_qkv"], 3)):
            ret += [packed[H * k: H * (k + 1)] if packed is not None and n[lo + k] else None for k in range(3)]
        ret += [g["d" + name] for name in ops.BERT_LAYER_FIELDS[2:]]
    return g_x0, d_bias, tuple(ret)


class BertEmbedFn(torch.autograd.Function):
    """``x0 [B,T,H]`` = the embedding stage of a BERT-class LM - the lookups, the positions (``pad_id`` None: 0 .. T-1, else
    counted from the ids), the LayerNorm and the dropout of keep plane 0 (``keep`` uint8 [B*T,H] or None) - on
    ``gnnrag_bert_embed_forward_save`` / ``gnnrag_bert_embed_backward``.  Differentiable inputs: ``word_emb``, ``pos_emb``,
    ``type_emb`` (None for an encoder without a token-type term), ``ln_g``, ``ln_b``; a table's gradient is dense, with the
    rows ``word_pad`` / ``pos_pad`` (transformers' ``padding_idx``, or None) exactly zero.  The reserve belongs to the
    context of THIS call."""

    @staticmethod
    def forward(ctx, ids, keep, scale, pad_id, word_pad, pos_pad, eps, word_emb, pos_emb, type_emb, ln_g, ln_b):
        x0, reserve = ops.bert_embed_forward_save(ids, word_emb, pos_emb, type_emb, ln_g, ln_b, float(eps), pad_id=pad_id,
                                                  keep=keep, scale=scale)
        ctx.meta = (float(scale), word_pad, pos_pad, float(eps), int(word_emb.shape[0]), int(pos_emb.shape[0]),
                    0 if type_emb is None else int(type_emb.shape[0]))
        ctx.save_for_backward(ids, reserve, keep, ln_g.detach())
        return x0

    @staticmethod
    @once_differentiable
    def backward(ctx, g_x0):
        scale, word_pad, pos_pad, eps, vocab, max_pos, n_type = ctx.meta
        ids, reserve, keep, ln_g = ctx.saved_tensors
        need = dict(zip(ops.BERT_EMBED_GRADS, ctx.needs_input_grad[7:12]))
        g = ops.bert_embed_backward(g_x0.float().contiguous(), ids, reserve, ln_g, eps, vocab, max_pos, n_type,
                                    word_pad=word_pad, pos_pad=pos_pad, keep=keep, scale=scale, need=need)
        return (None,) * 7 + tuple(g[n] for n in ops.BERT_EMBED_GRADS)
