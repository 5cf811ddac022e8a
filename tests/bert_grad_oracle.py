"""Oracle of the fine-tuning tests of the LM question encoder (a helper, not a test): transformers' own ``BertModel`` /
``RobertaModel`` in float64 and in fp32, in TRAINING mode, UNDER AUTOGRAD, with ``torch.nn.functional.dropout`` replaced for
the duration of one call by the injected masks - the mechanism of ``bert_dropout_oracle.run`` without its ``no_grad``.

``grads`` returns every parameter gradient and the gradient of the embedding stage's output (the layers' input ``x0``) for a
given upstream gradient.  The float64 module is the oracle; the fp32 module on the same ids, masks and upstream gradient
gives ``e_ref`` of ``bert_oracle.bound`` per gradient tensor.  Nothing here is derived from the code under test.

Also the numpy float64 statements of the three backward kernels: attention, LayerNorm, GELU."""
import math

import numpy as np
import torch

import bert_oracle as bo


def forward(model, ids, masks, scale_hidden=1.0, scale_att=1.0):
    """``(out, x0)`` of ``model`` in training mode under autograd with ``F.dropout`` replaced as in
    ``bert_dropout_oracle.run``: out = last_hidden_state, x0 = the output of ``model.embeddings`` (behind its dropout),
    kept with ``retain_grad``.  The model is returned to the mode it was in."""
    import torch.nn.functional as F
    todo = list(masks)
    orig, was_training = F.dropout, model.training
    dtype = next(model.parameters()).dtype
    seen = {}

    def replacement(x, p=0.5, training=True, inplace=False):
        assert training and todo, "an unexpected dropout call"
        keep = todo.pop(0)
        if keep is None:
            return x
        assert tuple(keep.shape) == tuple(x.shape), (keep.shape, tuple(x.shape))
        return x * torch.from_numpy(keep).to(dtype) * (scale_att if x.dim() == 4 else scale_hidden)

    def hook(_mod, _inp, out):
        out.retain_grad()
        seen["x0"] = out

    handle = model.embeddings.register_forward_hook(hook)
    F.dropout = replacement
    try:
        model.train()
        out = model(torch.from_numpy(np.asarray(ids, dtype=np.int64)))[0]
    finally:
        F.dropout = orig
        handle.remove()
        model.train(was_training)
    assert not todo, "%d masks were not consumed" % len(todo)
    return out, seen["x0"]


def grads(model, calls, g_outs):
    """Parameter gradients of ``sum_c (out_c * g_out_c).sum()`` over the calls ``(ids, masks, scale_hidden, scale_att)``:
    ``{name: numpy array or None}`` over ``named_parameters`` plus ``"x0"`` / ``"g_x0"`` lists (one per call): the embedding
    stage's output and its gradient.  ``.grad`` of the model is cleared before and after."""
    dtype = next(model.parameters()).dtype
    model.zero_grad(set_to_none=True)
    x0s, total = [], None
    for (ids, masks, sh, sa), g in zip(calls, g_outs):
        out, x0 = forward(model, ids, masks, sh, sa)
        x0s.append(x0)
        term = (out * torch.from_numpy(np.asarray(g)).to(dtype)).sum()
        total = term if total is None else total + term
    total.backward()
    res = {name: (None if p.grad is None else p.grad.detach().numpy().copy()) for name, p in model.named_parameters()}
    res["x0"] = [x.detach().numpy().copy() for x in x0s]
    res["g_x0"] = [x.grad.detach().numpy().copy() for x in x0s]
    model.zero_grad(set_to_none=True)
    return res


def layer_names(model, l):
    """``BERT_GRAD_FIELDS`` -> the parameter name(s) of layer ``l`` (a list of three for the packed QKV gradients)."""
    p = "encoder.layer.%d." % l
    s, ao = p + "attention.self.", p + "attention.output."
    return {"dW_qkv": [s + "query.weight", s + "key.weight", s + "value.weight"],
            "db_qkv": [s + "query.bias", s + "key.bias", s + "value.bias"],
            "dW_o": ao + "dense.weight", "db_o": ao + "dense.bias", "dln1_g": ao + "LayerNorm.weight",
            "dln1_b": ao + "LayerNorm.bias", "dW_i": p + "intermediate.dense.weight", "db_i": p + "intermediate.dense.bias",
            "dW_f": p + "output.dense.weight", "db_f": p + "output.dense.bias", "dln2_g": p + "output.LayerNorm.weight",
            "dln2_b": p + "output.LayerNorm.bias"}


def compare(got, G64, G32, name, worst=None):
    """Asserts ``rel_err(got, G64[name]) <= bound(e_ref)`` with ``e_ref`` the fp32 module's own error on that tensor;
    prints the figures first and keeps the largest err / e_ref in ``worst`` (a one-element list)."""
    want, ref = G64[name], G32[name]
    assert want is not None, name
    if np.abs(want).max() == 0:
        # one token: the softmax of a single key is 1 whatever the score, so the query / key gradients are identically
        # zero in float64; a relative error has no meaning there and the library must give exactly 0 as well
        print("%-52s identically zero in float64" % name)
        assert np.all(np.asarray(got) == 0), name
        return
    err, e_ref = bo.rel_err(got, want), bo.rel_err(ref, want)
    print("%-52s err %.3g e_ref %.3g ratio %.2f" % (name, err, e_ref, err / max(e_ref, 1e-30)))
    if worst is not None:
        worst[0] = max(worst[0], err / max(e_ref, 1e-30))
    assert err <= bo.bound(e_ref), (name, err, e_ref)


# ---- numpy float64 statements of the three kernels ------------------------------------------------------------------

def attention_bwd64(qkv, d_ctx, B, T, heads, dh, keep=None, scale=1.0):
    """d_qkv [B*T, 3*heads*dh] of ``ctx = (softmax(q k^T / sqrt(dh)) * keep * scale) v`` for the upstream ``d_ctx``."""
    x = np.asarray(qkv, dtype=np.float64).reshape(B, T, 3, heads, dh)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    do = np.asarray(d_ctx, dtype=np.float64).reshape(B, T, heads, dh)
    s = np.einsum("bihd,bjhd->bhij", q, k) / np.sqrt(dh)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    m = np.ones_like(p) if keep is None else np.asarray(keep, dtype=np.float64) * float(scale)
    pt = p * m
    dpt = np.einsum("bihd,bjhd->bhij", do, v)
    ds = p * (dpt * m - (pt * dpt).sum(-1, keepdims=True))
    dq = np.einsum("bhij,bjhd->bihd", ds, k) / np.sqrt(dh)
    dk = np.einsum("bhij,bihd->bjhd", ds, q) / np.sqrt(dh)
    dv = np.einsum("bhij,bihd->bjhd", pt, do)
    return np.stack([dq, dk, dv], axis=2).reshape(B * T, 3 * heads * dh)


def ln_bwd64(dy, d, g, eps, keep=None, scale=1.0, res=None):
    """``(dz, dY, dgamma, dbeta)`` of ``y = LN(z) g + b`` with z = d * keep * scale + res (or z = d), biased variance."""
    dy, d, g = (np.asarray(a, dtype=np.float64) for a in (dy, d, g))
    m = None if keep is None else np.asarray(keep, dtype=np.float64) * float(scale)
    z = d if m is None else d * m + np.asarray(res, dtype=np.float64)
    mean = z.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((z - mean) ** 2).mean(-1, keepdims=True) + eps)
    xh = (z - mean) * rstd
    a = dy * g
    dz = rstd * (a - a.mean(-1, keepdims=True) - xh * (a * xh).mean(-1, keepdims=True))
    return dz, (dz if m is None else dz * m), (dy * xh).sum(0), dy.sum(0)


def gelu_bwd64(pre, d_act):
    """``(d_pre, gelu(pre))`` of the erf GELU."""
    x, gy = np.asarray(pre, dtype=np.float64), np.asarray(d_act, dtype=np.float64)
    erf = np.vectorize(math.erf)
    cdf = 0.5 * (1.0 + erf(x / math.sqrt(2.0)))
    return gy * (cdf + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)), x * cdf
