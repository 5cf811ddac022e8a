"""Float64 numpy restatement of the training form of the instruction steps and of its backward, with explicit dropout
multipliers (m1 [n,B,D] on the node state, m2 [n,B,4D] on the concatenation, m3 [n,B,T,D] on the token products; None = ones),
shared by tests/test_instruction_train_host.py and tests/test_gpu_instruction_train*.py.  The cases come from
tests/instruction_oracle.py.

    n_s  = node * m1                        q  = W_q[s] n_s + b_q[s]
    z    = [r, q, q - r, q * r] * m2        cq = W_cq z + b_cq
    ca_t = sum_d w_ca[d] cq[d] h[t,d] m3[t,d] + b_ca
    a    = softmax_t(ca_t + (1 - mask_t) * VERY_NEG)        r' = sum_t a_t h[t,:]

The mask addition is straight-through: in fp32 a padded logit IS the constant VERY_NEG (instruction_oracle.py), yet autograd
passes the gradient through the addition with derivative 1 - so the backward below treats every logit, padded or not, as
ca_t plus a constant.  db_ca is exactly zero (the softmax does not move under a shift) and is returned as such."""
import numpy as np

from instruction_oracle import VERY_NEG

GRADS = ("dhidden", "dnode", "dr_in", "dW_q", "db_q", "dW_cq", "db_cq", "dw_ca", "db_ca")


def _f(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def forward(hidden, node, mask, W_q, b_q, W_cq, b_cq, w_ca, b_ca, r_in=None, m1=None, m2=None, m3=None):
    """(ins [n,B,D], attn [n,B,T], saved) in float64; ``saved`` is what :func:`backward` reads."""
    hidden, node, mask, W_cq, b_cq = _f(hidden), _f(node), _f(mask), _f(W_cq), _f(b_cq)
    w_ca, b_ca = _f(w_ca).reshape(-1), float(_f(b_ca).reshape(-1)[0])
    W_q, b_q = [_f(w) for w in W_q], [_f(b) for b in b_q]
    m1, m2, m3 = _f(m1), _f(m2), _f(m3)
    B, T, D = hidden.shape
    r = np.zeros((B, D)) if r_in is None else _f(r_in)
    ins, attn, steps = [], [], []
    for s, (W, b) in enumerate(zip(W_q, b_q)):
        n_s = node if m1 is None else node * m1[s]
        q = n_s @ W.T + b
        z = np.concatenate([r, q, q - r, q * r], axis=1)
        if m2 is not None:
            z = z * m2[s]
        cq = z @ W_cq.T + b_cq
        hm = hidden if m3 is None else hidden * m3[s]
        ca = np.einsum("d,bd,btd->bt", w_ca, cq, hm) + b_ca
        assert np.abs(ca).max() < 4096.0
        logit = np.where(mask != 0, ca, VERY_NEG)
        e = np.exp(logit - logit.max(axis=1, keepdims=True))
        a = e / e.sum(axis=1, keepdims=True)
        steps.append(dict(r=r, n_s=n_s, q=q, z=z, cq=cq, hm=hm, a=a, m3=None if m3 is None else m3[s]))
        r = np.einsum("bt,btd->bd", a, hidden)
        ins.append(r)
        attn.append(a)
    saved = dict(hidden=hidden, W_q=W_q, W_cq=W_cq, w_ca=w_ca, m1=m1, m2=m2, steps=steps)
    return np.stack(ins), np.stack(attn), saved


def backward(saved, g_ins=None, g_attn=None):
    """The gradients of ``sum(ins * g_ins) + sum(attn * g_attn)`` (None = zeros) as a dict over ``GRADS``; dW_q / db_q are
    lists per step."""
    hidden, W_q, W_cq, w_ca, m1, m2 = (saved[k] for k in ("hidden", "W_q", "W_cq", "w_ca", "m1", "m2"))
    B, T, D = hidden.shape
    n = len(W_q)
    g_ins = np.zeros((n, B, D)) if g_ins is None else _f(g_ins)
    g_attn = np.zeros((n, B, T)) if g_attn is None else _f(g_attn)
    out = dict(dhidden=np.zeros((B, T, D)), dnode=np.zeros((B, D)), dW_q=[None] * n, db_q=[None] * n,
               dW_cq=np.zeros((D, 4 * D)), db_cq=np.zeros(D), dw_ca=np.zeros(D), db_ca=np.zeros(1))
    carry = np.zeros((B, D))
    for s in range(n - 1, -1, -1):
        st = saved["steps"][s]
        a, cq, hm, q, r = st["a"], st["cq"], st["hm"], st["q"], st["r"]
        drp = g_ins[s] + carry
        da = np.einsum("bd,btd->bt", drp, hidden) + g_attn[s]
        dca = a * (da - (a * da).sum(axis=1, keepdims=True))
        u = np.einsum("bt,btd->bd", dca, hm)                     # hm = h * m3
        dcq = w_ca * u
        wc = (w_ca * cq)[:, None, :] if st["m3"] is None else (w_ca * cq)[:, None, :] * st["m3"]
        out["dhidden"] += a[:, :, None] * drp[:, None, :] + dca[:, :, None] * wc
        out["dw_ca"] += (cq * u).sum(axis=0)
        dz = dcq @ W_cq
        if m2 is not None:
            dz = dz * m2[s]
        z0, z1, z2, z3 = dz[:, :D], dz[:, D:2 * D], dz[:, 2 * D:3 * D], dz[:, 3 * D:]
        carry = z0 - z2 + z3 * q
        dq = z1 + z2 + z3 * r
        out["dW_cq"] += dcq.T @ st["z"]
        out["db_cq"] += dcq.sum(axis=0)
        out["dW_q"][s] = dq.T @ st["n_s"]
        out["db_q"][s] = dq.sum(axis=0)
        dn = dq @ W_q[s]
        out["dnode"] += dn if m1 is None else dn * m1[s]
    out["dr_in"] = carry
    return out


def train_case(B, T, D, n, p, seed):
    """``instruction_oracle.random_case`` plus what a training call adds, all fp32: r_in, the upstream gradients g_ins /
    g_attn and - for p > 0 - the three multipliers (0 with probability p, else the fp32 value of 1/(1-p)); p == 0: None."""
    from instruction_oracle import random_case
    c = random_case(B, T, D, n, seed)
    rng = np.random.default_rng(seed + 1000)
    c["r_in"] = np.tanh(rng.standard_normal((B, D))).astype(np.float32)
    c["g_ins"] = rng.standard_normal((n, B, D)).astype(np.float32)
    c["g_attn"] = rng.standard_normal((n, B, T)).astype(np.float32)
    scale = np.float32(1.0) / np.float32(1.0 - p)
    for k, shape in (("m1", (n, B, D)), ("m2", (n, B, 4 * D)), ("m3", (n, B, T, D))):
        c[k] = (rng.random(shape) >= p).astype(np.float32) * scale if p > 0 else None
    return c
