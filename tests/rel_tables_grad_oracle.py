"""float64 oracle of the relation tables of the fused training form and of their backward (gnnrag_relation_tables /
gnnrag_relation_tables_backward), written from the formulas of include/gnnrag.h over a list of compact rows
``rows [M, 2]`` = (question, relation):

    a[d,m,i,k]         = T_d[r_m,k] * ins[b_m,i,k]          one fp32 multiply, as the library's loaders form it
    z                  = relu(a),   blk(i,d) = (1 + 2 i + d) D
    P[d,m,o]           = sum_i sum_k W[o, blk(i,d)+k] z[d,m,i,k]
    G[d,m,i,k]         = (sum_o g_P[d,m,o] W[o, blk(i,d)+k]) * [a[d,m,i,k] > 0]
    g_W[o, blk(i,d)+k] = sum_m g_P[d,m,o] z[d,m,i,k]        columns < D: 0
    g_T_d[r,k]         = sum_{m: r_m = r} sum_i G[d,m,i,k] ins[b_m,i,k]
    g_ins[b,i,k]       = sum_d sum_{m: b_m = b} G[d,m,i,k] T_d[r_m,k]

Everything after the fp32 product is float64.  Shared by the host test (which holds it against torch's float64 autograd
of the per-fact expression) and the GPU tests."""
import numpy as np


def case(rows, R1, B, D, I, seed=0, exact=False, lim=3):
    """Inputs for a row list: T_fwd, T_inv [R1,D], ins [B,I,D], W [D,(2I+1)D], g_P [2,M,D] (fp32).  ``exact``: integers in
    [-lim, lim] - every product and sum is then an integer (no rounding in any summation order while the sums stay below
    2^24) and the gate meets many exact zeros."""
    rng = np.random.default_rng(seed)
    M, K = len(rows), (2 * I + 1) * D
    if exact:
        draw = lambda *sh: rng.integers(-lim, lim + 1, size=sh).astype(np.float32)      # noqa: E731
        return dict(T_fwd=draw(R1, D), T_inv=draw(R1, D), ins=draw(B, I, D), W=draw(D, K), g_P=draw(2, M, D))
    draw = lambda s, *sh: (s * rng.standard_normal(sh)).astype(np.float32)              # noqa: E731
    return dict(T_fwd=draw(0.5, R1, D), T_inv=draw(0.5, R1, D), ins=draw(0.5, B, I, D), W=draw(0.3, D, K),
                g_P=draw(1.0, 2, M, D))


def _parts(rows, T_fwd, T_inv, ins, W):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    b, r = rows[:, 0], rows[:, 1]
    I, D = ins.shape[1], ins.shape[2]
    q = np.asarray(ins, np.float32)[b]                                            # [M, I, D]
    out = []
    for d, T in enumerate((T_fwd, T_inv)):
        t = np.asarray(T, np.float32)[r][:, None, :]                              # [M, 1, D]
        a = (t * q).astype(np.float32)                                            # the fp32 product
        Wd = np.stack([np.asarray(W, np.float64)[:, (1 + 2 * i + d) * D:(2 + 2 * i + d) * D] for i in range(I)])  # [I, o, k]
        out.append((a > 0, np.maximum(a, np.float32(0)).astype(np.float64), t.astype(np.float64), Wd))
    return b, r, q.astype(np.float64), out


def forward(rows, T_fwd, T_inv, ins, W):
    """P [2, M, D] float64."""
    _, _, _, parts = _parts(rows, T_fwd, T_inv, ins, W)
    return np.stack([np.einsum("mik,iok->mo", z, Wd) for _, z, _, Wd in parts])


def backward(rows, R1, B, T_fwd, T_inv, ins, W, g_P, absolute=False):
    """dict g_T_fwd, g_T_inv [R1,D], g_ins [B,I,D], g_W [D,(2I+1)D] (float64).  ``absolute``: every operand replaced by its
    absolute value and nothing gated - an upper bound of every partial sum in any order (``"H"``: of the product in front
    of the gate as well)."""
    if absolute:
        T_fwd, T_inv, ins, W, g_P = (np.abs(np.asarray(x, np.float32)) for x in (T_fwd, T_inv, ins, W, g_P))
    b, r, q, parts = _parts(rows, T_fwd, T_inv, ins, W)
    I, D = ins.shape[1], ins.shape[2]
    gP = np.asarray(g_P, np.float64)
    g_T = [np.zeros((R1, D)), np.zeros((R1, D))]
    g_ins, g_W, hmax = np.zeros((B, I, D)), np.zeros((D, (2 * I + 1) * D)), 0.0
    for d, (gate, z, t, Wd) in enumerate(parts):
        H = np.einsum("mo,iok->mik", gP[d], Wd)
        hmax = max(hmax, float(np.abs(H).max()) if H.size else 0.0)
        G = H if absolute else np.where(gate, H, 0.0)
        for i in range(I):
            g_W[:, (1 + 2 * i + d) * D:(2 + 2 * i + d) * D] = np.einsum("mo,mk->ok", gP[d], z[:, i])
        np.add.at(g_T[d], r, (G * q).sum(axis=1))
        np.add.at(g_ins, b, G * t)
    out = dict(g_T_fwd=g_T[0] + 0.0, g_T_inv=g_T[1] + 0.0, g_ins=g_ins + 0.0, g_W=g_W + 0.0)      # + 0.0: no -0
    if absolute:
        out["H"] = hmax
    return out


def largest_sum(rows, R1, B, c):
    """Upper bound of the absolute value of every partial sum of the backward of case ``c`` (see ``backward``)."""
    g = backward(rows, R1, B, c["T_fwd"], c["T_inv"], c["ins"], c["W"], c["g_P"], absolute=True)
    return max(float(np.max(v)) if np.size(v) else 0.0 for v in g.values())
