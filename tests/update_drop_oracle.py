"""numpy float64 restatement of the concatenated update under dropout (gnnrag_update_drop_train / _backward;
reasongnn.py:161-163 in training): x = [h | agg], xd = keep ? x * scale : +0 with the product x * scale rounded to fp32 as the
library forms it (one fp32 multiply per element), everything behind it in float64.

    pre  = xd W^T + b
    g_x  = keep ? scale * (g_pre W) : +0          split into g_h (columns < D) and g_agg
    dW   = g_pre^T xd                              db = column sums of g_pre

``case`` draws the inputs; it guarantees rows with every element dropped, rows with none dropped, and ``keep=None`` for
p = 0.  ``exact=True`` draws integers in [-3, 3] (use p = 0.5, scale 2): every operand is exact in one bf16 plane and every
sum stays far below 2^24, so fp32 and bf16x3 kernels must reproduce the oracle bit for bit."""
import numpy as np


def xd_f32(h, agg, keep, scale):
    """The dropped operand as the library forms it, fp32 [BN, K]."""
    x = np.concatenate([h, agg], axis=1).astype(np.float32)
    if keep is None:
        return x
    xs = x * np.float32(scale)                                     # one fp32 multiply
    return np.where(keep != 0, xs, np.float32(0.0)).astype(np.float32)


def forward(h, agg, keep, scale, W, b):
    xd = xd_f32(h, agg, keep, scale).astype(np.float64)
    return xd @ W.astype(np.float64).T + b.astype(np.float64)


def backward(g_pre, h, agg, keep, scale, W):
    D = h.shape[1]
    g = g_pre.astype(np.float64)
    gx = g @ W.astype(np.float64)
    if keep is not None:
        gx = np.where(keep != 0, gx * float(np.float32(scale)), 0.0)
    xd = xd_f32(h, agg, keep, scale).astype(np.float64)
    return {"g_h": np.ascontiguousarray(gx[:, :D]), "g_agg": np.ascontiguousarray(gx[:, D:]), "dW": g.T @ xd,
            "db": g.sum(axis=0)}


def case(BN, D, I, p, seed=0, exact=False):
    """dict(h, agg, keep, scale, W, b, g_pre).  keep is None for p = 0; otherwise row 0 (and, from 3 rows on, a middle
    row) has every element dropped and row BN - 1 (from 2 rows on) none."""
    rng = np.random.default_rng(1000003 * seed + 7919 * BN + 31 * D + I)
    K = (2 * I + 1) * D
    f32 = np.float32
    if exact:
        draw = lambda *s: rng.integers(-3, 4, size=s).astype(f32)          # noqa: E731
    else:
        draw = lambda *s: rng.standard_normal(s).astype(f32)               # noqa: E731
    c = dict(h=draw(BN, D), agg=draw(BN, 2 * I * D), W=draw(D, K), b=draw(D), g_pre=draw(BN, D))
    if not exact:
        c["W"] *= f32(1.0 / np.sqrt(K))
    if p == 0:
        c["keep"], c["scale"] = None, 1.0
        return c
    keep = (rng.random((BN, K)) >= p).astype(np.uint8)
    keep[0] = 0
    if BN >= 3:
        keep[BN // 2] = 0
    if BN >= 2:
        keep[BN - 1] = 1
    c["keep"], c["scale"] = keep, float(f32(1.0) / f32(1.0 - p))
    return c
