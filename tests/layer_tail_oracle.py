"""Float64 oracle of the reasoning layer's tail under autograd (reasongnn.py:163-169) for the tests of
``gnnrag_layer_tail_train`` / ``gnnrag_layer_tail_backward``, and the generator of their cases.

With pre = pre_a (+ pre_b), the keep flags k (0/1) and scale of the dropout in front of ``score_func``, w / b the score
function and the node mask:

    h = max(pre, 0)      s = scale * sum_d h k w + b      score = s + (1 - mask) * (-1e11)      dist = softmax_n(score)

``pre_a + pre_b`` is ONE fp32 addition, as torch's ``a + b`` is, so ``h`` is an fp32 value held in float64.  The live score
``s`` is rounded to fp32 and the mask term added in fp32, as the reference does; only then is the softmax taken in float64.  A
pure float64 addition of -1e11 does not reproduce the reference: the fp32 sum is exactly ``float32(-1e11)`` for any
|s| < 4096 and a fully padded question comes out uniform, the float64 sum keeps s and it does not.

Backward: per question sigma = sum_n dist g_dist and gs = dist (g_dist - sigma) - the mask addition passes the gradient with
derivative 1, as autograd does - then g_pre = (h > 0) (g_h + gs w k scale), dw = sum_r gs k scale h, and db = 0: a softmax
does not move under a shift of its scores (autograd's own db is rounding residue)."""
import numpy as np

VERY_NEG = np.float32(-100000000000)


def _k(keep, scale):
    return 1.0 if keep is None else keep.astype(np.float64) * float(np.float32(scale))


def forward(pre_a, pre_b, keep, scale, w, b, mask):
    """(h [B*N,D] float64 holding fp32 values, s [B,N] float64 live score, score [B,N] float32, dist [B,N] float64)."""
    B, N = mask.shape
    pre = np.asarray(pre_a, np.float32) if pre_b is None else np.asarray(pre_a, np.float32) + np.asarray(pre_b, np.float32)
    assert pre.dtype == np.float32
    h = np.maximum(pre, np.float32(0)).astype(np.float64)
    s = ((h * _k(keep, scale)) @ np.asarray(w, np.float64).reshape(-1) + float(np.asarray(b).reshape(-1)[0])).reshape(B, N)
    score = s.astype(np.float32) + (np.float32(1) - np.asarray(mask, np.float32)) * VERY_NEG
    assert score.dtype == np.float32
    x = score.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return h, s, score, e / e.sum(axis=1, keepdims=True)


def backward(h, dist, keep, scale, w, g_h, g_dist):
    """{"g_pre" [B*N,D], "dw" [D], "db" 0.0}; g_h / g_dist may be None (that output was not used)."""
    w = np.asarray(w, np.float64).reshape(-1)
    gs = np.zeros(dist.shape)
    if g_dist is not None:
        g = np.asarray(g_dist, np.float64)
        gs = dist * (g - (dist * g).sum(axis=1, keepdims=True))
    gs = gs.reshape(-1, 1)
    k = _k(keep, scale)
    g_pre = gs * w[None, :] * k
    if g_h is not None:
        g_pre = g_pre + np.asarray(g_h, np.float64)
    return {"g_pre": np.where(h > 0, g_pre, 0.0), "dw": (gs * k * h).sum(axis=0), "db": 0.0}


def case(B, N, D, seed, p=0.0, with_b=True):
    """Inputs as fp32 / uint8 arrays.  For B > 1: every question has padded nodes, the last question is padded throughout,
    question 0 has a single live node (slot N - 1 when N > 1); about half of ``pre_a + pre_b`` is negative and at least one
    entry is exactly 0.  ``keep`` is None at p = 0."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    mask = np.ones((B, N), f32)
    if B > 1:
        for q in range(B):
            live = max(1, (2 * N) // 3 - q)
            mask[q, live:] = 0
            mask[q, 1:live:7] = 0                       # holes between live nodes too
        mask[0] = 0
        mask[0, N - 1] = 1
        mask[B - 1] = 0
    elif N > 2:
        mask[0, N - 2:] = 0
    pre_a = (0.5 * rng.standard_normal((B * N, D))).astype(f32)
    pre_b = (0.5 * rng.standard_normal((B * N, D))).astype(f32) if with_b else None
    r0, d0 = (B * N) // 2, D // 2
    if with_b:
        pre_a[r0, d0] = -pre_b[r0, d0]
        pre_a[B * N - 1, D - 1] = -pre_b[B * N - 1, D - 1]
    else:
        pre_a[r0, d0] = pre_a[B * N - 1, D - 1] = 0
    keep = (rng.random((B * N, D)) < 1.0 - p).astype(np.uint8) if p > 0 else None
    return dict(pre_a=pre_a, pre_b=pre_b, keep=keep, scale=1.0 / (1.0 - p) if p > 0 else 1.0,
                w=((rng.standard_normal(D) + 0.5) / np.sqrt(D)).astype(f32), b=np.array([0.3], f32), mask=mask,
                g_h=rng.standard_normal((B * N, D)).astype(f32), g_dist=rng.standard_normal((B, N)).astype(f32))
