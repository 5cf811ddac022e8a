"""The relation tables in V form on the 2:4 sparse matrix instruction (tables_b3.hip: k_tables_vq).

The kernel interleaves K as (k+, k-): of relu(T)[r, k] and relu(-T)[r, k] at most one is non-zero, so the left operand
is |T| (plane+ OR plane-) plus one 2-bit position per value, taken from the sign of T.  These tests aim at what that
can get wrong and a random-data comparison hides in its tolerance: a wrong K position, index bit, stage boundary (k
blocks 0-2 / 3-5 / 6) or padding column selects a wrong element of W.  Everything goes through ops.rel_transform(...,
planes=True) and ops.relation_tables_planes.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_INTERNAL = 2e-5    # vs the float64 definition, times max(1, max |want|) (test_gpu_parity.py)


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()                      # the native library must be the thing under test
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _plan(B, R, used, I, N, D):
    from gnnrag_amd import ops, synth
    cfg = synth.GraphConfig(name="tabsp", B=B, N=N, E=6 * N, R=R, D=D, I=I, L=1, T=1, seed=B + R, rel_per_question=used,
                            n_real_min=N // 3)
    batch = synth.make_batch(cfg)
    et = batch.edge_tuple
    plan = ops.CsrPlan(et[0], et[1], et[2], cfg.B, cfg.N, cfg.R1, torch.device("cuda", 0))
    assert plan.rel_total >= 1024
    return cfg, plan, plan.rel_rows()


def _planes_of(dev, Tf, Ti):
    """T given directly: the projection with an identity weight and a zero bias reproduces its input."""
    from gnnrag_amd import ops
    D = Tf.shape[1]
    layers = [(torch.eye(D, device=dev), torch.zeros(D, device=dev), None, None)]
    T, planes = ops.rel_transform(torch.from_numpy(Tf).to(dev), torch.from_numpy(Ti).to(dev), layers, planes=True)
    return T[0].cpu().numpy(), planes[0]


def _want(Tn, rows, ins, W, D, I):
    want = np.zeros((2, rows.shape[0], D))
    for d in range(2):
        for i in range(I):
            A = np.maximum(Tn[d][rows[:, 1]].astype(np.float64) * ins[rows[:, 0], i].astype(np.float64), 0.0)
            want[d] += A @ W[:, (1 + 2 * i + d) * D:(2 + 2 * i + d) * D].astype(np.float64).T
    return want


@pytest.mark.parametrize("I", [1, 2])
@pytest.mark.parametrize("D", [200, 208])
def test_exact_selection(dev, D, I):
    """T in {+1, -1, 0} with one non-zero per row, at k = r mod D with the sign changing every D rows (every k with both
    signs), ins in {+1, -1}: a table entry is one element of W (I = 1) or a sum of I of them, and a product by 1.0 loses
    nothing in the 3-way split - so I = 1 must equal the float64 definition EXACTLY and I = 2 within one fp32 rounding
    (V is rounded to fp32 once before its exact split)."""
    from gnnrag_amd import ops
    cfg, plan, rows = _plan(4, 600, None, I, 400, D)
    R1 = cfg.R1
    r = np.arange(R1)
    T = np.zeros((2, R1, D), dtype=np.float32)
    T[0, r, r % D] = np.where((r // D) % 2 == 0, 1.0, -1.0)
    T[1, r, (r + 77) % D] = np.where((r // D) % 2 == 0, -1.0, 1.0)
    for d, shift in ((0, 0), (1, 77)):      # the rows in use put a non-zero of either sign at every k
        ru = np.unique(rows[:, 1])
        seen = {((x + shift) % D, T[d, x, (x + shift) % D]) for x in ru}
        assert len(seen) == 2 * D
    Tn, planes = _planes_of(dev, T[0], T[1])
    assert np.array_equal(Tn, T)
    rng = np.random.default_rng(D + I)
    ins = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(cfg.B, I, D))
    W = rng.uniform(-0.05, 0.05, size=(D, (2 * I + 1) * D)).astype(np.float32)
    got = ops.relation_tables_planes(plan, planes, torch.from_numpy(ins).to(dev), torch.from_numpy(W).to(dev)).cpu().numpy()
    want = _want(Tn, rows, ins, W, D, I)
    err = np.abs(got - want)
    print("exact selection D=%d I=%d: max |diff| = %.3g, entries that differ: %d of %d" % (D, I, err.max(), int((err > 0).sum()), err.size))
    if I == 1:
        assert np.array_equal(got.astype(np.float64), want)
    else:
        assert (err <= 2.0 ** -24 * np.abs(want)).all()


_PATTERNS = ["all_plus", "all_minus", "alternating_k", "alternating_pairs", "random_with_zeros"]


@pytest.mark.parametrize("pattern", _PATTERNS)
def test_index_patterns(dev, pattern):
    """Random |T| under imposed sign patterns: the positions (0,2), (1,3), (0,3), (1,2) of a group of four all occur at
    every k pair (the alternating pattern changes phase with the row), and the random one adds exact zeros of both signs
    and fp32 denormals, where either position is right but the value must stay out of the sum."""
    from gnnrag_amd import ops
    D, I = 200, 2
    cfg, plan, rows = _plan(4, 600, None, I, 400, D)
    R1 = cfg.R1
    rng = np.random.default_rng(_PATTERNS.index(pattern))
    mag = np.abs(rng.standard_normal((2, R1, D))).astype(np.float32) + np.float32(1e-3)
    k, r = np.arange(D)[None, None, :], np.arange(R1)[None, :, None]
    if pattern == "all_plus":
        sign = np.ones((2, R1, D), dtype=np.float32)
    elif pattern == "all_minus":
        sign = -np.ones((2, R1, D), dtype=np.float32)
    elif pattern == "alternating_k":
        sign = np.broadcast_to(np.where((k + r) % 2 == 0, 1.0, -1.0), (2, R1, D)).astype(np.float32)
    elif pattern == "alternating_pairs":
        sign = np.broadcast_to(np.where((k // 2 + r) % 2 == 0, 1.0, -1.0), (2, R1, D)).astype(np.float32)
    else:
        sign = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(2, R1, D))
    T = (mag * sign).astype(np.float32)
    if pattern == "random_with_zeros":
        u = rng.random((2, R1, D))
        T[u < 0.04] = 0.0
        T[(u >= 0.04) & (u < 0.08)] = -0.0
        den = (u >= 0.08) & (u < 0.10)
        T[den] = (sign[den] * np.float32(1e-41)).astype(np.float32)
    Tn, planes = _planes_of(dev, T[0], T[1])
    normal = np.abs(T) >= np.finfo(np.float32).tiny
    assert np.array_equal(Tn[normal], T[normal])              # the pattern under test is the one in the planes
    ins = (0.3 * rng.standard_normal((cfg.B, I, D))).astype(np.float32)
    W = rng.uniform(-0.05, 0.05, size=(D, (2 * I + 1) * D)).astype(np.float32)
    got = ops.relation_tables_planes(plan, planes, torch.from_numpy(ins).to(dev), torch.from_numpy(W).to(dev)).cpu().numpy()
    want = _want(Tn, rows, ins, W, D, I)
    scale = max(1.0, np.abs(want).max())
    err = np.abs(got - want).max()
    print("index pattern %s: max |diff| = %.3g, bound %.3g" % (pattern, err, TOL_INTERNAL * scale))
    assert err <= TOL_INTERNAL * scale


@pytest.mark.parametrize("B,R,used,I,N", [(70, 900, 40, 1, 300), (9, 1500, 260, 3, 300), (4, 600, None, 2, 400)])
def test_ragged_shapes_and_determinism(dev, B, R, used, I, N):
    """Fewer row tiles than a wave holds with many questions; very different relation counts with three instructions;
    row chunks per question.  Random T through a random projection; float64 definition at TOL_INTERNAL; a second call on
    the same inputs is bit-identical."""
    from gnnrag_amd import ops
    D = 200
    cfg, plan, rows = _plan(B, R, used, I, N, D)
    rng = np.random.default_rng(B + I)
    relf = [rng.standard_normal((cfg.R1, D)).astype(np.float32) for _ in range(2)]
    Wr = (rng.standard_normal((D, D)) / np.sqrt(D) * 0.4).astype(np.float32)
    br = (0.1 * rng.standard_normal(D)).astype(np.float32)
    layers = [(torch.from_numpy(Wr).to(dev), torch.from_numpy(br).to(dev), None, None)]
    T, planes = ops.rel_transform(torch.from_numpy(relf[0]).to(dev), torch.from_numpy(relf[1]).to(dev), layers, planes=True)
    Tn = T[0].cpu().numpy()
    ins = (0.3 * rng.standard_normal((B, I, D))).astype(np.float32)
    W = rng.uniform(-0.05, 0.05, size=(D, (2 * I + 1) * D)).astype(np.float32)
    dins, dW = torch.from_numpy(ins).to(dev), torch.from_numpy(W).to(dev)
    first = ops.relation_tables_planes(plan, planes[0], dins, dW).clone()
    second = ops.relation_tables_planes(plan, planes[0], dins, dW)
    assert torch.equal(first, second)
    want = _want(Tn, rows, ins, W, D, I)
    scale = max(1.0, np.abs(want).max())
    err = np.abs(first.cpu().numpy() - want).max()
    print("ragged B=%d R=%d used=%s I=%d: max |diff| = %.3g, bound %.3g" % (B, R, used, I, err, TOL_INTERNAL * scale))
    assert err <= TOL_INTERNAL * scale
