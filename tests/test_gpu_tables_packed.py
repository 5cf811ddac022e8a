"""The packed sparse operand of the relation tables on the GPU: what k_rel_transform writes (ops.rel_transform(...,
packed=True)) against the host packer bit for bit, k_tables_vq reading it (ops.relation_tables_packed) against float64 bit
for bit on the certificate families of tests/b3_probe.py, against the public plane path on full-mantissa data, and the
layer sequence - which runs on the packed form - against digests of what the library computed before it did
(tests/golden/stack_packed_parent.json) and against itself with GNNRAG_PATH_REUSE_PROJ.

Shapes: the smallest the table kernel admits (rel_total = 1025) with 130 questions, so that every question is one
workgroup's rows (no row chunks, also with one direction): one question with 7 rows (fewer than a tile), one with 37 (a
ragged tile), one with 600 (38 tiles: the waves take 4 or 5, so the pair branch and the odd fifth tile both run), one
without facts, the rest 3 or 6 rows.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import b3_probe as bp
import rel_packed as rp
from test_gpu_tables_sparse import _plan, _planes_of, _want

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stack_packed_parent.json")


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(dev)


# ---- the writer ----------------------------------------------------------------------------------------------------------

TINY = f32(1e-41)            # below half the smallest bf16: all three planes are empty


def _writer_T(rng, R1, D, tiny=True):
    """T [2, R1, D] with full mantissas, zeros of both signs sprinkled in, with `tiny` also values of both signs below the
    smallest bf16; in every row columns 8-11 hold both signs next to each other and 12-15 are +0.0, -0.0, 0, 0."""
    T = rng.standard_normal((2, R1, D)).astype(f32)
    u = rng.random((2, R1, D))
    T[u < 0.04] = 0.0
    T[(u >= 0.04) & (u < 0.08)] = -0.0
    if tiny:
        T[(u >= 0.08) & (u < 0.10)] = -TINY
        T[(u >= 0.10) & (u < 0.12)] = TINY
    T[:, :, 8:16] = np.array([1.5, -2.5, -0.75, 3.0, 0.0, -0.0, 0.0, 0.0], dtype=f32)
    return T


@pytest.mark.parametrize("pos", [False, True])
@pytest.mark.parametrize("D", [200, 208])
@pytest.mark.parametrize("R1", [37, 602])
def test_packed_writer(dev, R1, D, pos):
    """L = 2 layers; layer 0 projects with the identity (T is the input, specials included), layer 1 with a random
    weight; with `pos`, position rows (fewer than R1) are added, one layer's carrying the specials.  The packed operand
    must be the host packing of the very T the call returns.  What reaches the writer: the kernel's sums start at +0.0,
    so a -0.0 of the input arrives as +0.0 (-0.0 + 0.0); the values below the smallest bf16 arrive through the bias of
    layer 0 (an fp32 add onto an exact zero), whatever the matrix instruction does with such inputs."""
    from gnnrag_amd import ops
    rng = np.random.default_rng([R1, D, int(pos)])
    T = _writer_T(rng, R1, D)
    Wr = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(f32)
    br = (0.1 * rng.standard_normal(D)).astype(f32)
    b0 = np.zeros(D, dtype=f32)
    b0[14], b0[15] = -TINY, TINY                                # columns 14 and 15 of the input are zero
    prow = R1 - 5
    layers = []
    for j in range(2):
        W, b = (np.eye(D, dtype=f32), b0) if j == 0 else (Wr, br)
        pe = [None, None]
        if pos:
            pe = [_t(dev, 0.5 * _writer_T(rng, prow, D)[d] if j == 1 else np.zeros((prow, D))) for d in range(2)]
        layers.append((_t(dev, W), _t(dev, b), pe[0], pe[1]))
    rel = [_t(dev, T[0]), _t(dev, T[1])]
    Tn, packed = ops.rel_transform(rel[0], rel[1], layers, packed=True)
    assert tuple(packed.shape) == (2, 2, R1, rp.ROW_B) and packed.dtype == torch.uint8
    Tn = Tn.cpu().numpy()
    assert np.array_equal(Tn, ops.rel_transform(rel[0], rel[1], layers).cpu().numpy())          # T itself is untouched
    T0 = Tn[0]                                                  # layer 0: what the test put in
    normal = np.abs(T) >= np.finfo(f32).tiny
    assert np.array_equal(T0[normal], T[normal]), "the identity projection returns its input"
    hi = rp.planes3(np.abs(T0))[0]
    assert (T0[:, :, 12:14] == 0).all() and (T[:, :, 13] == 0).all() and np.signbit(T[:, :, 13]).all()
    assert (T0[:, :, 14] == -TINY).all() and (T0[:, :, 15] == TINY).all()
    assert ((T0 < 0) & (hi == 0)).any() and ((T0 > 0) & (hi == 0)).any()
    g = (T0 < 0).reshape(2, R1, D // 4, 4)
    assert (g.any(-1) & ~g.all(-1)).all(1).any()               # a group of four with both signs in every row
    got = packed.cpu().numpy()
    want = rp.pack(Tn)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d bytes differ, first at (layer, dir, row, byte) %s: got %#x want %#x" % (
        len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- the table kernel ------------------------------------------------------------------------------------------------------

B_Q, N_Q, R1_Q = 130, 40, 602
COUNTS = [7, 37, 600, 0, 6] + [3] * 125


@functools.lru_cache(maxsize=1)
def _small_plan():
    from gnnrag_amd import ops
    assert len(COUNTS) == B_Q and sum(COUNTS) == 1025
    rng = np.random.default_rng(130)
    h, r, t = [], [], []
    for b, n in enumerate(COUNTS):
        ids = np.sort(rng.choice(R1_Q, size=n, replace=False))
        i = np.arange(n)
        h.append(b * N_Q + i % N_Q)
        r.append(ids)
        t.append(b * N_Q + (i + 1) % N_Q)
    h, r, t = (np.concatenate(x).astype(np.int64) for x in (h, r, t))
    plan = ops.CsrPlan(h, r, t, B_Q, N_Q, R1_Q, torch.device("cuda", 0))
    rows = plan.rel_rows()
    assert plan.rel_total == 1025 and rows.shape == (1025, 2)
    assert np.array_equal(np.bincount(rows[:, 0], minlength=B_Q), np.array(COUNTS))
    # 38 tiles over 8 waves as the kernel deals them out: 4 and 5 tiles
    U = (600 + 15) // 16
    per_wave = {U * (w + 1) // 8 - U * w // 8 for w in range(8)}
    assert per_wave == {4, 5}
    return plan, rows


@functools.lru_cache(maxsize=1)
def _tables_data(D, I, name, layout, room):
    """As test_gpu_b3_planes._tables_data, on the small plan: T carries the A-side family, W_e2e the weight side, ins in
    {+-1, +-2}; the certified float64 tables."""
    plan, rows = _small_plan()
    rng = np.random.default_rng([D, I])
    fxs = [bp.family(name, layout, R1_Q, D, 2 * I * D, seed=4 + d, room=room) for d in range(2)]
    T = np.stack([fxs[0].A, np.roll(fxs[1].A, 76, axis=1)])    # (a multiple of four: the groups of four stay groups)
    W = np.full((D, (2 * I + 1) * D), 3.0, dtype=f32)
    W[:, D:] = fxs[0].W.reshape(2 * I, D, D).transpose(1, 0, 2).reshape(D, 2 * I * D)
    ins = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], dtype=f32), size=(B_Q, I, D))
    want = np.zeros((2, rows.shape[0], D))
    for d in range(2):
        A = np.concatenate([np.maximum(T[d][rows[:, 1]] * ins[rows[:, 0], i], 0) for i in range(I)], 1)
        Wd = np.concatenate([W[:, (1 + 2 * i + d) * D:(2 + 2 * i + d) * D] for i in range(I)], 1)
        want[d] = bp.certify(A, Wd, fxs[0].live)
    assert np.array_equal(want, _want(T, rows, ins, W, D, I))
    ru = np.unique(rows[:, 1])
    pa = [bp.planes_in_use(bp.Fixture(name, layout, T[d][ru], fxs[0].W, fxs[0].live)) for d in range(2)]
    for t in fxs[0].live:                                      # the planes this case is about are really there
        assert all(p[0][bp.TERMS[t][0]] > 0 and p[1][bp.TERMS[t][1]] > 0 for p in pa)
    assert all((T[d][ru] < 0).any() and (T[d][ru] > 0).any() for d in range(2))
    return plan, rows, T, ins, W, want


def _packed_of(dev, T):
    """T given directly (identity projection); returns one layer's packed operand [2, R1, 1408]."""
    from gnnrag_amd import ops
    D = T.shape[2]
    layers = [(torch.eye(D, device=dev), torch.zeros(D, device=dev), None, None)]
    Tn, packed = ops.rel_transform(_t(dev, T[0]), _t(dev, T[1]), layers, packed=True)
    assert np.array_equal(Tn[0].cpu().numpy(), T)
    return packed[0]


def _same(got, want64, what):
    got = got.cpu().numpy().astype(f64)
    bad = np.argwhere(got != want64)
    assert bad.size == 0, "%s: %d of %d entries differ, first at %s: got %r want %r" % (
        what, len(bad), want64.size, tuple(bad[0]), got[tuple(bad[0])], want64[tuple(bad[0])])


# A-side, weight-side, mid x mid in the one-non-zero layout, the same accumulating over rows of 3-4 non-zeros per k block
# (two of opposite sign inside one group of four), and two instructions
TABLE_CASES = [(1, n, "one", False) for n in bp.EXACT] + [(1, n, "sparse4", False) for n in bp.EXACT] + \
              [(2, n, "one", True) for n in ("a3_whi", "ahi_w3")]


@pytest.mark.parametrize("I,name,layout,room", TABLE_CASES)
@pytest.mark.parametrize("D", [200, 208])
def test_tables_packed_exact(dev, D, I, name, layout, room):
    from gnnrag_amd import ops
    plan, rows, T, ins, W, want = _tables_data(D, I, name, layout, room)
    packed = _packed_of(dev, T)
    assert np.array_equal(packed.cpu().numpy(), rp.pack(T))
    dins, dW = _t(dev, ins), _t(dev, W)
    _same(ops.relation_tables_packed(plan, packed, dins, dW), want, "k_tables_vq<packed>")
    for d in range(2):
        one = want.copy()
        one[1 - d] = 0.0
        _same(ops.relation_tables_packed(plan, packed, dins, dW, only_dir=d), one, "k_tables_vq<packed>, direction %d" % d)


@pytest.mark.parametrize("I", [1, 2])
@pytest.mark.parametrize("D", [200, 208])
def test_tables_packed_equals_planes(dev, D, I):
    """Full-mantissa random T, ins and W (with zeros of both signs in T): the packed path returns the plane path's P bit
    for bit."""
    from gnnrag_amd import ops
    plan, rows = _small_plan()
    rng = np.random.default_rng([D, I, 7])
    T = _writer_T(rng, R1_Q, D, tiny=False)
    ins = (0.3 * rng.standard_normal((B_Q, I, D))).astype(f32)
    W = rng.uniform(-0.05, 0.05, size=(D, (2 * I + 1) * D)).astype(f32)
    Tn, planes = _planes_of(dev, T[0], T[1])
    assert np.array_equal(Tn, T)
    packed = _packed_of(dev, T)
    dins, dW = _t(dev, ins), _t(dev, W)
    a = ops.relation_tables_packed(plan, packed, dins, dW)
    b = ops.relation_tables_planes(plan, planes, dins, dW)
    assert torch.equal(a, b), "%d entries differ" % int((a != b).sum())
    want = _want(T, rows, ins, W, D, I)
    assert np.abs(a.cpu().numpy() - want).max() <= 2e-5 * max(1.0, np.abs(want).max())
    assert torch.equal(a, ops.relation_tables_packed(plan, packed, dins, dW))


# ---- the layer sequence ----------------------------------------------------------------------------------------------------

STACK_CASES = [("d200_i2_l3", 200, 2, 3, False), ("d208_i1_l2_pos", 208, 1, 2, True)]


def stack_outputs(dev, D, I, L, pos):
    """Runs the layer stack twice on deterministic inputs (the second run reuses the projections in the workspace);
    returns ((h, score, dist) of the first run, the same of the second)."""
    from gnnrag_amd import _lib, ops
    cfg, plan, rows = _plan(4, 600, None, I, 400, D)
    B, N, R1 = cfg.B, cfg.N, cfg.R1
    rng = np.random.default_rng([D, I, L])
    relf = [_t(dev, rng.standard_normal((R1, D))) for _ in range(2)]
    layers = []
    for _ in range(L):
        pe = [_t(dev, 0.1 * rng.standard_normal((R1 - 3, D))) for _ in range(2)] if pos else [None, None]
        layers.append((_t(dev, rng.standard_normal((D, D)) / np.sqrt(D) * 0.4), _t(dev, 0.1 * rng.standard_normal(D)),
                       _t(dev, rng.standard_normal((D, (2 * I + 1) * D)) / np.sqrt((2 * I + 1) * D)),
                       _t(dev, 0.1 * rng.standard_normal(D)), pe[0], pe[1]))
    w_s, b_s = _t(dev, rng.standard_normal(D) / np.sqrt(D)), _t(dev, [0.1])
    mask = (rng.random(B * N) < 0.8).astype(f32)
    h0 = _t(dev, 0.5 * rng.standard_normal((B * N, D)))
    d0 = rng.random((B, N)) * mask.reshape(B, N)
    d0 = _t(dev, d0 / d0.sum(1, keepdims=True))
    ins = _t(dev, 0.3 * rng.standard_normal((B, I, D)))
    assert plan.rel_total >= 1024                              # the V form of the tables
    st = ops.LayerStack(plan, relf[0], relf[1], layers, w_s, b_s, _t(dev, mask), I, path=_lib.PATH_FUSED,
                        math=ops.MATH_BF16X3)
    first = st.run(h0, d0, ins)
    second = st.run(h0, d0, ins)
    torch.cuda.synchronize()
    return first, second


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def stack_digests(out, L):
    h, score, dist = out
    return {"dist": [digest(dist[j]) for j in range(L)], "h_final": digest(h[L - 1])}


@pytest.mark.parametrize("case,D,I,L,pos", STACK_CASES)
def test_layer_stack_unchanged_and_reuse(dev, case, D, I, L, pos):
    first, second = stack_outputs(dev, D, I, L, pos)
    for a, b in zip(first, second):
        assert torch.equal(a, b), "the run on reused projections differs"
    assert torch.isfinite(first[0]).all() and torch.isfinite(first[2]).all()
    with open(GOLDEN) as fh:
        want = json.load(fh)[case]
    assert stack_digests(first, L) == want, "every layer's dist and the final h: not what the plane-format library computed"
