"""The middle and low bf16 planes of the bf16x3 kernels, checked exactly (data and proofs: tests/b3_probe.py,
tests/test_b3_probe_host.py).

The other dense tests pin down WHICH element meets which; their exact data (small integers, +-1) lives in the high
plane alone, and their random data is held to 2e-5 of the largest entry - seven times more than the loss of a whole
low-order plane product costs.  Here the operands carry non-zero middle and low planes and still have one right answer
(b3_probe.certify, asserted for the very arrays that go to the GPU), so h' / P / C must equal the float64 result BIT FOR
BIT: in k_update_b3, its row-gated form, k_tables_vq, k_tables_b3, the plane writer of k_rel_transform and the MATH = 1
forms of k_gemm_f32 - and, as a proof of the fixtures that owes nothing to a bf16 split, in the exact-fp32 kernels that
MATH_FP32 selects for the same data.  Full mantissas on both sides are not exact; for them every entry is held to the
project's cap |got - float64| <= 4e-7 |a||w|, which the host model meets (8e-8 with an accumulator that rounds to
nearest, 1.3e-7 toward zero) and a kernel that loses any one plane product misses by more than 17 x.
Every case first asserts the kernel it is there for.  GNNRAG_DENSE_FORMS_TABLE=<file> appends the measured e lines.
"""
import ctypes
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import b3_probe as bp
from test_gpu_tables_sparse import _plan, _planes_of, _want

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
NEG = np.float32(-1e11)
# (layout, room): full mantissas have no room for addends, so bias / neighbour sum / a second instruction ride on the
# coarser "room" grids of the "one" layout and on the sparse layout
ZERO, INTS = "zero", "ints"
UPDATE_VARIANTS = [("one", ZERO), ("one", INTS), ("sparse", ZERO), ("sparse", INTS)]


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(dev)


def _record(text):
    print(text)
    if os.environ.get("GNNRAG_DENSE_FORMS_TABLE"):
        with open(os.environ["GNNRAG_DENSE_FORMS_TABLE"], "a") as fh:
            fh.write(text + "\n")


def _same(got, want64, what):
    """Bit-for-bit: the float64 result is an fp32 number (certified) and the kernel must return exactly it."""
    got = got.cpu().numpy().reshape(want64.shape).astype(f64)
    bad = np.flatnonzero((got != want64).ravel())
    assert bad.size == 0, "%s: %d of %d entries differ, first at %s: got %r want %r" % (
        what, bad.size, want64.size, np.unravel_index(bad[0], want64.shape), got.ravel()[bad[0]], want64.ravel()[bad[0]])


def _mask(BN):
    m = (np.random.default_rng(BN).random(BN) < 0.75).astype(f32)
    m[-1] = 0.0                      # the (ragged) last tile holds a masked row ...
    m[-2] = 1.0                      # ... next to a live one
    return m


def _col(key, lo, hi):
    """The rotating score column: a different one per case, inside [lo, hi)."""
    return lo + zlib.crc32(repr(key).encode()) % (hi - lo)


# ---- k_update_b3 -------------------------------------------------------------------------------------------------------

BN_MAX = 8199


@functools.lru_cache(maxsize=2)
def _update_data(D, name, layout, variant):
    """h [BN_MAX, D] and the self block of W from a family; b / nbr zero or small integers; the certified float64
    pre-activation.  Shared by the cases that differ in row count and math mode (they take the leading rows)."""
    ints, rows = variant == INTS, BN_MAX
    fx = bp.family(name, layout, rows, D, D, seed=2, room=ints)
    b, nbr = bp.addends(np.random.default_rng(D), rows, D)
    if not ints:
        b, nbr = np.zeros_like(b), np.zeros_like(nbr)
    pre = bp.certify(fx.A, fx.W, fx.live, extra=(b[None, :], nbr) if ints else ())
    na, nw = bp.planes_in_use(fx)
    for t in fx.live:                                          # the planes this case is about are really there
        assert na[bp.TERMS[t][0]] > 0 and nw[bp.TERMS[t][1]] > 0
    W = np.full((D, 3 * D), 3.0, dtype=f32)                    # I = 1; the neighbour blocks are not this launch's business
    W[:, :D] = fx.W
    return {"h": fx.A, "W": W, "b": b, "nbr": nbr, "hn": np.maximum(pre, 0.0)}


def _check_update(dev, d, BN, math, c0, b_s=3.0, twice=False):
    """One gnnrag_update_score_fused call on the leading BN rows: h' bit for bit, live scores = the ONE h' entry the
    one-hot w_s selects plus b_s (a single fp32 add of two fp32 numbers: correctly rounded whichever column part's
    atomic share carries it), masked scores exactly -1e11."""
    from gnnrag_amd import ops
    D = d["h"].shape[1]
    w_s = np.zeros(D, dtype=f32)
    w_s[c0] = 1.0
    mask = _mask(BN)
    args = [_t(dev, d["h"][:BN]), _t(dev, d["nbr"][:BN]), _t(dev, d["W"]), _t(dev, d["b"]), _t(dev, w_s),
            _t(dev, [b_s]), _t(dev, mask)]
    h_out, score = ops.update_score_fused(*args, 1, math=math)
    hn = d["hn"][:BN]
    _same(h_out, hn, "h'")
    s = (hn[:, c0].astype(f32) + np.float32(b_s)).astype(f64)
    _same(score, np.where(mask != 0, s, np.float64(NEG)), "score")
    assert (score.cpu().numpy()[mask == 0] == NEG).all()
    if twice:
        h2, s2 = ops.update_score_fused(*args, 1, math=math)
        assert torch.equal(h_out, h2) and torch.equal(score, s2)


def _update_cases():
    """(D, family, layout, variant, rows, kernel), the cases of one fixture next to each other (it is built once): the
    bf16x3 kernel at 8192 rows and with a ragged last tile, and at D = 200 the kernels MATH_FP32 selects for the leading
    4096 rows (k_gemm_wres) and 4095 rows (k_update_skinny) of the same data - no bf16 split is involved there, so
    they prove the fixtures exact on their own."""
    out = []
    for D in (200, 208):
        for name in bp.EXACT:
            for layout, variant in UPDATE_VARIANTS:
                out += [(D, name, layout, variant, BN, "UPDATE_B3") for BN in (8192, BN_MAX)]
                if D == 200:
                    out += [(D, name, layout, variant, 4096, "WRES"), (D, name, layout, variant, 4095, "UPDATE_SKINNY")]
    return out


@pytest.mark.parametrize("D,name,layout,variant,BN,kernel", _update_cases())
def test_update_exact(dev, D, name, layout, variant, BN, kernel):
    from gnnrag_amd import ops
    family = getattr(ops, "DENSE_" + kernel)
    maths = (ops.MATH_BF16X3, ops.MATH_MIXED) if kernel == "UPDATE_B3" else (ops.MATH_FP32,)
    for math in maths:
        assert ops.dense_form("update_score_fused", BN, D, 1, math=math, add_rows=BN).family == family
    d = _update_data(D, name, layout, variant)
    key = (D, name, layout, variant, BN)
    _check_update(dev, d, BN, maths[0], _col(key, 0, 112), twice=True)              # the score rides on column part 0
    _check_update(dev, d, BN, maths[-1], _col(key, 112, D), b_s=-2.0)               # ... and on part 1


@pytest.mark.parametrize("BN,D", [(8192, 200), (BN_MAX, 200), (8192, 208), (BN_MAX, 208)])
def test_update_b3_full_mantissas_bounded(dev, BN, D):
    """full_full, one non-zero per row: every entry within 4e-7 |a||w| of the float64 product."""
    from gnnrag_amd import ops
    fx = bp.family("full_full", "one", BN, D, D, seed=3)
    W = np.full((D, 3 * D), 3.0, dtype=f32)
    W[:, :D] = fx.W
    z = np.zeros(D, dtype=f32)
    mask = _mask(BN)
    args = [_t(dev, fx.A), _t(dev, np.zeros((BN, D))), _t(dev, W), _t(dev, z), _t(dev, z), _t(dev, [0.0]), _t(dev, mask)]
    outs = {}
    for math in (ops.MATH_BF16X3, ops.MATH_MIXED):
        assert ops.dense_form("update_score_fused", BN, D, 1, math=math, add_rows=BN).family == ops.DENSE_UPDATE_B3
        outs[math] = ops.update_score_fused(*args, 1, math=math)
    again = ops.update_score_fused(*args, 1, math=ops.MATH_BF16X3)
    for a, b in zip(outs[ops.MATH_BF16X3], again):
        assert torch.equal(a, b)
    for a, b in zip(outs[ops.MATH_BF16X3], outs[ops.MATH_MIXED]):
        assert torch.equal(a, b)
    got = outs[ops.MATH_BF16X3][0].cpu().numpy().astype(f64)
    want = np.maximum(bp.rows_matmul(fx.A, fx.W), 0.0)         # relu is 1-Lipschitz: the bound carries over
    e = float((np.abs(got - want) / bp.rows_matmul(np.abs(fx.A), np.abs(fx.W))).max())
    _record("b3_planes k_update_b3        M=%-6d K=%-4d N=%-4d math=1 full mantissas, one non-zero per row  out: e=%.3g" % (BN, D, D, e))
    assert e <= bp.E_CAP


# ---- k_update_b3<true>: the row-gated form behind the seed-prior layer ---------------------------------------------------

@functools.lru_cache(maxsize=1)
def _gated_plan():
    from gnnrag_amd import ops, synth
    cfg = synth.GraphConfig(name="b3gate", B=5, N=1700, E=6000, R=40, D=200, I=1, L=1, T=1, seed=11, n_real_min=600)
    batch = synth.make_batch(cfg)
    et = batch.edge_tuple
    return cfg, batch, ops.CsrPlan(et[0], et[1], et[2], cfg.B, cfg.N, cfg.R1, torch.device("cuda", 0))


@pytest.mark.parametrize("layout,variant", [("one", ZERO), ("one", INTS), ("sparse", INTS)])
@pytest.mark.parametrize("name", bp.EXACT)
def test_update_b3_row_gated_exact(dev, name, layout, variant):
    """reason_layer on a one-seed prior with zero relation features, projection and position rows: T = 0, so every
    table row and every neighbour sum is exactly 0, and h' = relu(h W_self^T + b) bit for bit on the rows the
    frontier lists (nbr read through an open gate) AND on the others (gate closed: the zero row;
    their rows of nbr are never written and hold NaN here)."""
    from gnnrag_amd import _lib, ops
    cfg, batch, plan = _gated_plan()
    B, N, D, R1 = cfg.B, cfg.N, cfg.D, cfg.R1
    BN = B * N
    assert BN >= 8192
    # the kernel this case is there for: the frontier form of the layer, and a gated update on k_update_b3
    assert _lib.load().gnnrag_frontier_supported(ctypes.byref(plan.c), D) and plan.rel_total > 0
    assert ops.dense_form("update_score_fused", BN, D, 1, math=ops.MATH_BF16X3, add_rows=BN).family == ops.DENSE_UPDATE_B3
    dist = batch.seed_dist.astype(f32)
    assert ((dist != 0).sum(1) == 1).all()
    flags = ops.Frontier(plan, _t(dev, dist)).read()[2].astype(bool)
    assert flags.any() and (~flags).any()

    fx = bp.family(name, layout, BN, D, D, seed=2, room=variant == INTS)
    b = bp.addends(np.random.default_rng(D), BN, D)[0] if variant == INTS else np.zeros(D, dtype=f32)
    pre = np.maximum(bp.certify(fx.A, fx.W, fx.live, extra=(b[None, :],)), 0.0)      # the neighbour sum is the layer's own: 0
    W = np.full((D, 3 * D), 3.0, dtype=f32)
    W[:, :D] = fx.W
    c0 = _col((name, layout, variant), 0, D)
    w_s = np.zeros(D, dtype=f32)
    w_s[c0] = 1.0
    mask = _mask(BN)
    zRD, zD = _t(dev, np.zeros((R1, D))), _t(dev, np.zeros(D))
    ins = _t(dev, np.random.default_rng(5).standard_normal((B, 1, D)))
    ws = ops.LayerWorkspace()
    ws.get(plan, D, 1, dev).fill_(255)      # every float of the workspace a NaN: a row of nbr behind a closed gate stays one
    h_out, score, _ = ops.reason_layer(plan, _t(dev, fx.A).view(B, N, D), _t(dev, dist), ins, zRD, zRD.clone(),
                                       _t(dev, np.zeros((D, D))), zD, _t(dev, W), _t(dev, b), _t(dev, w_s),
                                       _t(dev, [1.0]), _t(dev, mask), ws=ws,
                                       path=_lib.PATH_FUSED | _lib.PATH_SEED_PRIOR, math=ops.MATH_BF16X3)
    got = h_out.cpu().numpy().reshape(BN, D).astype(f64)
    for kind, sel in (("listed", flags), ("unlisted", ~flags)):
        assert np.array_equal(got[sel], pre[sel]), "%s rows: %d entries differ" % (kind, int((got[sel] != pre[sel]).sum()))
    s = (pre[:, c0].astype(f32) + np.float32(1.0)).astype(f64)
    _same(score, np.where(mask != 0, s, np.float64(NEG)), "score")


# ---- the relation tables: k_rel_transform's plane writer, k_tables_vq, k_tables_b3, exact fp32 ---------------------------

def _tables_shape_ok(D):
    return D % 8 == 0 and (D + 31) // 32 == 7 and (D + 15) // 16 == 13


@functools.lru_cache(maxsize=1)
def _tables_data(D, I, name, layout, room):
    cfg, plan, rows = _plan(4, 600, None, I, 400, D)
    R1 = cfg.R1
    rng = np.random.default_rng([D, I])
    fxs = [bp.family(name, layout, R1, D, 2 * I * D, seed=4 + d, room=room) for d in range(2)]
    T = np.stack([fxs[0].A, np.roll(fxs[1].A, 76, axis=1)])    # (a multiple of four: the groups of four stay groups)
    W = np.full((D, (2 * I + 1) * D), 3.0, dtype=f32)          # block 1 + 2 i + d; the self block is not used here
    W[:, D:] = fxs[0].W.reshape(2 * I, D, D).transpose(1, 0, 2).reshape(D, 2 * I * D)
    ins = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], dtype=f32), size=(cfg.B, I, D))
    ru = np.unique(rows[:, 1])
    if layout == "one":                                        # the rows in use put a non-zero of either sign at every k
        for d in range(2):
            k = np.argmax(T[d][ru] != 0, 1)
            assert len({(a, b) for a, b in zip(k, np.sign(T[d][ru, k]))}) == 2 * D
    want = np.zeros((2, rows.shape[0], D))
    for d in range(2):
        # the product as k_tables_b3 and the fp32 kernel form it: A = relu(T * ins) (exact: ins is a power of two)
        A = np.concatenate([np.maximum(T[d][rows[:, 1]] * ins[rows[:, 0], i], 0) for i in range(I)], 1)
        Wd = np.concatenate([W[:, (1 + 2 * i + d) * D:(2 + 2 * i + d) * D] for i in range(I)], 1)
        want[d] = bp.certify(A, Wd, fxs[0].live)
        # ... and as k_tables_vq forms it: [relu(T) | relu(-T)] times V = sum_i max(+-ins_i, 0) W_i, per question
        for b in range(cfg.B):
            m = rows[:, 0] == b
            A2 = np.concatenate([np.maximum(T[d][rows[m, 1]], 0), np.maximum(-T[d][rows[m, 1]], 0)], 1)
            V = sum(np.concatenate([np.maximum(s * ins[b, i], 0)[None, :].astype(f64) *
                                    W[:, (1 + 2 * i + d) * D:(2 + 2 * i + d) * D] for s in (1, -1)], 1) for i in range(I))
            assert np.array_equal(V, V.astype(f32).astype(f64))          # V is rounded to fp32 once: nothing to round
            assert np.array_equal(bp.certify(A2, V.astype(f32), fxs[0].live), want[d][m])
    assert np.array_equal(want, _want(T, rows, ins, W, D, I))
    pa = [bp.planes_in_use(bp.Fixture(name, layout, T[d][ru], fxs[0].W, fxs[0].live)) for d in range(2)]
    for t in fxs[0].live:
        assert all(p[0][bp.TERMS[t][0]] > 0 and p[1][bp.TERMS[t][1]] > 0 for p in pa)
    return cfg, plan, rows, T, ins, W, want


def _host_planes(T, D):
    """What k_rel_transform writes for T [2, R1, D]: [2, 3, R1, 448] bf16 bit patterns of the planes of
    [relu(T) | relu(-T)], each half padded with zeros to 224."""
    out = np.zeros((2, 3, T.shape[1], 448), dtype=np.uint16)
    for d in range(2):
        for half, x in enumerate((np.maximum(T[d], 0), np.maximum(-T[d], 0))):
            for p, plane in enumerate(bp.split3(x)):
                out[d, p, :, 224 * half:224 * half + D] = (plane.view(np.uint32) >> 16).astype(np.uint16)
    return out


TABLE_CASES = [(1, n, "one", False) for n in bp.EXACT] + [(1, n, "sparse4", False) for n in bp.EXACT] + \
              [(2, n, "one", True) for n in ("a3_whi", "ahi_w3")]


@pytest.mark.parametrize("I,name,layout,room", TABLE_CASES)
@pytest.mark.parametrize("D", [200, 208])
def test_relation_tables_exact(dev, D, I, name, layout, room):
    """T carries the A-side family, W_e2e the weight side, ins in {+-1, +-2}: the planes k_rel_transform writes are the
    host split bit for bit, and the V-form kernel (OR-merge of plane+ and plane-, sign bits of the - half, on non-zero
    middle and low planes), the register-operand kernel and the exact-fp32 kernel all return the float64 tables."""
    from gnnrag_amd import ops
    cfg, plan, rows, T, ins, W, want = _tables_data(D, I, name, layout, room)
    # the kernels these calls run: the W-resident ones take 192 < D <= 208 with >= 1024 rows (relation_tables_planes
    # raises otherwise), and the call is too large for the one-workgroup-per-tile kernel of small batches
    assert _tables_shape_ok(D) and plan.rel_total >= 1024 and 4.0 * plan.rel_total * I * D * D > 1.5e8
    Tn, planes = _planes_of(dev, T[0], T[1])
    assert np.array_equal(Tn, T)
    assert np.array_equal(planes.cpu().numpy().view(np.uint16), _host_planes(T, D)), "k_rel_transform planes"
    dins, dW = _t(dev, ins), _t(dev, W)
    _same(ops.relation_tables_planes(plan, planes, dins, dW), want, "k_tables_vq")
    dT = _t(dev, T)
    _same(ops.relation_tables(plan, dT[0], dT[1], dins, dW, math=ops.MATH_BF16X3), want, "k_tables_b3")
    _same(ops.relation_tables(plan, dT[0], dT[1], dins, dW, math=ops.MATH_MIXED), want, "k_tables_b3 (mixed)")
    _same(ops.relation_tables(plan, dT[0], dT[1], dins, dW, math=ops.MATH_FP32), want, "fp32 tables")


@pytest.mark.parametrize("D", [200, 208])
def test_relation_tables_full_mantissas_bounded(dev, D):
    from gnnrag_amd import ops
    I = 1
    cfg, plan, rows = _plan(4, 600, None, I, 400, D)
    assert _tables_shape_ok(D) and plan.rel_total >= 1024 and 4.0 * plan.rel_total * I * D * D > 1.5e8
    fxs = [bp.family("full_full", "one", cfg.R1, D, 2 * D, seed=6 + d) for d in range(2)]
    T = np.stack([fxs[0].A, np.roll(fxs[1].A, 76, axis=1)])
    W = np.full((D, 3 * D), 3.0, dtype=f32)
    W[:, D:] = fxs[0].W.reshape(2, D, D).transpose(1, 0, 2).reshape(D, 2 * D)
    ins = np.random.default_rng(D).choice(np.array([-2.0, -1.0, 1.0, 2.0], dtype=f32), size=(cfg.B, I, D))
    Tn, planes = _planes_of(dev, T[0], T[1])
    assert np.array_equal(Tn, T)
    assert np.array_equal(planes.cpu().numpy().view(np.uint16), _host_planes(T, D))
    dins, dW, dT = _t(dev, ins), _t(dev, W), _t(dev, T)
    got = {"k_tables_vq": ops.relation_tables_planes(plan, planes, dins, dW),
           "k_tables_b3": ops.relation_tables(plan, dT[0], dT[1], dins, dW, math=ops.MATH_BF16X3)}
    for kernel, g in got.items():
        g = g.cpu().numpy().astype(f64)
        e = 0.0
        for d in range(2):
            A = np.maximum(T[d][rows[:, 1]] * ins[rows[:, 0], 0], 0)
            Wd = W[:, (1 + d) * D:(2 + d) * D]
            S = bp.rows_matmul(A, np.abs(Wd))
            live = S > 0
            e = max(e, float((np.abs(g[d] - bp.rows_matmul(A, Wd))[live] / S[live]).max()))
            assert (g[d][~live] == 0).all()
        _record("b3_planes %-18s M=%-6d K=%-4d N=%-4d math=1 full mantissas, one non-zero per row  out: e=%.3g" % (
            kernel, plan.rel_total, D, D, e))
        assert e <= bp.E_CAP, kernel


# ---- k_gemm_f32, MATH = 1 ------------------------------------------------------------------------------------------------

LIN_M = 16391
LIN_SHAPES = [(200, 208, 13), (200, 128, 8), (36, 64, 4), (36, 208, 13)]         # (K, N, NT)


@functools.lru_cache(maxsize=1)
def _linear_data(K, N, name, layout, variant):
    ints = variant == INTS
    fx = bp.family(name, layout, LIN_M, K, N, seed=8, room=ints)
    b, add = bp.addends(np.random.default_rng(K + N), LIN_M, N)
    want = bp.certify(fx.A, fx.W, fx.live, extra=(b[None, :], add) if ints else ())
    return fx, (b, add) if ints else (None, None), want


@pytest.mark.parametrize("layout,variant", [("one", ZERO), ("one", INTS), ("sparse", INTS)])
@pytest.mark.parametrize("name", bp.EXACT)
@pytest.mark.parametrize("K,N,NT", LIN_SHAPES)
def test_linear_b3_exact(dev, K, N, NT, name, layout, variant):
    """ops.linear above the skinny bound: the bf16x3 form of the k-tiled kernel (MATH = 1) in both modes that select it,
    and on the same data the exact-fp32 form and, on the leading 16384 rows, k_gemm_skinny."""
    from gnnrag_amd import ops
    fx, (b, add), want = _linear_data(K, N, name, layout, variant)
    dA, dW = _t(dev, fx.A), _t(dev, fx.W)
    db, dadd = (None, None) if b is None else (_t(dev, b), _t(dev, add))
    ar = None if b is None else LIN_M
    for math in (ops.MATH_BF16X3, ops.MATH_MIXED, ops.MATH_FP32):
        f = ops.dense_form("linear", LIN_M, K, N, math=math, add_rows=ar)
        assert (f.family, f.nt, f.v4, f.math) == (ops.DENSE_KTILED, NT, 1, int(math != ops.MATH_FP32)), f
        _same(ops.linear(dA, dW, db, dadd, math=math), want, "k_gemm_f32 math=%d" % math)
    M = 16384
    assert ops.dense_form("linear", M, K, N, math=ops.MATH_FP32, add_rows=None if b is None else M).family == ops.DENSE_SKINNY
    _same(ops.linear(dA[:M], dW, db, None if b is None else dadd[:M], math=ops.MATH_FP32), want[:M], "k_gemm_skinny")


@pytest.mark.parametrize("K,N,NT", [(200, 208, 13), (36, 64, 4)])
def test_linear_b3_full_mantissas_bounded(dev, K, N, NT):
    from gnnrag_amd import ops
    fx = bp.family("full_full", "one", LIN_M, K, N, seed=9)
    f = ops.dense_form("linear", LIN_M, K, N, math=ops.MATH_BF16X3)
    assert (f.family, f.nt, f.v4, f.math) == (ops.DENSE_KTILED, NT, 1, 1), f
    dA, dW = _t(dev, fx.A), _t(dev, fx.W)
    out = ops.linear(dA, dW, math=ops.MATH_BF16X3)
    assert torch.equal(out, ops.linear(dA, dW, math=ops.MATH_BF16X3))
    e = bp.entry_error(out.cpu().numpy(), fx.A, fx.W)
    _record("b3_planes k_gemm_f32 MATH=1  M=%-6d K=%-4d N=%-4d math=1 full mantissas, one non-zero per row  out: e=%.3g" % (LIN_M, K, N, e))
    assert e <= bp.E_CAP
