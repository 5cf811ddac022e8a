"""k_update_b3 at the row counts where a wave's "next tile" changes meaning (csrc/tables_b3.hip: update_b3_part
requests a tile's h pieces a tile ahead and the row gates with them):

    8192        the smallest launch the kernel takes: every wave runs ONE tile, so the next tile is the tile itself
    8192 + 48   waves with one tile and waves with two
    8199        a partial last tile (rows past M are clamped, never stored)

at D = 200 and 208 (the last k block is clamped differently; the 6-tile column part ends at its last staged row) and in
both math modes that reach the kernel.  Written for the forms that request weight fragments and memory lines further
ahead (measured and rejected - they passed these tests); what any such form must keep is what the
kernel does today.  Data and proofs are those of tests/b3_probe.py: on the certified families h' must equal the float64
result BIT FOR BIT (a fragment that arrives a step late, a k block taken from the wrong tile or a product issued twice
changes an entry by at least one unit), full mantissas are held to the project's cap 4e-7 |a||w|
(profiles/dense_forms_rounding.txt), and a masked slot's score is exactly -1e11.  The row-gated form runs behind the
seed-prior layer with gates that are all closed, all open, alternate per row and alternate per 16-row tile; rows of
nbr behind a closed gate hold NaN.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import b3_probe as bp

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
NEG = np.float32(-1e11)
ROWS = (8192, 8192 + 48, 8199)
BN_MAX = max(ROWS)


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(dev)


def _same(got, want64, what):
    got = got.cpu().numpy().reshape(want64.shape).astype(f64)
    bad = np.flatnonzero((got != want64).ravel())
    assert bad.size == 0, "%s: %d of %d entries differ, first at %s: got %r want %r" % (
        what, bad.size, want64.size, np.unravel_index(bad[0], want64.shape), got.ravel()[bad[0]], want64.ravel()[bad[0]])


def _mask(BN):
    m = (np.random.default_rng(BN).random(BN) < 0.75).astype(f32)
    m[-1] = 0.0                      # the last (partial) tile holds a masked row next to a live one
    m[-2] = 1.0
    return m


def _maths():
    from gnnrag_amd import ops
    return (ops.MATH_BF16X3, ops.MATH_MIXED)


def _takes_update_b3(BN, D):
    from gnnrag_amd import ops
    return all(ops.dense_form("update_score_fused", BN, D, 1, math=m, add_rows=BN).family == ops.DENSE_UPDATE_B3
               for m in _maths())


def _self_block(W_self):
    D = W_self.shape[0]
    W = np.full((D, 3 * D), 3.0, dtype=f32)                    # I = 1; the neighbour blocks are not this launch's business
    W[:, :D] = W_self
    return W


# ---- the ungated form ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _exact_data(D, name, layout):
    """h [BN_MAX, D] and W's self block from a certified family; with the sparse layout also bias and neighbour sum
    (small integers).  The cases with fewer rows take the leading rows."""
    ints = layout == "sparse"
    fx = bp.family(name, layout, BN_MAX, D, D, seed=12, room=ints)
    b, nbr = bp.addends(np.random.default_rng(D + 1), BN_MAX, D)
    if not ints:
        b, nbr = np.zeros_like(b), np.zeros_like(nbr)
    pre = bp.certify(fx.A, fx.W, fx.live, extra=(b[None, :], nbr) if ints else ())
    na, nw = bp.planes_in_use(fx)
    for t in fx.live:
        assert na[bp.TERMS[t][0]] > 0 and nw[bp.TERMS[t][1]] > 0
    return fx.A, _self_block(fx.W), b, nbr, np.maximum(pre, 0.0)


@pytest.mark.parametrize("D,layout", [(200, "one"), (200, "sparse"), (208, "sparse")])
@pytest.mark.parametrize("name", bp.EXACT)
def test_update_exact(dev, name, D, layout):
    from gnnrag_amd import ops
    h, W, b, nbr, hn = _exact_data(D, name, layout)
    dW, db = _t(dev, W), _t(dev, b)
    for BN in ROWS:
        assert _takes_update_b3(BN, D)
        mask = _mask(BN)
        dh, dn, dm = _t(dev, h[:BN]), _t(dev, nbr[:BN]), _t(dev, mask)
        for i, math in enumerate(_maths()):
            c0 = (37 * BN + 5 * D) % 112 if i == 0 else 112 + (BN + D) % (D - 112)      # the score on part 0 / part 1
            w_s = np.zeros(D, dtype=f32)
            w_s[c0] = 1.0
            h_out, score = ops.update_score_fused(dh, dn, dW, db, _t(dev, w_s), _t(dev, [3.0]), dm, 1, math=math)
            _same(h_out, hn[:BN], "h' (M=%d math=%d)" % (BN, math))
            # one h' entry plus b_s: a single fp32 add, whichever part's atomic share carries it; masked: exactly -1e11
            s = (hn[:BN, c0].astype(f32) + np.float32(3.0)).astype(f64)
            _same(score, np.where(mask != 0, s, np.float64(NEG)), "score (M=%d math=%d)" % (BN, math))
            assert (score.cpu().numpy()[mask == 0] == NEG).all()


@pytest.mark.parametrize("D", [200, 208])
def test_update_full_mantissas_bounded(dev, D):
    """Random full-mantissa operands: every entry within 4e-7 |a||w| of the float64 product, the two math modes equal."""
    from gnnrag_amd import ops
    fx = bp.family("full_full", "one", BN_MAX, D, D, seed=13)
    dW, z = _t(dev, _self_block(fx.W)), _t(dev, np.zeros(D))
    want = np.maximum(bp.rows_matmul(fx.A, fx.W), 0.0)         # relu is 1-Lipschitz: the bound carries over
    S = bp.rows_matmul(np.abs(fx.A), np.abs(fx.W))
    for BN in ROWS:
        assert _takes_update_b3(BN, D)
        mask = _mask(BN)
        args = [_t(dev, fx.A[:BN]), _t(dev, np.zeros((BN, D))), dW, z, z, _t(dev, [0.0]), _t(dev, mask)]
        outs = [ops.update_score_fused(*args, 1, math=m) for m in _maths()]
        for a, b in zip(*outs):
            assert torch.equal(a, b)
        e = float((np.abs(outs[0][0].cpu().numpy().astype(f64) - want[:BN]) / S[:BN]).max())
        print("k_update_b3 M=%d D=%d full mantissas: e=%.3g" % (BN, D, e))
        assert e <= bp.E_CAP
        assert (outs[0][1].cpu().numpy()[mask == 0] == NEG).all()


# ---- the row-gated form --------------------------------------------------------------------------------------------------

GATES = {"closed": lambda r: np.zeros_like(r, dtype=bool), "open": lambda r: np.ones_like(r, dtype=bool),
         "per_row": lambda r: r % 2 == 1, "per_tile": lambda r: (r // 16) % 2 == 0}


@functools.lru_cache(maxsize=None)
def _gate_plan(BN, pattern):
    """One question of BN nodes whose frontier is exactly the wanted rows: two seeds s0, s1 among them, a fact from s0 to
    every other wanted row (s1 included) and one from s1 back to s0.  All gates closed: facts among the other rows and
    the seed on the last row, which no fact touches."""
    from gnnrag_amd import ops
    R1 = 12
    want = GATES[pattern](np.arange(BN))
    rows = np.flatnonzero(want) if want.any() else np.arange(BN - 1)
    s0, s1 = int(rows[0]), int(rows[1])
    heads = np.concatenate([np.full(rows.size - 1, s0), [s1]]).astype(np.int64)
    tails = np.concatenate([rows[1:], [s0]]).astype(np.int64)
    rels = (np.arange(heads.size) % (R1 - 2)).astype(np.int64)
    dist = np.zeros((1, BN), dtype=f32)
    if want.any():
        dist[0, [s0, s1]] = 0.5
    else:
        dist[0, BN - 1] = 1.0
    return ops.CsrPlan(heads, rels, tails, 1, BN, R1, torch.device("cuda", 0)), R1, dist, want


@functools.lru_cache(maxsize=None)
def _gated_data(D, name):
    fx = bp.family(name, "sparse", BN_MAX, D, D, seed=14, room=True)
    b = bp.addends(np.random.default_rng(D + 2), BN_MAX, D)[0]
    pre = np.maximum(bp.certify(fx.A, fx.W, fx.live, extra=(b[None, :],)), 0.0)      # the neighbour sum is the layer's own: 0
    return fx.A, _self_block(fx.W), b, pre


@pytest.mark.parametrize("pattern", list(GATES))
@pytest.mark.parametrize("D,name", [(200, "a3_whi"), (200, "ahi_w3"), (208, "mid_mid")])
def test_update_row_gated_exact(dev, D, name, pattern):
    """reason_layer on a seed prior with zero relation features (every table row and neighbour sum is exactly 0), the
    workspace filled with NaN first: h' = relu(h W_self^T + b) bit for bit on listed and unlisted rows alike."""
    from gnnrag_amd import _lib, ops
    h, W, b, pre = _gated_data(D, name)
    dW, db = _t(dev, W), _t(dev, b)
    c0 = 13 * len(pattern) % D
    w_s = np.zeros(D, dtype=f32)
    w_s[c0] = 1.0
    for BN in ROWS:
        plan, R1, dist, want = _gate_plan(BN, pattern)
        assert _lib.load().gnnrag_frontier_supported(ctypes.byref(plan.c), D) and plan.rel_total > 0
        assert ops.dense_form("update_score_fused", BN, D, 1, math=ops.MATH_BF16X3, add_rows=BN).family == ops.DENSE_UPDATE_B3
        flags = ops.Frontier(plan, _t(dev, dist)).read()[2].astype(bool)
        assert np.array_equal(flags, want), "the graph does not give the wanted gates"
        mask = _mask(BN)
        zRD, zD = _t(dev, np.zeros((R1, D))), _t(dev, np.zeros(D))
        ins = _t(dev, np.random.default_rng(5).standard_normal((1, 1, D)))
        for math in _maths():
            ws = ops.LayerWorkspace()
            ws.get(plan, D, 1, dev).fill_(255)      # every float of the workspace a NaN: nbr behind a closed gate stays one
            h_out, score, _ = ops.reason_layer(plan, _t(dev, h[:BN]).view(1, BN, D), _t(dev, dist), ins, zRD, zRD.clone(),
                                               _t(dev, np.zeros((D, D))), zD, dW, db, _t(dev, w_s), _t(dev, [1.0]),
                                               _t(dev, mask), ws=ws, path=_lib.PATH_FUSED | _lib.PATH_SEED_PRIOR, math=math)
            _same(h_out, pre[:BN], "h' (M=%d math=%d, gates %s)" % (BN, math, pattern))
            s = (pre[:BN, c0].astype(f32) + np.float32(1.0)).astype(f64)
            _same(score, np.where(mask != 0, s, np.float64(NEG)), "score")
