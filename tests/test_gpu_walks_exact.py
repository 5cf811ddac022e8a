"""Exact and per-row tests of the sparse walks and of their backward, through gnnrag_amd.ops only.

EXACT cases (tests/walk_probe.py builds them, tests/test_walk_probe_host.py proves them on the host): row lengths placed
on every step boundary of the walks, data on a grid (priors m 2^-10, tables in [-4, 4], weights in {0.5, 1, 2}) with a
certificate - asserted here again on the very arrays that go to the device - that makes every partial sum in every
order an fp32 number.  The device result must equal the float64 sum over the caller's tuple BIT FOR BIT.  Each case first
asserts the form it means to test: the walk variant, the plan's big-node lists, the launch regime computed from the
device's CU count.  The fused gather walk (tables larger than LDS) has no case here: see DESIGN 5.1.

PER-ROW ROUNDING CLASS on full-mantissa data (priors = softmax of 6 standard_normal: eight decades; standard_normal
tables): for every output entry e = |got - want64| / S with S = sum of |terms|;
  (a)  e <= (n + k + 4) 2^-23 for a row of n terms in a question of k relations - it holds for ANY summation order
       (n - 1 additions, the k-term relation product of the dense hub form, the roundings of w^2, w^2 p and the products;
       unit 2^-23 because the matrix pipe's fp32 accumulation may truncate);
  (b)  the largest e over the rows of a class is at most 8 times the same figure of a numpy float32 sum of the same
       terms, one after the other in stored order.
Rows with S = 0 must be exactly 0.  No row is left out.  Measured maxima: profiles/walks_rounding.txt (written when
GNNRAG_WALKS_ROUNDING_OUT names a file).

Two calls on the same inputs must return identical bytes - asserted on the arrays every case computes anyway."""
import os

import numpy as np
import pytest
import torch

import walk_probe as wp

pytestmark = pytest.mark.gpu
U23 = 2.0 ** -23
SENTINEL = -7.25


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    return torch.device("cuda", 0)


def _t(dev, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in arrs]


def _plan(g, dev, w=None, wrel=None):
    from gnnrag_amd import ops
    plan = ops.CsrPlan(g.h, g.r, g.t, g.B, g.N, g.R, dev)
    rows = plan.rel_rows().astype(np.int64)
    assert plan.rel_total == g.rel_total and np.array_equal(rows[:, 0] * (g.R + 1) + rows[:, 1], g.rel_key)
    if w is not None:
        plan.attach_w_gnn(w)
    if wrel is not None:
        plan.attach_w_rel(wrel)
    return plan


def _same(got, want64, g=None, what=""):
    """Bit for bit; a failure names the rows: node, slot, len0, len1, first wrong column."""
    want = np.asarray(want64).astype(np.float32)
    got = np.asarray(got).reshape(want.shape)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    msg = "%s: %d entries of %d differ" % (what, len(bad), want.size)
    if g is not None and want.ndim == 2 and want.shape[0] == g.B * g.N:
        rows = np.unique(bad[:, 0])[:12]
        msg += "; (node, question, slot, len0, len1, first column, got, want): " + str(
            [(int(n), int(n // g.N), int(n % g.N), int(g.len0[n]), int(g.len1[n]), int(bad[bad[:, 0] == n][0, 1]),
              float(got[n, bad[bad[:, 0] == n][0, 1]]), float(want[n, bad[bad[:, 0] == n][0, 1]])) for n in rows])
    else:
        msg += "; first: " + str([(tuple(int(x) for x in b), float(got[tuple(b)]), float(want[tuple(b)])) for b in bad[:8]])
    raise AssertionError(msg)


def _bits(a, b, what):
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what + ": two calls differ"


def _assert_form(plan, g, name, dev):
    """The form an LDS-walk case means to test: variant, launch regime (from the CU count), the plan's big-node lists."""
    from gnnrag_amd import ops
    _, _, D, variant, _, _ = wp.FUSED_BY_NAME[name]
    assert variant != wp.WALK_L2_GATHER
    assert ops.aggregate_fused_variant(plan, D) == variant == wp.walk_variant(g.rel_max, D), name
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    if cus not in wp.REGIME_AT:
        pytest.fail("no expected launch regime for a device of %d CUs: add it to walk_probe.REGIME_AT" % cus)
    reg = wp.launch_regime(g.B, g.N, D, variant, cus)
    assert reg["regime"] == wp.REGIME_AT[cus][name], (name, cus, reg)
    big = plan.to_host()["big"]
    for q in range(g.B):
        assert np.array_equal(big[q], g.big_nodes(q) + q * g.N), (name, q)
    return reg


def _fused_exact(name, wts, dev, dirs=(0, 1)):
    from gnnrag_amd import ops
    g, dist, P, w = wp.fused_data(name, wts)
    if dirs != (0, 1):
        P = P.copy()
        P[1 - dirs[0]] = 0.0
    want = wp.ref_fused(g, dist, P, w, dirs=dirs)
    wp.certify_fused(name, g, dist, P, w, want)
    plan = _plan(g, dev, w)
    _assert_form(plan, g, name, dev)
    d_dist, d_P = _t(dev, dist, P)
    got = ops.aggregate_fused(plan, d_dist, d_P).cpu().numpy()
    again = ops.aggregate_fused(plan, d_dist, d_P).cpu().numpy()
    _same(got, want, g, name)
    _bits(got, again, name)


IN_PROCESS = wp.GPU_FUSED_CASES


@pytest.mark.parametrize("wts", [False, True], ids=["plain", "weights"])
@pytest.mark.parametrize("name", IN_PROCESS)
def test_fused_walk_exact(dev, name, wts):
    _fused_exact(name, wts, dev)


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("name", ["ladder_d200", "ladder32_d72"])
def test_fused_walk_exact_one_direction(dev, name, d):
    """Each direction alone: the other direction's tables are zero (the entry point walks both)."""
    _fused_exact(name, True, dev, dirs=(d,))


@pytest.mark.parametrize("wts", [False, True], ids=["plain", "weights"])
@pytest.mark.parametrize("I,D", wp.UNFUSED_CASES)
def test_unfused_walk_exact(dev, I, D, wts):
    from gnnrag_amd import ops
    g, dist, ins, Tf, Ti, w = wp.unfused_data(I, D, wts)
    want = wp.ref_unfused(g, dist, ins, Tf, Ti, w)
    wp.certify_unfused(g, dist, ins, Tf, Ti, w, want)
    assert len(g.hubs(0)) and len(g.hubs(1))                    # rows above 256 facts: k_heavy_partial / k_heavy_reduce
    plan = _plan(g, dev, w)
    args = _t(dev, dist, ins, Tf, Ti)
    got = ops.aggregate(plan, *args).cpu().numpy()
    _same(got, want, g, "aggregate I=%d D=%d" % (I, D))
    _bits(got, ops.aggregate(plan, *args).cpu().numpy(), "aggregate")


@pytest.mark.parametrize("wts", [False, True], ids=["plain", "w_rel"])
def test_typelayer_walk_exact(dev, wts):
    from gnnrag_amd import ops
    g, T, w = wp.typelayer_data(200, wts)
    want = wp.ref_typelayer(g, T, w)
    wp.certify_typelayer(g, T, w, want)
    plan = _plan(g, dev, wrel=w)
    (d_T,) = _t(dev, T)
    got = ops.typelayer(plan, d_T, wts).cpu().numpy()
    _same(got, want, g, "typelayer")
    _bits(got, ops.typelayer(plan, d_T, wts).cpu().numpy(), "typelayer")


def _frontier(dev, case, exact=True):
    from gnnrag_amd import ops
    g, dist, P, w, D = wp.frontier_data(case, exact)
    flag, want = wp.ref_frontier(g, dist, P, w)
    if exact:
        wp.certify_fused(case, g, dist, P, w, want)
    plan = _plan(g, dev, w)
    d_dist, d_P = _t(dev, dist, P)
    fr = ops.Frontier(plan, d_dist)
    nrows, _, flags = fr.read()
    listed = flags.astype(bool)
    if case == "more_seeds_than_the_list":      # question 0 overflows the LDS seed list: flagged as a whole (a superset)
        assert listed[:g.N].all() and np.array_equal(listed[g.N:], flag[g.N:])
    else:
        assert np.array_equal(listed, flag)
    assert nrows == int(listed.sum()) and (~listed).any()
    outs = []
    for _ in range(2):
        out = torch.full((g.B * g.N, D), SENTINEL, device=dev)
        outs.append(fr.aggregate(d_P, out).cpu().numpy())
    _bits(outs[0], outs[1], case)
    return g, dist, P, w, listed, outs[0], want


@pytest.mark.parametrize("case", wp.FRONTIER_CASES)
def test_frontier_walk_exact(dev, case):
    g, _, _, _, listed, got, want = _frontier(dev, case)
    if case == "reaches_4097_row":
        assert ((g.len0 + g.len1)[listed] > 4096).any()
    assert (got[~listed] == SENTINEL).all(), "an unlisted row was written"
    w32 = want.astype(np.float32)
    w32[~listed] = SENTINEL
    _same(got, w32, g, case)


@pytest.mark.parametrize("gname,D", wp.GPU_BACKWARD_CASES)
def test_backward_exact(dev, gname, D):
    from gnnrag_amd import ops
    g, d = wp.backward_data(gname, D)
    t = dict(zip(d, _t(dev, *d.values())))
    plan = _plan(g, dev, d["w"])
    (gd, gP), want, want_tl = wp.certify_backward(g, d)
    got = [x.cpu().numpy() for x in ops.aggregate_fused_backward(plan, t["dist"], t["P"], t["gn"])]
    again = [x.cpu().numpy() for x in ops.aggregate_fused_backward(plan, t["dist"], t["P"], t["gn"])]
    _same(got[0], gd, None, "fused g_dist")
    _same(got[1], gP, None, "fused g_P")
    for a, b in zip(got, again):
        _bits(a, b, "aggregate_fused_backward")
    for gather in (True, False):
        run = lambda: [x.cpu().numpy() for x in ops.aggregate_backward(plan, t["dist"], t["ins"], t["Tf"], t["Ti"], t["gagg"],
                                                                        gather=gather)]
        got = run()
        for x, wv, nm in zip(got, want, ("g_dist", "g_ins", "g_T_fwd", "g_T_inv")):
            _same(x, wv, None, "%s gather=%s" % (nm, gather))
        for a, b in zip(got, run()):            # exact data: even the atomic (LDS) form has one answer
            _bits(a, b, "aggregate_backward gather=%s" % gather)
    for wrel in (None, d["wrel"]):
        plan_t = _plan(g, dev, wrel=wrel)
        wantT = want_tl[wrel is not None]
        for gather in (True, False):
            got = ops.typelayer_backward(plan_t, t["gn"], wrel is not None, gather=gather).cpu().numpy()
            _same(got, wantT, None, "typelayer g_T gather=%s w_rel=%s" % (gather, wrel is not None))
            _bits(got, ops.typelayer_backward(plan_t, t["gn"], wrel is not None, gather=gather).cpu().numpy(), "typelayer_backward")


# ---- per-row rounding class ------------------------------------------------------------------------------------------

MEASURED = []


def _record(form, cls, rows, e_dev, e_f32, bound):
    line = "%-34s %-7s rows %6d   device max e %.3e   float32 in stored order %.3e   bound (a) at that row %.3e" % (
        form, cls, rows, e_dev, e_f32, bound)
    MEASURED.append(line)
    print(line)
    path = os.environ.get("GNNRAG_WALKS_ROUNDING_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _rounding_class(form, got, want, S, yard, n, k, classes):
    """(a) and (b) for an output [rows, columns]; n, k per row; classes = {name: row mask}, together every row."""
    got, yard = np.asarray(got, np.float64).reshape(want.shape), np.asarray(yard, np.float64).reshape(want.shape)
    zero = S == 0
    assert (got[zero] == 0).all(), form + ": an entry without terms is not exactly 0"
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(zero, 0.0, np.abs(got - want) / S)
        ey = np.where(zero, 0.0, np.abs(yard - want) / S)
    cap = ((n + k + 4) * U23).reshape((-1,) + (1,) * (want.ndim - 1))
    cover = np.zeros(want.shape[0], bool)
    fails = []
    for cls, m in classes.items():
        cover |= m
        if not m.any():
            continue
        em, eym = float(e[m].max()), float(ey[m].max())
        worst = np.unravel_index(np.argmax(np.where(m.reshape((-1,) + (1,) * (want.ndim - 1)), e, -1.0)), e.shape)
        _record(form, cls, int(m.sum()), em, eym, float(cap[worst[0]].max()))
        if em > 8 * eym:
            fails.append("(b) %s %s: device %.3e > 8 x float32 %.3e" % (form, cls, em, eym))
    assert cover.all(), form + ": a row is in no class"
    over = e > cap
    if over.any():
        r = np.argwhere(over)[0]
        fails.append("(a) %s: row %d e = %.3e > (n + k + 4) 2^-23 = %.3e" % (form, r[0], e[tuple(r)], cap[r[0]].max()))
    assert not fails, "; ".join(fails)


def _lds_classes(g):
    ln, big = g.len0 + g.len1, np.maximum(g.len0, g.len1) > wp.BIG_DEG
    return {"light": ~big, "medium": big & (ln <= wp.TEAM_DEG), "huge": big & (ln > wp.TEAM_DEG)}


def _gather_classes(g):
    hub = np.maximum(g.len0, g.len1) > wp.HEAVY_DEG
    return {"light": ~hub, "hub": hub}


@pytest.mark.parametrize("name,wts", [("ladder_d200", True), ("ladder32_d200", False), ("b1_n1024_d200", False)])
def test_fused_walk_rounding_class(dev, name, wts):
    from gnnrag_amd import ops
    g, dist, P, w = wp.fused_data(name, wts, exact=False)
    plan = _plan(g, dev, w)
    _assert_form(plan, g, name, dev)
    d_dist, d_P = _t(dev, dist, P)
    got = ops.aggregate_fused(plan, d_dist, d_P).cpu().numpy()
    _bits(got, ops.aggregate_fused(plan, d_dist, d_P).cpu().numpy(), name)
    n, k = wp.ref_row_terms(g)
    _rounding_class("aggregate_fused " + name, got, wp.ref_fused(g, dist, P, w), wp.ref_fused(g, dist, P, w, absolute=True),
                    wp.f32_stored_order(g, dist, P, w), n, k, _lds_classes(g))


def test_unfused_walk_rounding_class(dev):
    from gnnrag_amd import ops
    I, D = 2, 200
    g, dist, ins, Tf, Ti, w = wp.unfused_data(I, D, True, exact=False)
    plan = _plan(g, dev, w)
    got = ops.aggregate(plan, *_t(dev, dist, ins, Tf, Ti)).cpu().numpy()
    want = wp.ref_unfused(g, dist, ins, Tf, Ti, w)
    n, k = wp.ref_row_terms(g)
    _rounding_class("aggregate I=2 D=200", got, want, wp.ref_unfused(g, dist, ins, Tf, Ti, w, absolute=True),
                    wp.f32_stored_order_unfused(g, dist, ins, Tf, Ti, w), n, k, _gather_classes(g))


def test_typelayer_walk_rounding_class(dev):
    from gnnrag_amd import ops
    g, T, w = wp.typelayer_data(200, True, exact=False)
    plan = _plan(g, dev, wrel=w)
    got = ops.typelayer(plan, _t(dev, T)[0], True).cpu().numpy()
    n, k = wp.ref_row_terms(g)
    _rounding_class("typelayer D=200", got, wp.ref_typelayer(g, T, w), wp.ref_typelayer(g, T, w, absolute=True),
                    wp.f32_stored_order_typelayer(g, T, w), n, k, _gather_classes(g))


def test_frontier_walk_rounding_class(dev):
    g, dist, P, w, listed, got, want = _frontier(dev, "reaches_4097_row", exact=False)
    assert (got[~listed] == SENTINEL).all()
    n, k = wp.ref_row_terms(g)
    sub = lambda a: a[listed]
    cls = {c: m[listed] for c, m in _lds_classes(g).items()}
    _rounding_class("Frontier.aggregate", sub(got), sub(want), sub(wp.ref_fused(g, dist, P, w, absolute=True)),
                    sub(wp.f32_stored_order(g, dist, P, w)), sub(n), sub(k), cls)


@pytest.mark.parametrize("gname,D", wp.GPU_BACKWARD_CASES)
def test_backward_rounding_class(dev, gname, D):
    """n of the bound = the number of terms of an entry: facts x D for g_dist (a dot product per fact), facts of the
    (question, relation) row for g_P, facts of the relation for g_T, facts of the question for g_ins."""
    from gnnrag_amd import ops
    g, d = wp.backward_data(gname, D, exact=False)
    t = dict(zip(d, _t(dev, *d.values())))
    plan = _plan(g, dev, d["w"])
    BN = g.B * g.N
    deg = g.len0 + g.len1
    kq = np.repeat(g.rel_cnt, g.N)
    all_rows = lambda m: {"all": np.ones(m, bool)}
    want = wp.ref_fused_backward(g, d["dist"], d["P"], d["gn"], d["w"])
    S = wp.ref_fused_backward(g, d["dist"], d["P"], d["gn"], d["w"], absolute=True)
    yard = wp.f32_fused_backward(g, d["dist"], d["P"], d["gn"], d["w"])
    got = [x.cpu().numpy() for x in ops.aggregate_fused_backward(plan, t["dist"], t["P"], t["gn"])]
    per_row = np.bincount(g.row_of, minlength=g.rel_total)
    _rounding_class("aggregate_fused_backward g_dist " + gname, got[0], want[0], S[0], yard[0], deg * D, kq, all_rows(BN))
    for dd in (0, 1):
        _rounding_class("aggregate_fused_backward g_P[%d] %s" % (dd, gname), got[1][dd], want[1][dd], S[1][dd], yard[1][dd],
                        per_row, np.zeros(g.rel_total), all_rows(g.rel_total))
    want = wp.ref_unfused_backward(g, d["dist"], d["ins"], d["Tf"], d["Ti"], d["gagg"], d["w"])
    S = wp.ref_unfused_backward(g, d["dist"], d["ins"], d["Tf"], d["Ti"], d["gagg"], d["w"], absolute=True)
    yard = wp.f32_unfused_backward(g, d["dist"], d["ins"], d["Tf"], d["Ti"], d["gagg"], d["w"])
    I = d["ins"].shape[1]
    per_rel = np.bincount(g.r, minlength=g.R)
    per_q = np.bincount(g.h // g.N, minlength=g.B)
    for gather in (True, False):
        got = [x.cpu().numpy() for x in ops.aggregate_backward(plan, t["dist"], t["ins"], t["Tf"], t["Ti"], t["gagg"], gather=gather)]
        tag = " %s gather=%s" % (gname, gather)
        _rounding_class("aggregate_backward g_dist" + tag, got[0], want[0], S[0], yard[0], deg * D * I, kq, all_rows(BN))
        _rounding_class("aggregate_backward g_ins" + tag, got[1], want[1], S[1], yard[1], 2 * per_q, np.zeros(g.B), all_rows(g.B))
        _rounding_class("aggregate_backward g_T_fwd" + tag, got[2], want[2], S[2], yard[2], I * per_rel, np.zeros(g.R), all_rows(g.R))
        _rounding_class("aggregate_backward g_T_inv" + tag, got[3], want[3], S[3], yard[3], I * per_rel, np.zeros(g.R), all_rows(g.R))
    plan_t = _plan(g, dev, wrel=d["wrel"])
    for gather in (True, False):
        got = ops.typelayer_backward(plan_t, t["gn"], True, gather=gather).cpu().numpy()
        _rounding_class("typelayer_backward g_T %s gather=%s" % (gname, gather), got, wp.ref_typelayer_backward(g, d["gn"], d["wrel"]),
                        wp.ref_typelayer_backward(g, d["gn"], d["wrel"], absolute=True),
                        wp.f32_typelayer_backward(g, d["gn"], d["wrel"]), 2 * per_rel, np.zeros(g.R), all_rows(g.R))
