"""gnnrag_relation_tables_backward in guarded buffers (tests/guarded.py): every buffer the binding allocates (``ops._buf``: the
four gradients and the workspace) and every input is an exact-sized view between two 64 KiB guards; the call runs with the
buffers pre-filled with 0x00, with the leftovers of a call on other inputs and with 0xFF, on the default and on another
stream.  All guards and inputs must hold their bytes, the buffer sizes are exact, and the results and the unguarded one must
be the same bits: every element of every output is written and nothing depends on what a buffer or the workspace held."""
import ctypes
import re

import numpy as np
import pytest
import torch

import guarded
import rel_tables_grad_oracle as ro
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
TOL_KERNEL = 2e-5
OUTS = ("g_T_fwd", "g_T_inv", "g_ins", "g_W")


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _structure(dev, B, N, E, R, D, I, **kw):
    from gnnrag_amd import ops, synth
    cfg = synth.GraphConfig(name="guarded", B=B, N=N, E=E, R=R, D=D, I=I, seed=13, **kw)
    et = synth.make_batch(cfg).edge_tuple
    plan = ops.CsrPlan(et[0], et[1], et[2], cfg.B, cfg.N, cfg.R1, dev)
    return plan, plan.rel_rows().astype(np.int64), cfg


def _tensors(dev, c):
    return {k: torch.from_numpy(v).to(dev) for k, v in c.items()}


def _wrap(g, t):
    return {k: g.wrap(v, "input " + k) for k, v in t.items()}


def _call(plan, t, math):
    from gnnrag_amd import ops
    got = ops.relation_tables_backward(plan, t["T_fwd"], t["T_inv"], t["ins"], t["W"], t["g_P"], math=math)
    return [got[k].cpu() for k in OUTS]


# partial column tiles with three instructions (skinny product); past the skinny kernel's rows, several gemm_tn chunks
@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("shape", [dict(B=4, N=40, E=90, R=7, D=52, I=3, n_real_min=5),
                                   dict(B=17, N=64, E=8000, R=1000, D=4, I=1, zipf_heads=False)], ids=["d52", "big"])
def test_relation_tables_backward_guarded(dev, monkeypatch, shape, math):
    from gnnrag_amd import ops
    plan, rows, cfg = _structure(dev, **shape)
    R1, B, D, I, M = cfg.R1, cfg.B, cfg.D, cfg.I, plan.rel_total
    K = (2 * I + 1) * D
    c = ro.case(rows, R1, B, D, I, seed=3)
    plain_in, other_in = _tensors(dev, c), _tensors(dev, ro.case(rows, R1, B, D, I, seed=4))
    plain = _call(plan, plain_in, math)

    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    assert ops._buf == g.buf
    side = torch.cuda.Stream(device=dev)
    runs = []
    for fill, inp, stream in ((FILL_ZERO, plain_in, None), (FILL_ZERO, other_in, None), (FILL_LEFTOVERS, plain_in, None),
                              (FILL_ONES, plain_in, None), (FILL_ONES, plain_in, side)):
        g.fill = fill
        hits = g.leftover_hits
        wrapped = _wrap(g, inp)
        if stream is None:
            out = _call(plan, wrapped, math)
        else:
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                out = _call(plan, wrapped, math)
            stream.synchronize()
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits > hits
        g.check("body fill %r%s%s" % (fill, "" if inp is plain_in else " (other inputs)", "" if stream is None else " (side stream)"))
        if inp is plain_in:
            runs.append(out)
    role = "relation_tables_backward: "
    want_sizes = {role + "g_T_fwd": R1 * D * 4, role + "g_T_inv": R1 * D * 4, role + "g_ins": B * I * D * 4,
                  role + "g_W": D * K * 4}
    assert set(g.sizes) == set(want_sizes) | {role + "workspace"}
    for r, size in want_sizes.items():
        assert g.sizes[r] == size, r
    need = ops._lib.load().gnnrag_relation_tables_backward_workspace_bytes(ctypes.byref(plan.c), D, I)
    assert g.sizes[role + "workspace"] == need >= (K * D + 2 * I * M * D + 2 * D * I * D) * 4
    for out in runs:
        assert len(out) == len(plain)
        for i, (got, want) in enumerate(zip(out, plain)):
            assert got.shape == want.shape and got.numpy().tobytes() == want.numpy().tobytes(), OUTS[i]
    # and the guarded results are right
    want = ro.backward(rows, R1, B, c["T_fwd"], c["T_inv"], c["ins"], c["W"], c["g_P"])
    for k, got in zip(OUTS, runs[-1]):
        err, scale = np.abs(got.numpy() - want[k]).max(), max(np.abs(want[k]).max(), 1e-6)
        assert err <= TOL_KERNEL * scale, (k, err, scale)
    g.release()


def test_a_workspace_stated_one_byte_short_is_refused_and_nothing_is_written(dev, monkeypatch):
    from gnnrag_amd import _lib, ops
    plan, rows, cfg = _structure(dev, B=4, N=40, E=90, R=7, D=52, I=3, n_real_min=5)
    t = _tensors(dev, ro.case(rows, cfg.R1, cfg.B, cfg.D, cfg.I, seed=5))
    g = guarded.Guard(dev, fill=FILL_ONES)
    guarded.install(monkeypatch, g)

    def bwd():
        return ops.relation_tables_backward(plan, t["T_fwd"], t["T_inv"], t["ins"], t["W"], t["g_P"])

    g.short = {"relation_tables_backward: workspace": 1}
    first = len(g.blocks)
    with pytest.raises(_lib.GnnragError) as e:
        bwd()
    assert int(re.search(r"failed \((-?\d+)\)", str(e.value)).group(1)) == -3
    g.check("workspace one byte short")
    assert len(g.blocks) - first == 5                  # the four gradients and the workspace
    for b in g.blocks[first:]:                         # nothing was launched: every buffer still holds its 0xFF fill
        assert bool((b.raw[g.G: g.G + b.nbytes] == 0xFF).all()), b.role
    g.short = {}
    bwd()
    g.check("stated size again")
    g.release()
