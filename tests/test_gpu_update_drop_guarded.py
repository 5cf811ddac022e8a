"""gnnrag_update_drop_train and gnnrag_update_drop_backward in guarded buffers (tests/guarded.py): every buffer the binding
allocates (``ops._buf``: pre, g_h, g_agg, dW, db, the backward's workspace) and every input is an exact-sized view between two
64 KiB guards; the calls run with the buffers pre-filled with 0x00, with the leftovers of a call on other inputs and with
0xFF.  All guards and inputs must hold their bytes, the buffer sizes are exact, and the three results and the unguarded one
must be the same bits: every element of every output is written and nothing is accumulated into what a buffer held."""
import re

import numpy as np
import pytest
import torch

import guarded
import update_drop_oracle as uo
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
TOL_KERNEL = 2e-5


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _tensors(dev, c):
    return {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def _wrap(g, t):
    return {k: (g.wrap(v, "input " + k) if isinstance(v, torch.Tensor) else v) for k, v in t.items()}


def _call(t, math):
    """Forward and backward; everything they return as one flat list of host tensors."""
    from gnnrag_amd import ops
    pre = ops.update_drop_train(t["h"], t["agg"], t["keep"], t["scale"], t["W"], t["b"], math=math)
    g = ops.update_drop_backward(t["g_pre"], t["h"], t["agg"], t["keep"], t["scale"], t["W"], math=math)
    return [o.cpu() for o in (pre, g["g_h"], g["g_agg"], g["dW"], g["db"])], g


# partial tiles, 4 column tiles; the trainer's K = 1400 with its seven input-gradient column blocks
@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("BN,D,I", [(70, 52, 2), (260, 200, 3)])
def test_update_drop_train_and_backward_guarded(dev, monkeypatch, BN, D, I, math):
    from gnnrag_amd import ops
    K = (2 * I + 1) * D
    c = uo.case(BN, D, I, 0.2, seed=3)
    plain_in, other_in = _tensors(dev, c), _tensors(dev, uo.case(BN, D, I, 0.2, seed=4))
    plain, _ = _call(plain_in, math)

    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    assert ops._buf == g.buf
    runs = []
    for fill, inp in ((FILL_ZERO, plain_in), (FILL_ZERO, other_in), (FILL_LEFTOVERS, plain_in), (FILL_ONES, plain_in)):
        g.fill = fill
        hits = g.leftover_hits
        out, _ = _call(_wrap(g, inp), math)
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits > hits
        g.check("body fill %r%s" % (fill, "" if inp is plain_in else " (other inputs)"))
        if inp is plain_in:
            runs.append(out)
    fwd, bwd = "update_drop_train: ", "update_drop_backward: "
    want_sizes = {fwd + "pre": BN * D * 4, bwd + "g_h": BN * D * 4, bwd + "g_agg": BN * (K - D) * 4, bwd + "dW": D * K * 4,
                  bwd + "db": D * 4}
    assert set(g.sizes) == set(want_sizes) | {bwd + "workspace"}
    for role, size in want_sizes.items():
        assert g.sizes[role] == size, role
    assert g.sizes[bwd + "workspace"] == ops._lib.load().gnnrag_update_drop_backward_workspace_bytes(BN, D, I) >= 2 * D * K * 4
    for out in runs:
        assert len(out) == len(plain)
        for i, (got, want) in enumerate(zip(out, plain)):
            assert got.shape == want.shape and got.numpy().tobytes() == want.numpy().tobytes(), "output %d" % i
    # and the guarded results are right
    want = dict(pre=uo.forward(c["h"], c["agg"], c["keep"], c["scale"], c["W"], c["b"]))
    want.update(uo.backward(c["g_pre"], c["h"], c["agg"], c["keep"], c["scale"], c["W"]))
    g.fill = FILL_ONES
    out, _ = _call(_wrap(g, plain_in), math)
    for k, got in zip(("pre", "g_h", "g_agg", "dW", "db"), out):
        err, scale = np.abs(got.numpy() - want[k]).max(), max(np.abs(want[k]).max(), 1e-6)
        assert err <= TOL_KERNEL * scale, (k, err, scale)
    g.release()


def test_a_workspace_stated_four_bytes_short_is_refused_and_nothing_is_written(dev, monkeypatch):
    from gnnrag_amd import _lib, ops
    t = _tensors(dev, uo.case(70, 52, 2, 0.2, seed=5))
    g = guarded.Guard(dev, fill=FILL_ONES)
    guarded.install(monkeypatch, g)

    def bwd():
        return ops.update_drop_backward(t["g_pre"], t["h"], t["agg"], t["keep"], t["scale"], t["W"])

    g.short = {"update_drop_backward: workspace": 4}
    first = len(g.blocks)
    with pytest.raises(_lib.GnnragError) as e:
        bwd()
    assert int(re.search(r"failed \((-?\d+)\)", str(e.value)).group(1)) == -3
    g.check("workspace four bytes short")
    assert len(g.blocks) - first == 5                  # g_h, g_agg, dW, db, workspace
    for b in g.blocks[first:]:                         # nothing was launched: every buffer still holds its 0xFF fill
        assert bool((b.raw[g.G: g.G + b.nbytes] == 0xFF).all()), b.role
    g.short = {}
    bwd()
    g.check("stated size again")
    g.release()
