"""gnnrag_layer_tail_train and gnnrag_layer_tail_backward in guarded buffers (tests/guarded.py): every buffer the binding
allocates (``ops._buf``: h, score, dist, g_pre, dw, db, the backward's workspace) and every input is an exact-sized view
between two 64 KiB guards; the calls run with the buffers pre-filled with 0x00, with the leftovers of a call on other inputs
and with 0xFF.  All guards and inputs must hold their bytes, and the three results and the unguarded one must be the same
bits: ``g_pre`` in particular is fully written and nothing is accumulated into what a buffer held."""
import re

import numpy as np
import pytest
import torch

import guarded
import layer_tail_oracle as lo
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


def _call(t):
    """Forward and backward; everything they return as one flat list of host tensors."""
    from gnnrag_amd import ops
    h, score, dist = ops.layer_tail_train(t["pre_a"], t["pre_b"], t["keep"], t["scale"], t["w"], t["b"], t["mask"])
    g = ops.layer_tail_backward(h, dist, t["keep"], t["scale"], t["w"], t["g_h"], t["g_dist"])
    return [o.cpu() for o in (h, score, dist, g["g_pre"], g["dw"], g["db"])], g


# D % 4 != 0 (the element form of the row kernels); the trainer's hidden size (float4 accesses)
@pytest.mark.parametrize("B,N,D", [(3, 70, 50), (2, 130, 200)])
def test_layer_tail_train_and_backward_guarded(dev, monkeypatch, B, N, D):
    from gnnrag_amd import ops
    c = lo.case(B, N, D, seed=3, p=0.2)
    plain_in, other_in = _tensors(dev, c), _tensors(dev, lo.case(B, N, D, seed=4, p=0.2))
    plain, _ = _call(plain_in)

    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    assert ops._buf == g.buf
    runs = []
    for fill, inp in ((FILL_ZERO, plain_in), (FILL_ZERO, other_in), (FILL_LEFTOVERS, plain_in), (FILL_ONES, plain_in)):
        g.fill = fill
        hits = g.leftover_hits
        out, _ = _call(_wrap(g, inp))
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits > hits
        g.check("body fill %r%s" % (fill, "" if inp is plain_in else " (other inputs)"))
        if inp is plain_in:
            runs.append(out)
    fwd, bwd = "layer_tail_train: ", "layer_tail_backward: "
    want_sizes = {fwd + "h": B * N * D * 4, fwd + "score": B * N * 4, fwd + "dist": B * N * 4, bwd + "g_pre": B * N * D * 4,
                  bwd + "dw": D * 4, bwd + "db": 4}
    assert set(g.sizes) == set(want_sizes) | {bwd + "workspace"}
    for role, size in want_sizes.items():
        assert g.sizes[role] == size, role
    assert g.sizes[bwd + "workspace"] == ops._lib.load().gnnrag_layer_tail_backward_workspace_bytes(B, N, D) > 256
    for out in runs:
        assert len(out) == len(plain)
        for i, (got, want) in enumerate(zip(out, plain)):
            assert got.shape == want.shape and got.numpy().tobytes() == want.numpy().tobytes(), "output %d" % i
    # and the guarded results are right
    h, _, _, dist = lo.forward(c["pre_a"], c["pre_b"], c["keep"], c["scale"], c["w"], c["b"], c["mask"])
    want = lo.backward(h, dist, c["keep"], c["scale"], c["w"], c["g_h"], c["g_dist"])
    g.fill = FILL_ONES
    _, got = _call(_wrap(g, plain_in))
    for k in ("g_pre", "dw"):
        err, scale = np.abs(got[k].cpu().numpy() - want[k]).max(), max(np.abs(want[k]).max(), 1e-6)
        assert err <= TOL_KERNEL * scale, (k, err, scale)
    assert float(got["db"].item()) == 0.0
    g.release()


def test_a_workspace_stated_four_bytes_short_is_refused_and_nothing_is_written(dev, monkeypatch):
    from gnnrag_amd import _lib, ops
    t = _tensors(dev, lo.case(3, 70, 50, seed=5, p=0.2))
    h, _, dist = ops.layer_tail_train(t["pre_a"], t["pre_b"], t["keep"], t["scale"], t["w"], t["b"], t["mask"])
    g = guarded.Guard(dev, fill=FILL_ONES)
    guarded.install(monkeypatch, g)

    def bwd():
        return ops.layer_tail_backward(h, dist, t["keep"], t["scale"], t["w"], t["g_h"], t["g_dist"])

    g.short = {"layer_tail_backward: workspace": 4}
    first = len(g.blocks)
    with pytest.raises(_lib.GnnragError) as e:
        bwd()
    assert int(re.search(r"failed \((-?\d+)\)", str(e.value)).group(1)) == -3
    g.check("workspace four bytes short")
    assert len(g.blocks) - first == 4                  # g_pre, dw, db, workspace
    for b in g.blocks[first:]:                         # nothing was launched: every buffer still holds its 0xFF fill
        assert bool((b.raw[g.G: g.G + b.nbytes] == 0xFF).all()), b.role
    g.short = {}
    bwd()
    g.check("stated size again")
    g.release()
