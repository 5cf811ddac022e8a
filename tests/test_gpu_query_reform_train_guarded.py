"""gnnrag_query_reform_train and gnnrag_query_reform_backward in guarded buffers (tests/guarded.py): every buffer the binding
allocates (``ops._buf``: out, the reserve, every gradient, the backward's workspace) and every input is an exact-sized view
between two 64 KiB guards; the calls run with the buffers pre-filled with 0x00, with the leftovers of a call on other inputs
and with 0xFF.  All guards and inputs must hold their bytes, and the three results and the unguarded one must be the same
bits: ``d_ent`` in particular is fully written and nothing is accumulated into what a buffer held."""
import numpy as np
import pytest
import torch

import guarded
import query_reform_grad_oracle as qo
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
    to = lambda a: [torch.from_numpy(x).to(dev) for x in a] if isinstance(a, list) else torch.from_numpy(a).to(dev)  # noqa: E731
    t = {k: to(v) for k, v in c.items()}
    t["G"] = list(t["G"].unbind(0))
    return t


def _wrap(g, t):
    return {k: ([g.wrap(x, "input %s[%d]" % (k, i)) for i, x in enumerate(v)] if isinstance(v, list) else
                g.wrap(v, "input " + k)) for k, v in t.items()}


def _call(t):
    """Forward and backward; everything they return as one flat list of host tensors."""
    from gnnrag_amd import ops
    out, reserve = ops.query_reform_train(t["qs"], t["seed"], t["ent"], t["W_rs"], t["W_gs"])
    g = ops.query_reform_backward(t["qs"], t["seed"], t["W_rs"], t["W_gs"], reserve, t["G"])
    return [o.cpu() for o in [out, reserve, g["d_ent"]] + g["dq"] + g["dW_r"] + g["dW_g"]], g


# D % 4 != 0 (the scalar form of the node-state pass); the trainer's hidden size (float4 stores)
@pytest.mark.parametrize("B,N,D,n", [(3, 70, 50, 3), (2, 130, 200, 2)])
def test_query_reform_train_and_backward_guarded(dev, monkeypatch, B, N, D, n):
    from gnnrag_amd import ops
    c = qo.train_case(B, N, D, n, seed=3)
    plain_in, other_in = _tensors(dev, c), _tensors(dev, qo.train_case(B, N, D, n, seed=4))
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
    fwd, bwd = "query_reform_train: ", "query_reform_backward: "
    want_sizes = {fwd + "out": n * B * D * 4, fwd + "reserve": (B * D + n * B * 2 * D) * 4, bwd + "dq": B * D * 4,
                  bwd + "dW_r": D * 3 * D * 4, bwd + "dW_g": D * 3 * D * 4, bwd + "d_ent": B * N * D * 4}
    assert set(g.sizes) == set(want_sizes) | {bwd + "workspace"}
    for role, size in want_sizes.items():
        assert g.sizes[role] == size, role
    assert g.sizes[bwd + "workspace"] == ops._lib.load().gnnrag_query_reform_backward_workspace_bytes(B, N, D, n) > 256
    for out in runs:
        assert len(out) == len(plain)
        for i, (got, want) in enumerate(zip(out, plain)):
            assert got.shape == want.shape and got.numpy().tobytes() == want.numpy().tobytes(), "output %d" % i
    # and the guarded results are right
    _, saved = qo.forward(c["qs"], c["seed"], c["ent"], c["W_rs"], c["W_gs"])
    want = qo.backward(saved, list(c["G"]))
    g.fill = FILL_ONES
    _, got = _call(_wrap(g, plain_in))
    pairs = [("d_ent", got["d_ent"], want["d_ent"])]
    for k in ("dq", "dW_r", "dW_g"):
        pairs += [("%s[%d]" % (k, j), got[k][j], want[k][j]) for j in range(n)]
    for k, a, w in pairs:
        err, scale = np.abs(a.cpu().numpy() - w).max(), max(np.abs(w).max(), 1e-6)
        assert err <= TOL_KERNEL * scale, (k, err, scale)
    assert not got["d_ent"].cpu().numpy()[c["seed"] == 0].any()
    g.release()


def test_buffers_one_byte_short_are_refused_and_nothing_is_written(dev, monkeypatch):
    import re
    from gnnrag_amd import _lib, ops
    t = _tensors(dev, qo.train_case(3, 70, 50, 3, seed=5))
    _, reserve = ops.query_reform_train(t["qs"], t["seed"], t["ent"], t["W_rs"], t["W_gs"])
    g = guarded.Guard(dev, fill=FILL_ONES)
    guarded.install(monkeypatch, g)

    def fwd():
        return ops.query_reform_train(t["qs"], t["seed"], t["ent"], t["W_rs"], t["W_gs"])

    def bwd(res=reserve):
        return ops.query_reform_backward(t["qs"], t["seed"], t["W_rs"], t["W_gs"], res, t["G"])

    for role, fn in (("query_reform_train: reserve", fwd), ("query_reform_backward: workspace", bwd),
                     (None, lambda: bwd(reserve[:-1]))):
        g.short = {role: 1} if role else {}
        first = len(g.blocks)
        with pytest.raises(_lib.GnnragError) as e:
            fn()
        assert int(re.search(r"failed \((-?\d+)\)", str(e.value)).group(1)) == -3, role
        g.check("%s one byte short" % (role or "query_reform_backward: reserve"))
        for b in g.blocks[first:]:                     # nothing was launched: every buffer still holds its 0xFF fill
            assert bool((b.raw[g.G: g.G + b.nbytes] == 0xFF).all()), (role, b.role)
    g.short = {}
    bwd()
    g.check("stated sizes again")
    g.release()
