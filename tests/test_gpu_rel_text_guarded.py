"""gnnrag_rel_text_pool / gnnrag_rel_text_pool_backward in guarded buffers (tests/guarded.py, as
tests/test_gpu_instruction_guarded.py does for gnnrag_instructions): every buffer the binding allocates (``ops._buf``:
outputs, xbar, alpha, the two workspaces - of exactly the stated size) and every input is an exact-sized view between two
64 KiB guards; the calls run with the buffers pre-filled with 0x00, with the leftovers of a call on other inputs and with
0xFF.  All guards and inputs must hold their bytes, and the three results and the unguarded one must be the same bits (the
outputs are fully written, nothing is accumulated into, one summation order)."""
import pytest
import torch

import guarded
import rel_text_oracle as ro
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _tensors(dev, c):
    return [torch.from_numpy(a).to(dev) for a in c["Xs"] + [c["mask"], c["W"], c["b"], c["a"]] + c["gs"]]


def _call(t, n_dir):
    """Forward (saving) and backward; every result as a CPU tensor, None where there is none."""
    from gnnrag_amd import ops
    Xf, Xi, mask, W, b, a, gf, gi = t
    if n_dir == 1:
        Xi = gi = None
    of, oi, xbar, alpha = ops.rel_text_pool(Xf, Xi, mask, W, b, a, save=True)
    fwd_only = ops.rel_text_pool(Xf, Xi, mask, W, b, a)[:2]
    dW, db, da = ops.rel_text_pool_backward(Xf, Xi, W, a, xbar, alpha, gf, gi)
    return [None if o is None else o.cpu() for o in (of, oi, xbar, alpha, fwd_only[0], fwd_only[1], dW, db, da)]


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n_dir", [1, 2])
@pytest.mark.parametrize("R,T,K,D", [(37, 5, 20, 12), (130, 12, 384, 50)])
def test_rel_text_guarded(dev, monkeypatch, R, T, K, D, n_dir):
    from gnnrag_amd import _lib, ops
    lib = _lib.load()
    plain_in = _tensors(dev, ro.random_case(R, T, K, D, seed=3))
    other_in = _tensors(dev, ro.random_case(R, T, K, D, seed=4))
    plain = _call(plain_in, n_dir)
    assert _same(plain[:2], plain[4:6])                       # forward only = the saving forward

    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    assert ops._buf == g.buf
    runs = []
    for fill, inp in ((FILL_ZERO, plain_in), (FILL_ZERO, other_in), (FILL_LEFTOVERS, plain_in), (FILL_ONES, plain_in)):
        g.fill = fill
        w = [g.wrap(t, "input %d" % i) for i, t in enumerate(inp)]
        hits = g.leftover_hits
        out = _call(w, n_dir)
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits > hits
        g.check("body fill %r%s" % (fill, "" if inp is plain_in else " (other inputs)"))
        if inp is plain_in:
            runs.append(out)
    roles = {"rel_text_pool: out_fwd": R * D * 4, "rel_text_pool: xbar": n_dir * R * K * 4,
             "rel_text_pool: alpha": n_dir * R * T * 4,
             "rel_text_pool: workspace": lib.gnnrag_rel_text_workspace_bytes(R, T, K, D, n_dir),
             "rel_text_pool_backward: dW": D * K * 4, "rel_text_pool_backward: db": D * 4,
             "rel_text_pool_backward: da": D * 4,
             "rel_text_pool_backward: workspace": lib.gnnrag_rel_text_backward_workspace_bytes(R, T, K, D, n_dir)}
    if n_dir == 2:
        roles["rel_text_pool: out_inv"] = R * D * 4
    assert g.sizes == roles
    for out in runs:
        assert _same(out, plain)
    g.release()
