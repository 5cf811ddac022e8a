"""gnnrag_instructions in guarded buffers (tests/guarded.py, as tests/test_gpu_guarded.py does for the other entry points):
every buffer the binding allocates (``ops._buf``: ins_out, attn_out) and every input is an exact-sized view between two
64 KiB guards; the call runs with the buffers pre-filled with 0x00, with the leftovers of a call on other inputs and with
0xFF.  All guards and inputs must hold their bytes, and the three results and the unguarded one must be the same bits (the
outputs are fully written, nothing is accumulated into, one summation order)."""
import numpy as np
import pytest
import torch

import guarded
import instruction_oracle as io
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
TOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _tensors(dev, c):
    """The nine arguments as one flat list (the two lists of per-step parameters unrolled) plus r_in."""
    n = len(c["W_q"])
    flat = [c["hidden"], c["node"], c["mask"]] + c["W_q"] + c["b_q"] + [c["W_cq"], c["b_cq"], c["w_ca"], c["b_ca"]]
    return n, [torch.from_numpy(a).to(dev) for a in flat]


def _call(n, t, r_in=None):
    from gnnrag_amd import ops
    return ops.instructions(t[0], t[1], t[2], t[3:3 + n], t[3 + n:3 + 2 * n], *t[3 + 2 * n:], r_in=r_in)


# T D odd and D % 4 != 0 (scalar staging); T over 64 lanes with vector staging
@pytest.mark.parametrize("B,T,D,I", [(3, 7, 50, 3), (2, 70, 200, 2)])
def test_instructions_guarded(dev, monkeypatch, B, T, D, I):
    from gnnrag_amd import ops
    c = io.random_case(B, T, D, I, seed=3)
    other = io.random_case(B, T, D, I, seed=4)
    n, plain_in = _tensors(dev, c)
    _, other_in = _tensors(dev, other)
    r_in = torch.tanh(torch.randn(B, D, device=dev))
    plain = [[o.cpu() for o in _call(n, plain_in)], [o.cpu() for o in _call(n, plain_in, r_in)]]

    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    assert ops._buf == g.buf
    runs = []
    for fill, inp in ((FILL_ZERO, plain_in), (FILL_ZERO, other_in), (FILL_LEFTOVERS, plain_in), (FILL_ONES, plain_in)):
        g.fill = fill
        w = [g.wrap(t, "input %d" % i) for i, t in enumerate(inp)]
        wr = g.wrap(r_in, "input r_in")
        hits = g.leftover_hits
        out = [[o.cpu() for o in _call(n, w)], [o.cpu() for o in _call(n, w, wr)]]
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits > hits
        g.check("body fill %r%s" % (fill, "" if inp is plain_in else " (other inputs)"))
        if inp is plain_in:
            runs.append(out)
    assert set(g.sizes) == {"instructions: ins_out", "instructions: attn_out"}
    assert g.sizes["instructions: ins_out"] == I * B * D * 4 and g.sizes["instructions: attn_out"] == I * B * T * 4
    for out in runs:
        for got, want in zip(out, plain):
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    want_ins, want_attn = io.instructions(*[c[k] for k in io.ARGS])
    assert np.abs(runs[0][0][0].numpy() - want_ins).max() <= TOL
    assert np.abs(runs[0][0][1].numpy() - want_attn).max() <= TOL
    g.release()
