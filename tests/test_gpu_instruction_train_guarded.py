"""gnnrag_instructions_train and gnnrag_instructions_backward in guarded buffers (tests/guarded.py, as
tests/test_gpu_instruction_guarded.py does for the inference entry point): every buffer the binding allocates (``ops._buf``:
ins_out, attn_out, the reserve, every gradient, the backward's workspace) and every input is an exact-sized view between two
64 KiB guards; the calls run with the buffers pre-filled with 0x00, with the leftovers of a call on other inputs and with
0xFF.  All guards and inputs must hold their bytes, and the three results and the unguarded one must be the same bits: the
outputs and the reserve are fully written, nothing is accumulated into what a buffer held, one summation order."""
import numpy as np
import pytest
import torch

import guarded
import instruction_grad_oracle as igo
import instruction_oracle as io
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
TOL_KERNEL = 2e-5
KEYS = io.ARGS + ("r_in", "g_ins", "g_attn", "m1", "m2", "m3")


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _tensors(dev, c):
    to = lambda a: [torch.from_numpy(x).to(dev) for x in a] if isinstance(a, list) else torch.from_numpy(a).to(dev)  # noqa: E731
    return {k: to(c[k]) for k in KEYS}


def _wrap(g, t):
    return {k: ([g.wrap(x, "input %s[%d]" % (k, i)) for i, x in enumerate(v)] if isinstance(v, list) else
                g.wrap(v, "input " + k)) for k, v in t.items()}


def _call(t):
    """Forward and backward; everything they return as one flat list of host tensors."""
    from gnnrag_amd import ops
    masks = dict(drop_node=t["m1"], drop_cat=t["m2"], drop_tok=t["m3"])
    ins, attn, reserve = ops.instructions_train(*[t[k] for k in io.ARGS], r_in=t["r_in"], **masks)
    g = ops.instructions_backward(t["hidden"], t["node"], t["W_q"], t["W_cq"], t["w_ca"], ins, attn, reserve, t["g_ins"],
                                  t["g_attn"], r_in=t["r_in"], **masks)
    flat = [ins, attn, reserve] + [g[k] for k in ("dhidden", "dnode", "dr_in", "dW_cq", "db_cq", "dw_ca", "db_ca")]
    return [o.cpu() for o in flat + g["dW_q"] + g["db_q"]], g


# D % 4 != 0 (padded operand copies, the unpad copies); the encoder's shape (the products write the gradients directly)
@pytest.mark.parametrize("B,T,D,I", [(3, 5, 50, 3), (2, 12, 200, 2)])
def test_instructions_train_and_backward_guarded(dev, monkeypatch, B, T, D, I):
    from gnnrag_amd import ops
    c = igo.train_case(B, T, D, I, 0.2, seed=3)
    plain_in, other_in = _tensors(dev, c), _tensors(dev, igo.train_case(B, T, D, I, 0.2, seed=4))
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
    fwd, bwd = "instructions_train: ", "instructions_backward: "
    want_sizes = {fwd + "ins_out": I * B * D * 4, fwd + "attn_out": I * B * T * 4, fwd + "reserve": I * B * 2 * D * 4,
                  bwd + "dhidden": B * T * D * 4, bwd + "dnode": B * D * 4, bwd + "dr_in": B * D * 4, bwd + "dW_q": D * D * 4,
                  bwd + "db_q": D * 4, bwd + "dW_cq": D * 4 * D * 4, bwd + "db_cq": D * 4, bwd + "dw_ca": D * 4,
                  bwd + "db_ca": 4}
    assert set(g.sizes) == set(want_sizes) | {bwd + "workspace"}
    for role, size in want_sizes.items():
        assert g.sizes[role] == size, role
    assert g.sizes[bwd + "workspace"] == ops._lib.load().gnnrag_instructions_backward_workspace_bytes(B, T, D, I) > 256
    for out in runs:
        assert len(out) == len(plain)
        for i, (got, want) in enumerate(zip(out, plain)):
            assert got.shape == want.shape and got.numpy().tobytes() == want.numpy().tobytes(), "output %d" % i
    # and the guarded results are right
    _, _, saved = igo.forward(*[c[k] for k in io.ARGS], r_in=c["r_in"], m1=c["m1"], m2=c["m2"], m3=c["m3"])
    want = igo.backward(saved, c["g_ins"], c["g_attn"])
    g.fill = FILL_ONES
    _, got = _call(_wrap(g, plain_in))
    for k in ("dhidden", "dnode", "dr_in", "dW_cq", "db_cq", "dw_ca"):
        err, scale = np.abs(got[k].cpu().numpy() - want[k]).max(), max(np.abs(want[k]).max(), 1e-6)
        assert err <= TOL_KERNEL * scale, (k, err, scale)
    assert float(got["db_ca"][0]) == 0.0
    g.release()


def test_buffers_one_byte_short_are_refused_and_nothing_is_written(dev, monkeypatch):
    import re
    from gnnrag_amd import _lib, ops
    c = igo.train_case(3, 5, 50, 3, 0.2, seed=5)
    t = _tensors(dev, c)
    masks = dict(drop_node=t["m1"], drop_cat=t["m2"], drop_tok=t["m3"])
    ins, attn, reserve = ops.instructions_train(*[t[k] for k in io.ARGS], r_in=t["r_in"], **masks)
    g = guarded.Guard(dev, fill=FILL_ONES)
    guarded.install(monkeypatch, g)

    def fwd():
        return ops.instructions_train(*[t[k] for k in io.ARGS], r_in=t["r_in"], **masks)

    def bwd(res=reserve):
        return ops.instructions_backward(t["hidden"], t["node"], t["W_q"], t["W_cq"], t["w_ca"], ins, attn, res, t["g_ins"],
                                         t["g_attn"], r_in=t["r_in"], **masks)

    for role, fn in (("instructions_train: reserve", fwd), ("instructions_backward: workspace", bwd),
                     (None, lambda: bwd(reserve[:-1]))):
        g.short = {role: 1} if role else {}
        first = len(g.blocks)
        with pytest.raises(_lib.GnnragError) as e:
            fn()
        assert int(re.search(r"failed \((-?\d+)\)", str(e.value)).group(1)) == -3, role
        g.check("%s one byte short" % (role or "instructions_backward: reserve"))
        for b in g.blocks[first:]:                     # nothing was launched: every buffer still holds its 0xFF fill
            assert bool((b.raw[g.G: g.G + b.nbytes] == 0xFF).all()), (role, b.role)
    g.short = {}
    bwd()
    g.check("stated sizes again")
    g.release()
