"""gnnrag_bert_layers_forward_save / gnnrag_bert_layers_backward in guarded buffers (tests/guarded.py): every input - the
keep buffers and the reserve included - and every buffer the binding allocates (``ops._buf``: out, reserve, workspaces, g_x0
and the parameter gradients) is an exact-sized view between two 64 KiB guards; the calls run with the allocated buffers
pre-filled with 0x00, with the leftovers of a call on other inputs and with 0xFF, and on a non-default stream.  All guards and
inputs must hold their bytes and every run must give the bits of the unguarded call (every output is fully written, nothing
is accumulated into, one summation order)."""
import numpy as np
import pytest
import torch

import bert_dropout_oracle as do
import bert_oracle as bo
import guarded
import lm_variants_oracle as lo
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
B, T, L = 3, 9, 2
P_HIDDEN, P_ATT = 0.5, 0.3
SHAPE = bo.MINILM


@pytest.fixture(scope="module")
def dev():
    pytest.importorskip("transformers")
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _inputs(dev, seed):
    rs = np.random.RandomState(seed)
    H = SHAPE["H"]
    x0 = torch.from_numpy(rs.standard_normal((B, T, H)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rs.standard_normal((B, T, H)).astype(np.float32)).to(dev)
    kh, ka = do.pack(do.draw(seed + 1, L, B, T, H, SHAPE["heads"], P_HIDDEN, P_ATT), L)
    return x0, g, torch.from_numpy(kh).to(dev), torch.from_numpy(ka).to(dev)


def _run(ops, layers, P, x0, g, kh, ka, wrap):
    kw = dict(keep_hidden=wrap(kh, "keep_hidden"), scale_hidden=do.scale(P_HIDDEN), keep_att=wrap(ka, "keep_att"),
              scale_att=do.scale(P_ATT))
    lay = [{k: wrap(v, "layers[%d].%s" % (i, k)) for k, v in d.items()} for i, d in enumerate(layers)]
    out, reserve = ops.bert_layers_forward_save(wrap(x0, "x0"), lay, P["heads"], P["eps"], B, T, **kw)
    g_x0, grads = ops.bert_layers_backward(wrap(g, "g_out"), lay, P["heads"], P["eps"], B, T, wrap(reserve, "reserve"), **kw)
    return [out, g_x0] + [grads[l][k] for l in range(L) for k in ops.BERT_GRAD_FIELDS]


def test_forward_save_and_backward_guarded_fills_and_stream(dev, monkeypatch):
    from gnnrag_amd import _lib, ops
    m32, _ = do.make_bert(SHAPE, L, seed=71, max_pos=16)
    P = lo.layer_params(m32, T)
    layers = [{k: v.detach().to(dev) for k, v in d.items()} for d in P["layers"]]
    one, other = _inputs(dev, 72), _inputs(dev, 74)
    plain = [t.cpu() for t in _run(ops, layers, P, *one, wrap=lambda t, role: t)]
    assert all(torch.isfinite(t).all() for t in plain)

    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    assert ops._buf == g.buf
    runs = []
    for fill, inp in ((FILL_ZERO, one), (FILL_ZERO, other), (FILL_LEFTOVERS, one), (FILL_ONES, one)):
        g.fill = fill
        hits = g.leftover_hits
        outs = [t.cpu() for t in _run(ops, layers, P, *inp, wrap=g.wrap)]
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits > hits
        g.check("body fill %r%s" % (fill, "" if inp is one else " (other inputs)"))
        if inp is one:
            runs.append(outs)
    lib, H, I, heads = _lib.load(), SHAPE["H"], SHAPE["I"], SHAPE["heads"]
    assert g.sizes["bert_layers_forward_save: reserve"] == lib.gnnrag_bert_reserve_bytes(L, B, T, H, I)
    assert g.sizes["bert_layers_forward_save: workspace"] == lib.gnnrag_bert_workspace_bytes(B, T, H, I)
    assert g.sizes["bert_layers_backward: workspace"] == lib.gnnrag_bert_layers_backward_workspace_bytes(B, T, H, heads, I)
    assert {"bert_layers_forward_save: out", "bert_layers_backward: g_x0", "bert_layers_backward: dW_qkv",
            "bert_layers_backward: dln2_b"} <= set(g.sizes)
    for outs in runs:
        assert all(torch.equal(a, b) for a, b in zip(outs, plain))
    # a non-default stream
    g.fill = FILL_ONES
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        outs = _run(ops, layers, P, *one, wrap=g.wrap)
    side.synchronize()
    g.check("side stream")
    assert all(torch.equal(a.cpu(), b) for a, b in zip(outs, plain))
    g.release()


def test_short_reserve_and_workspace_are_refused(dev, monkeypatch):
    """A reserve or a workspace one byte short is GNNRAG_E_WORKSPACE before anything is launched: no guard is touched."""
    from gnnrag_amd import _lib, ops
    m32, _ = do.make_bert(SHAPE, L, seed=71, max_pos=16)
    P = lo.layer_params(m32, T)
    layers = [{k: v.detach().to(dev) for k, v in d.items()} for d in P["layers"]]
    x0, gr, kh, ka = _inputs(dev, 72)
    _, reserve = ops.bert_layers_forward_save(x0, layers, P["heads"], P["eps"], B, T)
    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    for role, call in (("bert_layers_forward_save: reserve",
                        lambda: ops.bert_layers_forward_save(x0, layers, P["heads"], P["eps"], B, T)),
                       ("bert_layers_forward_save: workspace",
                        lambda: ops.bert_layers_forward_save(x0, layers, P["heads"], P["eps"], B, T)),
                       ("bert_layers_backward: workspace",
                        lambda: ops.bert_layers_backward(gr, layers, P["heads"], P["eps"], B, T, reserve))):
        g.short = {role: 1}
        with pytest.raises(_lib.GnnragError) as e:
            call()
        assert e.value.code == -3
        g.check("short " + role)
    g.short = {}
    with pytest.raises(_lib.GnnragError) as e:
        ops.bert_layers_backward(gr, layers, P["heads"], P["eps"], B, T, reserve[:-1])
    assert e.value.code == -3
    g.check("short reserve of the backward")
    g.release()
