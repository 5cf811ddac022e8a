"""gnnrag_linear_splitk and gnnrag_bert_encode_splitk in guarded buffers (tests/guarded.py): every buffer the binding
allocates (``ops._buf``: out, workspace) and every input is an exact-sized view between two 64 KiB guards; the call runs with
the buffers pre-filled with 0x00, with the leftovers of a call on other inputs and with 0xFF.  All guards and inputs must hold
their bytes and every run must give the bits of the unguarded call: the partial products are fully written before they are
read, nothing is accumulated into, one summation order."""
import numpy as np
import pytest
import torch

import bert_oracle as bo
import guarded
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
M, K, NOUT, SPLITS = 17, 100, 68, 3
EPS = 1e-12
B, T, L = 3, 9, 1


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _operands(dev, seed):
    rs = np.random.RandomState(seed)
    f = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(dev)
    return dict(A=f(M, K), W=f(NOUT, K) * 0.05, bias=f(NOUT) * 0.1, add=f(M, NOUT), g=1.0 + f(NOUT) * 0.1, b=f(NOUT) * 0.1)


def _call(d, epi, alias=False):
    from gnnrag_amd import ops
    kw = dict(add=d["add"], ln=(d["g"], d["b"], EPS)) if epi == "add_ln" else {}
    if alias:
        kw["out"] = d["add"]
    return ops.linear_splitk(d["A"], d["W"], d["bias"], epi=epi, splits=SPLITS, **kw)


@pytest.mark.parametrize("epi", ["bias", "gelu", "add_ln"])
def test_linear_splitk_guarded_fills(dev, monkeypatch, epi):
    from gnnrag_amd import _lib, ops
    assert ops.linear_splitk_plan(M, K, NOUT, SPLITS).splits == SPLITS
    d, other = _operands(dev, 31), _operands(dev, 32)
    plain = _call(d, epi).cpu()
    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    assert ops._buf == g.buf
    wrap = lambda ops_: {k: g.wrap(v, k) for k, v in ops_.items()}
    gd, gother = wrap(d), wrap(other)
    for fill, inp in ((FILL_ZERO, gd), (FILL_ZERO, gother), (FILL_LEFTOVERS, gd), (FILL_ONES, gd)):
        g.fill = fill
        hits = g.leftover_hits
        out = _call(inp, epi).cpu()
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits > hits
        g.check("%s, body fill %r%s" % (epi, fill, "" if inp is gd else " (other inputs)"))
        if inp is gd:
            assert torch.equal(out, plain), fill
    assert g.sizes == {"linear_splitk: out": M * NOUT * 4,
                       "linear_splitk: workspace": _lib.load().gnnrag_linear_splitk_workspace_bytes(M, K, NOUT, SPLITS)}
    if epi == "add_ln":
        # C is the buffer of add: the guarded copy of add is written, and only it (its block is taken out of the
        # "inputs keep their bytes" check by wrapping a fresh one and forgetting its copy)
        g.fill = FILL_ONES
        fresh = g.wrap(d["add"], "add / out")
        g.blocks[-1].copy = None
        out = _call({**gd, "add": fresh}, epi, alias=True)
        g.check("add_ln into add")
        assert out is fresh and torch.equal(out.cpu(), plain)
    g.release()


@pytest.fixture(scope="module")
def case():
    pytest.importorskip("transformers")
    m32, m64 = bo.make_model(bo.config(L=L, vocab=64, max_pos=16, **bo.MINILM), seed=21)
    rs = np.random.RandomState(22)
    ids, other = rs.randint(0, 64, (B, T)), rs.randint(0, 64, (B, T))
    want = bo.states(m64, ids)
    return m32, ids, other, want, bo.rel_err(bo.states(m32, ids), want)


def _args(dev, model, wrap=None):
    P = bo.layer_params(model)
    w = (lambda t, role: t) if wrap is None else wrap
    top = {k: w(P[k].detach().to(dev), k) for k in ("word_emb", "pos_emb", "type_emb", "ln_g", "ln_b")}
    layers = [{k: w(v.detach().to(dev), "layers[%d].%s" % (i, k)) for k, v in d.items()} for i, d in enumerate(P["layers"])]
    return top, layers, P


def _encode(top, layers, P, ids):
    from gnnrag_amd import ops
    return ops.bert_encode(ids, top["word_emb"], top["pos_emb"], top["type_emb"], top["ln_g"], top["ln_b"], P["eps"], layers,
                           P["heads"], I=P["I"], splitk=True)


def test_encode_splitk_guarded_fills(dev, monkeypatch, case):
    from gnnrag_amd import _lib, ops
    m32, ids, other, want, e_ref = case
    top, layers, P = _args(dev, m32)
    ids_d, other_d = torch.from_numpy(ids).long().to(dev), torch.from_numpy(other).long().to(dev)
    plain = _encode(top, layers, P, ids_d).cpu()
    err = bo.rel_err(plain.numpy(), want)
    print("guarded split-K case: err %.3g, e_ref %.3g, bound %.3g" % (err, e_ref, bo.bound(e_ref)))
    assert err <= bo.bound(e_ref)
    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    assert ops._buf == g.buf
    gtop, glayers, _ = _args(dev, m32, g.wrap)
    for fill, inp in ((FILL_ZERO, ids_d), (FILL_ZERO, other_d), (FILL_LEFTOVERS, ids_d), (FILL_ONES, ids_d)):
        g.fill = fill
        gi = g.wrap(inp, "ids")
        hits = g.leftover_hits
        out = _encode(gtop, glayers, P, gi).cpu()
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits > hits
        g.check("encode, body fill %r%s" % (fill, "" if inp is ids_d else " (other inputs)"))
        if inp is ids_d:
            assert torch.equal(out, plain), fill
    assert g.sizes == {"bert_encode: out": B * T * 384 * 4,
                       "bert_encode: workspace": _lib.load().gnnrag_bert_splitk_workspace_bytes(B, T, 384, 1536)}
    g.release()
