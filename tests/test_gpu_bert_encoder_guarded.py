"""gnnrag_bert_encode / gnnrag_bert_attention in guarded buffers (tests/guarded.py): every buffer the binding allocates
(``ops._buf``: out, workspace, ctx) and every input is an exact-sized view between two 64 KiB guards; the call runs with the
buffers pre-filled with 0x00, with the leftovers of a call on other inputs and with 0xFF, and on a non-default stream.  All
guards and inputs must hold their bytes and every run must give the bits of the unguarded call (the outputs are fully
written, nothing is accumulated into, one summation order)."""
import numpy as np
import pytest
import torch

import bert_oracle as bo
import guarded
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
B, T, L = 3, 9, 1


@pytest.fixture(scope="module")
def dev():
    pytest.importorskip("transformers")
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def case():
    """MiniLM-shaped, one layer: (flat parameter tensors on the CPU, rebuild, ids, other ids, float64 states, e_ref)."""
    pytest.importorskip("transformers")
    m32, m64 = bo.make_model(bo.config(L=L, vocab=64, max_pos=16, **bo.MINILM), seed=21)
    rs = np.random.RandomState(22)
    ids, other = rs.randint(0, 64, (B, T)), rs.randint(0, 64, (B, T))
    want = bo.states(m64, ids)
    return m32, ids, other, want, bo.rel_err(bo.states(m32, ids), want)


def _args(dev, model, wrap=None):
    """The tensors of one ops.bert_encode call on the device, each through ``wrap`` (a guarded copy) when given."""
    P = bo.layer_params(model)
    w = (lambda t, role: t) if wrap is None else wrap
    top = {k: w(P[k].detach().to(dev), k) for k in ("word_emb", "pos_emb", "type_emb", "ln_g", "ln_b")}
    layers = [{k: w(v.detach().to(dev), "layers[%d].%s" % (i, k)) for k, v in d.items()} for i, d in enumerate(P["layers"])]
    return top, layers, P


def _call(top, layers, P, ids):
    from gnnrag_amd import ops
    return ops.bert_encode(ids, top["word_emb"], top["pos_emb"], top["type_emb"], top["ln_g"], top["ln_b"], P["eps"], layers,
                           P["heads"], I=P["I"])


def test_encode_guarded_fills_and_stream(dev, monkeypatch, case):
    from gnnrag_amd import _lib, ops
    m32, ids, other, want, e_ref = case
    top, layers, P = _args(dev, m32)
    ids_d, other_d = torch.from_numpy(ids).long().to(dev), torch.from_numpy(other).long().to(dev)
    plain = _call(top, layers, P, ids_d).cpu()
    err = bo.rel_err(plain.numpy(), want)
    print("guarded case: err %.3g, e_ref %.3g" % (err, e_ref))
    assert err <= bo.bound(e_ref)

    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    assert ops._buf == g.buf
    gtop, glayers, _ = _args(dev, m32, g.wrap)
    runs = []
    for fill, inp in ((FILL_ZERO, ids_d), (FILL_ZERO, other_d), (FILL_LEFTOVERS, ids_d), (FILL_ONES, ids_d)):
        g.fill = fill
        gi = g.wrap(inp, "ids")
        hits = g.leftover_hits
        out = _call(gtop, glayers, P, gi).cpu()
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits > hits
        g.check("body fill %r%s" % (fill, "" if inp is ids_d else " (other inputs)"))
        if inp is ids_d:
            runs.append(out)
    assert set(g.sizes) == {"bert_encode: out", "bert_encode: workspace"}
    assert g.sizes["bert_encode: out"] == B * T * 384 * 4
    assert g.sizes["bert_encode: workspace"] == _lib.load().gnnrag_bert_workspace_bytes(B, T, 384, 1536)
    for out in runs:
        assert torch.equal(out, plain)
    # a non-default stream
    g.fill = FILL_ONES
    side = torch.cuda.Stream(device=dev)
    gi = g.wrap(ids_d, "ids")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = _call(gtop, glayers, P, gi)
    side.synchronize()
    g.check("side stream")
    assert torch.equal(out.cpu(), plain)
    g.release()


def test_out_of_range_ids_poison_their_question_only(dev, monkeypatch, case):
    """Ids -1 and vocab in one question (a wrong kernel would read the guard right in front of and right behind the
    embedding table): that question's rows are NaN, the other questions' rows keep their bits, all guards intact."""
    m32, ids, _, _, _ = case
    top, layers, P = _args(dev, m32)
    plain = _call(top, layers, P, torch.from_numpy(ids).long().to(dev)).cpu()
    bad = ids.copy()
    bad[1, 2], bad[1, 7] = -1, 64
    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    gtop, glayers, _ = _args(dev, m32, g.wrap)
    for n_layers in (0, L):
        out = _call(gtop, glayers[:n_layers], P, g.wrap(torch.from_numpy(bad).long().to(dev), "ids")).cpu()
        g.check("out-of-range ids, L=%d" % n_layers)
        if n_layers == 0:
            nan_rows = torch.isnan(out).all(-1)
            assert nan_rows[1, 2] and nan_rows[1, 7] and int(nan_rows.sum()) == 2      # the two rows, whole
            assert not torch.isnan(out[[0, 2]]).any()
        else:
            assert torch.isnan(out[1]).all()                                           # every row attends the two
            assert torch.equal(out[0], plain[0]) and torch.equal(out[2], plain[2])
    g.release()


@pytest.mark.parametrize("Bq,Tq,heads,dh", [(3, 9, 2, 32), (1, 65, 3, 64)])
def test_attention_guarded(dev, monkeypatch, Bq, Tq, heads, dh):
    from gnnrag_amd import ops
    qkv = torch.from_numpy(np.random.RandomState(3).standard_normal((Bq * Tq, 3 * heads * dh)).astype(np.float32)).to(dev)
    plain = ops.bert_attention(qkv, Bq, Tq, heads, dh).cpu()
    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    for fill in (FILL_ZERO, FILL_LEFTOVERS, FILL_ONES):
        g.fill = fill
        out = ops.bert_attention(g.wrap(qkv, "qkv"), Bq, Tq, heads, dh).cpu()
        g.check("attention, body fill %r" % (fill,))
        assert torch.equal(out, plain)
    assert g.sizes == {"bert_attention: ctx": Bq * Tq * heads * dh * 4}
    g.release()
