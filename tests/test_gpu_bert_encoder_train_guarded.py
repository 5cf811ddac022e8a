"""gnnrag_bert_encode_train / gnnrag_bert_attention_drop in guarded buffers (tests/guarded.py): every input - the two keep
buffers included - and every buffer the binding allocates (``ops._buf``: out, workspace, ctx) is an exact-sized view between
two 64 KiB guards; the call runs with the allocated buffers pre-filled with 0x00, with the leftovers of a call on other
inputs and with 0xFF, and on a non-default stream.  All guards and inputs must hold their bytes and every run must give the
bits of the unguarded call (the outputs are fully written, nothing is accumulated into, one summation order)."""
import numpy as np
import pytest
import torch

import bert_dropout_oracle as do
import bert_oracle as bo
import guarded
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
B, T, L = 3, 9, 1
P_HIDDEN, P_ATT = 0.5, 0.3


@pytest.fixture(scope="module")
def dev():
    pytest.importorskip("transformers")
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def case():
    """MiniLM-shaped, one layer: (fp32 model, ids, other ids, packed masks, other masks, scales, float64 states, e_ref)."""
    pytest.importorskip("transformers")
    m32, m64 = do.make_bert(bo.MINILM, L, seed=21, max_pos=16)
    rs = np.random.RandomState(22)
    ids, other = rs.randint(0, 64, (B, T)), rs.randint(0, 64, (B, T))
    masks = do.draw(23, L, B, T, 384, 12, P_HIDDEN, P_ATT)
    scales = (do.scale(P_HIDDEN), do.scale(P_ATT))
    want = do.run(m64, ids, masks, *scales)
    e_ref = bo.rel_err(do.run(m32, ids, masks, *scales), want)
    return m32, ids, other, do.pack(masks, L), do.pack(do.draw(24, L, B, T, 384, 12, P_HIDDEN, P_ATT), L), scales, want, e_ref


def test_encode_train_guarded_fills_and_stream(dev, monkeypatch, case):
    from gnnrag_amd import _lib, ops
    m32, ids, other, (kh, ka), (kh2, ka2), (sh, sa), want, e_ref = case
    plain = do.encode_train(dev, m32, ids, kh, ka, sh, sa).cpu()
    err = bo.rel_err(plain.numpy(), want)
    print("guarded case: err %.3g, e_ref %.3g, ratio %.2f" % (err, e_ref, err / max(e_ref, 1e-30)))
    assert err <= bo.bound(e_ref)

    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    assert ops._buf == g.buf
    roles = []

    def wrap(t, role):
        roles.append(role)
        return g.wrap(t, role)

    runs = []
    for fill, inp in ((FILL_ZERO, (ids, kh, ka)), (FILL_ZERO, (other, kh2, ka2)), (FILL_LEFTOVERS, (ids, kh, ka)),
                      (FILL_ONES, (ids, kh, ka))):
        g.fill = fill
        hits = g.leftover_hits
        out = do.encode_train(dev, m32, *inp, sh, sa, wrap=wrap).cpu()
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits > hits
        g.check("body fill %r%s" % (fill, "" if inp[0] is ids else " (other inputs)"))
        if inp[0] is ids:
            runs.append(out)
    assert {"ids", "keep_hidden", "keep_att", "word_emb", "layers[0].W_qkv", "layers[0].ln2_b"} <= set(roles)
    assert set(g.sizes) == {"bert_encode_train: out", "bert_encode_train: workspace"}
    assert g.sizes["bert_encode_train: out"] == B * T * 384 * 4
    assert g.sizes["bert_encode_train: workspace"] == _lib.load().gnnrag_bert_workspace_bytes(B, T, 384, 1536)
    for out in runs:
        assert torch.equal(out, plain)
    # a non-default stream
    g.fill = FILL_ONES
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = do.encode_train(dev, m32, ids, kh, ka, sh, sa, wrap=wrap)
    side.synchronize()
    g.check("side stream")
    assert torch.equal(out.cpu(), plain)
    g.release()


def test_out_of_range_ids_poison_their_question_only(dev, monkeypatch, case):
    """Ids -1 and vocab in one question: that question's rows are NaN whatever its keep bytes are - also with every keep
    byte of the question 0 - the other questions' rows keep their bits, all guards intact."""
    m32, ids, _, (kh, ka), _, (sh, sa), _, _ = case
    plain = do.encode_train(dev, m32, ids, kh, ka, sh, sa).cpu()
    bad = ids.copy()
    bad[1, 2], bad[1, 7] = -1, 64
    kh0 = kh.copy()
    kh0.reshape(1 + 2 * L, B, T, -1)[:, 1] = 0
    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    for keep_hidden in (kh, kh0):
        for n_layers in (0, L):
            out = do.encode_train(dev, m32, bad, keep_hidden[:1 + 2 * n_layers], ka if n_layers else None, sh, sa, L=n_layers,
                                  wrap=g.wrap).cpu()
            g.check("out-of-range ids, L=%d" % n_layers)
            if n_layers == 0:
                nan_rows = torch.isnan(out).all(-1)
                assert nan_rows[1, 2] and nan_rows[1, 7] and int(nan_rows.sum()) == 2   # the two rows, whole
                assert not torch.isnan(out[[0, 2]]).any()
            else:
                # every row attends the two, and NaN * 0 is NaN (as in transformers): dropped elements stay NaN too
                assert torch.isnan(out[1]).all()
                assert torch.equal(out[0], plain[0]) and torch.equal(out[2], plain[2])
    g.release()


@pytest.mark.parametrize("Bq,Tq,heads,dh", [(3, 9, 2, 32), (1, 65, 3, 64)])
def test_attention_drop_guarded(dev, monkeypatch, Bq, Tq, heads, dh):
    from gnnrag_amd import ops
    rs = np.random.RandomState(3)
    qkv = torch.from_numpy(rs.standard_normal((Bq * Tq, 3 * heads * dh)).astype(np.float32)).to(dev)
    keep = torch.from_numpy((rs.random_sample((Bq, heads, Tq, Tq)) >= 0.3).astype(np.uint8)).to(dev)
    s = do.scale(0.3)
    plain = ops.bert_attention_drop(qkv, Bq, Tq, heads, dh, keep, s).cpu()
    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    for fill in (FILL_ZERO, FILL_LEFTOVERS, FILL_ONES):
        g.fill = fill
        out = ops.bert_attention_drop(g.wrap(qkv, "qkv"), Bq, Tq, heads, dh, g.wrap(keep, "keep"), s).cpu()
        g.check("attention_drop, body fill %r" % (fill,))
        assert torch.equal(out, plain)
    assert g.sizes == {"bert_attention_drop: ctx": Bq * Tq * heads * dh * 4}
    g.release()
