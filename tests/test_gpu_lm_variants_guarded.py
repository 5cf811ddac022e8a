"""gnnrag_bert_encode_ex / gnnrag_bert_attention_bias in guarded buffers (tests/guarded.py), as
tests/test_gpu_bert_encoder_guarded.py does for the BERT path: the ids, every table, ``rel_bias``, the workspace and the
output are exact-sized views between two 64 KiB guards; the call runs with the buffers pre-filled with 0x00, with the
leftovers of a call on other inputs and with 0xFF.  All guards and inputs must hold their bytes and every run must give the
bits of the unguarded call.  ``max_pos = T + pad + 1``: the full row reads the last row of the position table, whose back
guard (NaN) starts right behind it; the ids' guards are zero bytes, so a position count that read a neighbouring question
or past the row would count tokens that are not there."""
import numpy as np
import pytest
import torch

import bert_oracle as bo
import guarded
import lm_variants_oracle as lo
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
SHAPES = [(2, 1, 32), (2, 65, 32), (1, 128, 64)]                # (B, T, head width)


@pytest.fixture(scope="module")
def dev():
    pytest.importorskip("transformers")
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@pytest.mark.parametrize("B,T,dh", SHAPES, ids=["T1", "T65", "T128"])
@pytest.mark.parametrize("arch", lo.ARCHS)
def test_encode_guarded_fills(dev, monkeypatch, arch, B, T, dh):
    from gnnrag_amd import _lib, ops
    shape = lo.SMALL[dh]
    m32, m64 = lo.make_model(arch, lo.config(arch, L=1, max_pos=T + lo.PAD + 1, **shape), seed=41)
    ids, other = lo.ids_with_pads(B, T, seed=1), lo.ids_with_pads(B, T, seed=2)[::-1].copy()
    want = lo.states(m64, ids)
    e_ref = bo.rel_err(lo.states(m32, ids), want)
    plain = lo.encode(dev, m32, ids).cpu()
    err = bo.rel_err(plain.numpy(), want)
    print("%s guarded case B=%d T=%d: err %.3g, e_ref %.3g" % (arch, B, T, err, e_ref))
    assert err <= bo.bound(e_ref)

    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    assert ops._buf == g.buf
    runs = []
    for fill, inp in ((FILL_ZERO, ids), (FILL_ZERO, other), (FILL_LEFTOVERS, ids), (FILL_ONES, ids)):
        g.fill = fill
        hits = g.leftover_hits
        out = lo.encode(dev, m32, inp, wrap=g.wrap).cpu()
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits > hits
        g.check("%s, body fill %r%s" % (arch, fill, "" if inp is ids else " (other inputs)"))
        if inp is ids:
            runs.append(out)
    roles = {b.role for b in g.blocks}
    assert {"ids", "word_emb", "pos_emb", "ln_g", "layers[0].W_qkv"} <= roles
    assert ("rel_bias" in roles) == (arch == "mpnet") and ("type_emb" in roles) == (arch == "roberta")
    assert set(g.sizes) == {"bert_encode: out", "bert_encode: workspace"}
    assert g.sizes["bert_encode: out"] == B * T * shape["H"] * 4
    assert g.sizes["bert_encode: workspace"] == _lib.load().gnnrag_bert_workspace_bytes(B, T, shape["H"], shape["I"])
    for out in runs:
        assert torch.equal(out, plain)
    g.release()


@pytest.mark.parametrize("B,T,heads,dh", [(2, 1, 2, 32), (1, 65, 3, 64), (1, 128, 2, 64)], ids=["T1", "T65", "T128"])
def test_biased_attention_guarded(dev, monkeypatch, B, T, heads, dh):
    """The table's row of the LAST head ends where the back guard starts, the first head's row starts behind the front
    guard: entry 0 (j - i = -(T-1)) and entry 2T-2 are both read."""
    from gnnrag_amd import ops
    rs = np.random.RandomState(5)
    qkv = torch.from_numpy(rs.standard_normal((B * T, 3 * heads * dh)).astype(np.float32)).to(dev)
    bias = torch.from_numpy(rs.standard_normal((heads, 2 * T - 1)).astype(np.float32)).to(dev)
    plain = ops.bert_attention(qkv, B, T, heads, dh, rel_bias=bias).cpu()
    assert not torch.isnan(plain).any()
    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    for fill in (FILL_ZERO, FILL_LEFTOVERS, FILL_ONES):
        g.fill = fill
        out = ops.bert_attention(g.wrap(qkv, "qkv"), B, T, heads, dh, rel_bias=g.wrap(bias, "rel_bias")).cpu()
        g.check("biased attention, body fill %r" % (fill,))
        assert torch.equal(out, plain)
    assert g.sizes == {"bert_attention: ctx": B * T * heads * dh * 4}
    g.release()
