"""The new entry points of fine-tuning the whole LM question encoder in guarded buffers (tests/guarded.py): the embedding
forward that saves and its backward, the layers' saving forward and backward with MPNet's relative bias, the attention
backward with the bias and the bias-table reduce.  Every input - ids, keep bytes, reserves and the bias table included - and
every buffer the binding allocates (``ops._buf``: outputs, reserves, workspaces) is an exact-sized view between two 64 KiB
guards; the calls run with the allocated buffers pre-filled with 0x00, with the leftovers of a call on other inputs and with
0xFF, and on a non-default stream.  All guards and inputs must hold their bytes and every run must give the bits of the
unguarded call.  A reserve or workspace four bytes short is refused before anything is written."""
import numpy as np
import pytest
import torch

import bert_dropout_oracle as do
import guarded
import lm_variants_oracle as lo
from guarded import FILL_LEFTOVERS, FILL_ONES, FILL_ZERO

pytestmark = pytest.mark.gpu
B, T, L = 3, 9, 2
P_HIDDEN, P_ATT = 0.5, 0.3
SHAPE = lo.SMALL[32]


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
    ids = torch.from_numpy(lo.ids_with_pads(B, T, seed=seed)).to(dev)
    g = torch.from_numpy(rs.standard_normal((B, T, H)).astype(np.float32)).to(dev)
    kh, ka = do.pack(do.draw(seed + 1, L, B, T, H, SHAPE["heads"], P_HIDDEN, P_ATT), L)
    return ids, g, torch.from_numpy(kh).to(dev), torch.from_numpy(ka).to(dev)


def _run(ops, P, dev, ids, g, kh, ka, wrap):
    """The whole chain on MPNet's parameters; every tensor the library sees goes through ``wrap``."""
    heads, H = P["heads"], SHAPE["H"]
    top = {k: wrap(P[k].detach().to(dev), k) for k in ("word_emb", "pos_emb", "ln_g", "ln_b", "rel_bias")}
    lay = [{k: wrap(v.detach().to(dev), "layers[%d].%s" % (i, k)) for k, v in d.items()} for i, d in enumerate(P["layers"])]
    ids, kh, ka = wrap(ids, "ids"), wrap(kh, "keep_hidden"), wrap(ka, "keep_att")
    sh, sa = do.scale(P_HIDDEN), do.scale(P_ATT)
    x0, e_res = ops.bert_embed_forward_save(ids, top["word_emb"], top["pos_emb"], None, top["ln_g"], top["ln_b"], P["eps"],
                                            pad_id=P["pad_id"], keep=kh[0], scale=sh)
    kw = dict(keep_hidden=kh, scale_hidden=sh, keep_att=ka, scale_att=sa, rel_bias=top["rel_bias"])
    out, reserve = ops.bert_layers_forward_save(wrap(x0, "x0"), lay, heads, P["eps"], B, T, **kw)
    g_x0, grads, d_bias = ops.bert_layers_backward(wrap(g, "g_out"), lay, heads, P["eps"], B, T, wrap(reserve, "reserve"),
                                                   want_rel_bias_grad=True, **kw)
    eg = ops.bert_embed_backward(wrap(g_x0, "g_x0"), ids, wrap(e_res, "embed reserve"), top["ln_g"], P["eps"],
                                 int(top["word_emb"].shape[0]), int(top["pos_emb"].shape[0]), 0, word_pad=lo.PAD,
                                 pos_pad=lo.PAD, keep=kh[0], scale=sh)
    # layer 0's qkv block of the reserve (behind its xin block)
    qkv = wrap(reserve[B * T * H * 4: B * T * 4 * H * 4].view(torch.float32).view(B * T, 3 * H), "qkv")
    d_qkv, d_b1 = ops.bert_attention_backward(qkv, wrap(g.view(B * T, H), "d_ctx"), B, T, heads, H // heads, ka[0], sa,
                                              rel_bias=top["rel_bias"], want_bias_grad=True)
    return ([x0, e_res, out, g_x0, d_bias, d_qkv, d_b1] + [eg[k] for k in ("d_word", "d_pos", "d_ln_g", "d_ln_b")] +
            [grads[l][k] for l in range(L) for k in ops.BERT_GRAD_FIELDS])


def _params(dev):
    m32, _ = do.make_variant("mpnet", SHAPE, L, seed=71)
    return lo.layer_params(m32, T)


def test_whole_chain_guarded_fills_and_stream(dev, monkeypatch):
    from gnnrag_amd import _lib, ops
    P = _params(dev)
    one, other = _inputs(dev, 72), _inputs(dev, 74)
    plain = [t.cpu() for t in _run(ops, P, dev, *one, wrap=lambda t, role: t)]
    assert all(torch.isfinite(t).all() for t in plain if t.dtype == torch.float32)

    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    assert ops._buf == g.buf
    runs = []
    for fill, inp in ((FILL_ZERO, one), (FILL_ZERO, other), (FILL_LEFTOVERS, one), (FILL_ONES, one)):
        g.fill = fill
        hits = g.leftover_hits
        outs = [t.cpu() for t in _run(ops, P, dev, *inp, wrap=g.wrap)]
        if fill == FILL_LEFTOVERS:
            assert g.leftover_hits > hits
        g.check("body fill %r%s" % (fill, "" if inp is one else " (other inputs)"))
        if inp is one:
            runs.append(outs)
    lib, H, I, heads = _lib.load(), SHAPE["H"], SHAPE["I"], SHAPE["heads"]
    assert g.sizes["bert_embed_forward_save: reserve"] == lib.gnnrag_bert_embed_reserve_bytes(B, T, H) == B * T * (H + 1) * 4
    assert g.sizes["bert_embed_backward: workspace"] == lib.gnnrag_bert_embed_backward_workspace_bytes(B, T, H)
    assert g.sizes["bert_layers_forward_save: reserve"] == lib.gnnrag_bert_reserve_bytes(L, B, T, H, I)
    assert g.sizes["bert_layers_backward: workspace"] == lib.gnnrag_bert_layers_backward_workspace_bytes(B, T, H, heads, I)
    assert g.sizes["bert_attention_backward: workspace"] == lib.gnnrag_bert_attention_backward_workspace_bytes(B, T, heads)
    assert {"bert_embed_forward_save: out", "bert_embed_backward: d_word", "bert_embed_backward: d_pos",
            "bert_embed_backward: d_ln_g", "bert_layers_backward: d_rel_bias", "bert_rel_bias_reduce: d_bias",
            "bert_attention_backward: d_qkv"} <= set(g.sizes)
    assert "bert_embed_backward: d_type" not in g.sizes
    for outs in runs:
        assert all(torch.equal(a, b) for a, b in zip(outs, plain))
    # a non-default stream
    g.fill = FILL_ONES
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        outs = _run(ops, P, dev, *one, wrap=g.wrap)
    side.synchronize()
    g.check("side stream")
    assert all(torch.equal(a.cpu(), b) for a, b in zip(outs, plain))
    g.release()


def test_short_reserves_and_workspaces_are_refused(dev, monkeypatch):
    """A reserve or a workspace four bytes short is GNNRAG_E_WORKSPACE before anything is launched: no guard is touched."""
    from gnnrag_amd import _lib, ops
    P = _params(dev)
    heads, H = P["heads"], SHAPE["H"]
    ids, gr, kh, ka = _inputs(dev, 72)
    top = {k: P[k].detach().to(dev) for k in ("word_emb", "pos_emb", "ln_g", "ln_b", "rel_bias")}
    layers = [{k: v.detach().to(dev) for k, v in d.items()} for d in P["layers"]]
    emb = lambda: ops.bert_embed_forward_save(ids, top["word_emb"], top["pos_emb"], None, top["ln_g"], top["ln_b"],  # noqa: E731
                                              P["eps"], pad_id=P["pad_id"])
    x0, e_res = emb()
    ebw = lambda res=e_res: ops.bert_embed_backward(gr, ids, res, top["ln_g"], P["eps"], int(top["word_emb"].shape[0]),  # noqa: E731
                                                    int(top["pos_emb"].shape[0]), 0)
    save = lambda: ops.bert_layers_forward_save(x0, layers, heads, P["eps"], B, T, rel_bias=top["rel_bias"])  # noqa: E731
    _, reserve = save()
    back = lambda res=reserve: ops.bert_layers_backward(gr, layers, heads, P["eps"], B, T, res, rel_bias=top["rel_bias"],  # noqa: E731
                                                        want_rel_bias_grad=True)
    qkv = torch.randn(B * T, 3 * H, device=dev)
    att = lambda: ops.bert_attention_backward(qkv, gr.view(B * T, H), B, T, heads, H // heads, rel_bias=top["rel_bias"])  # noqa: E731
    g = guarded.Guard(dev)
    guarded.install(monkeypatch, g)
    for role, call in (("bert_embed_forward_save: reserve", emb), ("bert_embed_backward: workspace", ebw),
                       ("bert_layers_forward_save: reserve", save), ("bert_layers_forward_save: workspace", save),
                       ("bert_layers_backward: workspace", back), ("bert_attention_backward: workspace", att)):
        g.short = {role: 4}
        with pytest.raises(_lib.GnnragError) as e:
            call()
        assert e.value.code == -3, role
        g.check("short " + role)
    g.short = {}
    for call, res in ((ebw, e_res), (back, reserve)):
        with pytest.raises(_lib.GnnragError) as e:
            call(res[:-4])
        assert e.value.code == -3
        g.check("short reserve of a backward")
    g.release()
