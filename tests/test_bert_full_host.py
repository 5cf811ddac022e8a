"""Host side of fine-tuning the whole LM question encoder (CPU, no GPU): the numpy float64 statements of
tests/bert_full_oracle.py against torch float64 autograd, the sizes and the argument rules of the new entry points, and the
switch ``GNNRAG_HIP_LM_FINETUNE_FULL`` on CPU stand-ins of the three classes."""
import copy

import numpy as np
import pytest
import torch

import bert_full_oracle as fo
import bert_oracle as bo
import lm_variants_oracle as lo

SMALL = dict(H=64, heads=2, I=128)


@pytest.fixture(scope="module")
def lib():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    return _lib.load()


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


# -- the numpy statements ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad_id,typed,drop", [(None, True, False), (None, True, True), (1, True, True), (1, False, False)])
def test_embedding_statement_against_autograd(pad_id, typed, drop):
    B, T, H, vocab, max_pos, eps = 3, 6, 16, 12, 10, 1e-5
    rs = np.random.RandomState(3)
    ids = rs.randint(0, vocab, (B, T))
    ids[0, 2:4] = 1
    ids[1, :] = ids[1, 0]
    word, posw, typ = rs.standard_normal((vocab, H)), rs.standard_normal((max_pos, H)), rs.standard_normal((2, H))
    g, b = 1.0 + 0.1 * rs.standard_normal(H), 0.1 * rs.standard_normal(H)
    keep = (rs.random_sample((B * T, H)) >= 0.3).astype(np.uint8) if drop else None
    scale = 1.0 / 0.7 if drop else 1.0
    g_x0 = rs.standard_normal((B, T, H))
    tw, tp, tt = (torch.from_numpy(a).requires_grad_(True) for a in (word, posw, typ))
    tg, tb = torch.from_numpy(g).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    pos = torch.from_numpy(fo.positions(ids, pad_id, vocab, max_pos))
    F = torch.nn.functional
    s = F.embedding(torch.from_numpy(ids), tw, padding_idx=1) + F.embedding(pos, tp, padding_idx=pad_id)
    if typed:
        s = s + tt[0]
    y = F.layer_norm(s, (H,), tg, tb, eps)
    if drop:
        y = y * torch.from_numpy(keep).double().view(B, T, H) * scale
    y.backward(torch.from_numpy(g_x0))
    got = fo.embed_bwd64(g_x0, ids, word, posw, typ if typed else None, g, eps, pad_id, keep, scale, word_pad=1,
                         pos_pad=pad_id)
    assert _rel(got["d_word"], tw.grad.numpy()) <= 1e-12 and _rel(got["d_pos"], tp.grad.numpy()) <= 1e-12
    assert _rel(got["d_ln_g"], tg.grad.numpy()) <= 1e-12 and _rel(got["d_ln_b"], tb.grad.numpy()) <= 1e-12
    assert np.all(got["d_word"][1] == 0)
    if typed:
        assert _rel(got["d_type"], tt.grad.numpy()) <= 1e-12 and np.all(got["d_type"][1] == 0)


@pytest.mark.parametrize("drop", [False, True])
def test_attention_bias_statement_against_autograd(drop):
    B, T, heads, dh = 2, 7, 2, 32
    rs = np.random.RandomState(1)
    qkv = rs.standard_normal((B * T, 3 * heads * dh))
    d_ctx = rs.standard_normal((B * T, heads * dh))
    bias = rs.standard_normal((heads, 2 * T - 1))
    keep = (rs.random_sample((B, heads, T, T)) >= 0.3).astype(np.uint8) if drop else None
    scale = 1.0 / 0.7 if drop else 1.0
    x, tb = torch.from_numpy(qkv).requires_grad_(True), torch.from_numpy(bias).requires_grad_(True)
    v = x.view(B, T, 3, heads, dh)
    q, k, val = (v[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / float(np.sqrt(dh)) + tb[:, j - i + T - 1][None], dim=-1)
    if drop:
        p = p * torch.from_numpy(keep).double() * scale
    torch.matmul(p, val).permute(0, 2, 1, 3).reshape(B * T, heads * dh).backward(torch.from_numpy(d_ctx))
    d_qkv, d_bias, ds = fo.attention_bias_bwd64(qkv, d_ctx, B, T, heads, dh, bias, keep, scale)
    assert _rel(d_qkv, x.grad.numpy()) <= 1e-12 and _rel(d_bias, tb.grad.numpy()) <= 1e-12
    assert np.abs(ds.sum(-1)).max() <= 1e-12 * np.abs(ds).max()          # the rows of dS still sum to zero


# -- sizes and argument rules --------------------------------------------------------------------------------------------

def _up(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("B,T,H", [(1, 1, 32), (3, 9, 64), (64, 20, 768), (64, 128, 384)])
def test_embed_sizes(lib, B, T, H):
    M = B * T
    assert lib.gnnrag_bert_embed_reserve_bytes(B, T, H) == M * (H + 1) * 4
    assert lib.gnnrag_bert_embed_backward_workspace_bytes(B, T, H) == 3 * _up(M * H * 4)


def test_sizes_of_refused_shapes_are_zero(lib):
    from gnnrag_amd import ops
    assert lib.gnnrag_bert_embed_reserve_bytes(0, 5, 64) == 0 and lib.gnnrag_bert_embed_reserve_bytes(2, 5, 62) == 0
    assert lib.gnnrag_bert_embed_backward_workspace_bytes(2, 0, 64) == 0
    assert lib.gnnrag_bert_embed_backward_workspace_bytes(2, 5, 62) == 0
    assert lib.gnnrag_bert_embed_backward_workspace_bytes(512, 128, 64) == 3 * _up(65536 * 64 * 4)      # the largest M
    assert lib.gnnrag_bert_embed_backward_workspace_bytes(513, 128, 64) == 0
    assert ops.BERT_EMBED_BWD_MAX_ROWS == 65536 >= 8192
    assert ops.bert_embed_backward_supported(65536, 64) and not ops.bert_embed_backward_supported(65537, 64)
    assert not ops.bert_embed_backward_supported(10, 62) and not ops.bert_embed_backward_supported(0, 64)


def test_argument_rules_before_any_launch(lib):
    """Sizes, then shapes whatever the pointers are, then NULL pointers and scales, then alignment, then the buffer sizes."""
    from gnnrag_amd import _lib
    OK, ODD = 0x10000, 0x10004
    big = 1 << 30
    fwd = lambda ids=OK, B=2, T=5, H=64, vocab=50, max_pos=16, pad=-1, keep=None, sc=1.0, out=OK, rb=big: \
        lib.gnnrag_bert_embed_forward_save(ids, OK, vocab, OK, max_pos, OK, pad, OK, OK, 1e-12, B, T, H, keep, sc, out, OK,
                                           rb, None)  # noqa: E731
    assert fwd(B=0) == -1 and fwd(vocab=0) == -1 and fwd(None, B=0) == -1
    assert fwd(None, H=62) == -2 and fwd(None, T=129, max_pos=200) == -2 and fwd(None, T=17) == -2
    assert fwd(None, T=15, pad=1) == -2 and fwd(T=14, pad=1, rb=16) == -3          # T + pad_id <= max_pos - 1
    assert fwd(None) == -1 and fwd(out=None) == -1 and fwd(keep=OK, sc=float("inf")) == -1 and fwd(keep=OK, sc=0.0) == -1
    assert fwd(ODD) == -2 and fwd(out=ODD) == -2 and fwd(keep=OK + 2, sc=2.0) == -2
    assert fwd(rb=2 * 5 * 65 * 4 - 4) == -3 and fwd(keep=ODD, sc=2.0, rb=16) == -3       # keep: 4-byte alignment is enough

    bwd = lambda g=OK, B=2, T=5, H=64, vocab=50, n_type=2, keep=None, sc=1.0, dw=OK, dt=OK, rb=big, wb=big: \
        lib.gnnrag_bert_embed_backward(g, OK, OK, rb, B, T, H, vocab, 16, n_type, -1, -1, keep, sc, OK, 1e-12, dw, OK, dt,
                                       OK, OK, OK, wb, None)  # noqa: E731
    assert bwd(B=0) == -1 and bwd(vocab=0) == -1 and bwd(n_type=0) == -1 and bwd(n_type=0, dt=None, rb=16) == -3
    assert bwd(None, H=62) == -2 and bwd(None, B=513, T=128) == -2
    assert bwd(None) == -1 and bwd(keep=OK, sc=-1.0) == -1
    assert bwd(ODD) == -2 and bwd(dw=ODD) == -2 and bwd(keep=OK + 1, sc=2.0) == -2
    assert bwd(rb=2 * 5 * 65 * 4 - 4) == -3 and bwd(wb=3 * _up(2 * 5 * 64 * 4) - 4) == -3 and bwd(dw=None, wb=16) == -3

    arr = (_lib.BertLayer * 1)()
    for n, _ in _lib.BertLayer._fields_:
        setattr(arr[0], n, OK)
    save = lambda x0=OK, L=1, T=5, H=64, I=128, rel=OK, rb=big, wb=big: \
        lib.gnnrag_bert_layers_forward_save_ex(x0, L, arr, rel, 1e-12, 2, T, H, 2, I, None, 1.0, None, 1.0, OK, OK, rb, OK,
                                               wb, 0, None)  # noqa: E731
    back = lambda g=OK, L=1, T=5, H=64, I=128, rel=OK, drel=OK, rb=big, wb=big: \
        lib.gnnrag_bert_layers_backward_ex(g, L, arr, rel, 1e-12, 2, T, H, 2, I, None, 1.0, None, 1.0, OK, rb, OK, None,
                                           drel, OK, wb, None)  # noqa: E731
    for call in (save, back):
        assert call(L=0) == -1 and call(None, T=129) == -2 and call(None, H=96) == -2 and call(None, I=126) == -2
        assert call(None) == -1 and call(ODD) == -2 and call(rel=ODD) == -2 and call(rb=16) == -3 and call(wb=16) == -3
    assert save(rel=None, rb=16) == -3 and back(rel=None, drel=None, rb=16) == -3   # no table: the entries without one
    assert back(rel=None) == -1 and back(drel=ODD) == -2                            # a gradient of a table that is not given
    ab = lambda rel=OK, dh=32, d_ctx=OK, wb=1 << 20: \
        lib.gnnrag_bert_attention_backward_bias(OK, d_ctx, 2, 5, 2, dh, rel, None, 1.0, OK, OK, wb, None)  # noqa: E731
    assert ab(dh=48) == -2 and ab(d_ctx=None) == -1 and ab(rel=ODD) == -2 and ab(wb=16) == -3 and ab(rel=None, wb=16) == -3
    red = lambda sq=OK, T=5, out=OK: lib.gnnrag_bert_rel_bias_reduce(sq, 2, T, 2, out, None)  # noqa: E731
    assert red(T=0) == -1 and red(None, T=129) == -2 and red(None) == -1 and red(out=None) == -1 and red(ODD) == -2


# -- the switch ----------------------------------------------------------------------------------------------------------

class _Holder:
    def __init__(self, enc):
        self.node_encoder = enc


def _patched(arch):
    from gnnrag_amd.modules.question_encoding import lm_encoder as le
    if arch == "bert":
        enc = copy.deepcopy(bo.make_model(bo.config(L=1, vocab=50, max_pos=16, **SMALL), seed=5)[0])
    else:
        enc = copy.deepcopy(lo.make_model(arch, lo.config(arch, L=1, **lo.SMALL[32]), seed=6)[0])
    le.patch_lm_encoder(_Holder(enc))
    return le, enc, enc._gnnrag_lm_patch


@pytest.mark.parametrize("arch", ["bert", "roberta", "mpnet"])
def test_full_switch_refusals(monkeypatch, arch):
    """The refusal texts with GNNRAG_HIP_LM_FINETUNE_FULL unset, "0", empty and "1": off is today's text for every class;
    on, MPNet follows the rules of the other two (on the parent it still refuses)."""
    pytest.importorskip("transformers")
    le, enc, p = _patched(arch)
    ids = torch.from_numpy(lo.ids_with_pads(2, 5)).long()
    enc.train()
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    monkeypatch.delenv("GNNRAG_HIP_LM_TRAIN", raising=False)
    monkeypatch.delenv("GNNRAG_HIP_LM_FINETUNE", raising=False)
    monkeypatch.delenv("GNNRAG_HIP_LM_FINETUNE_FULL", raising=False)
    today = ("a gradient is needed and the relative attention bias has no backward on the library" if arch == "mpnet"
             else "input_ids is not a CUDA tensor")
    assert not le.finetune_full_enabled() and p.refusal((ids,), {}) == "a gradient is needed"
    monkeypatch.setenv("GNNRAG_HIP_LM_FINETUNE_FULL", "1")              # alone it means nothing
    assert le.finetune_full_enabled() and p.refusal((ids,), {}) == "a gradient is needed"
    monkeypatch.setenv("GNNRAG_HIP_LM_FINETUNE", "1")
    monkeypatch.delenv("GNNRAG_HIP_LM_FINETUNE_FULL")
    assert p.refusal((ids,), {}) == today
    for off in ("0", ""):
        monkeypatch.setenv("GNNRAG_HIP_LM_FINETUNE_FULL", off)
        assert not le.finetune_full_enabled() and p.refusal((ids,), {}) == today
    monkeypatch.setenv("GNNRAG_HIP_LM_FINETUNE_FULL", "1")              # read at every call
    assert p.refusal((ids,), {}) == "input_ids is not a CUDA tensor"    # every rule before it holds, for MPNet as well
    with monkeypatch.context() as m:
        m.setattr(enc.config, "intermediate_size", 126)
        assert p.refusal((ids,), {}) == "a shape the backward kernels do not take"
    with monkeypatch.context() as m:
        m.setattr(le.ops, "BERT_EMBED_BWD_MAX_ROWS", 9)
        assert p.refusal((ids,), {}) == "more rows than the embedding backward takes"
        m.setattr(enc.config, "intermediate_size", 126)                 # the order: the layers' shape rule comes first
        assert p.refusal((ids,), {}) == "a shape the backward kernels do not take"
        m.setenv("GNNRAG_HIP_LM_FINETUNE_FULL", "0")
        m.setattr(enc.config, "intermediate_size", 128)
        assert p.refusal((ids,), {}) == today                           # the row rule belongs to the new switch
    with monkeypatch.context() as m:
        m.setattr(enc.config, "hidden_dropout_prob", 1.0)
        assert p.refusal((ids,), {}) == "a dropout probability of 1"
    # nothing requires grad: the frozen rules, whatever the new switch says
    for q in enc.parameters():
        q.requires_grad_(False)
    assert p.refusal((ids,), {}) == "dropout is active"
    # a refused call is transformers' own forward and the counters stand still
    for q in enc.parameters():
        q.requires_grad_(True)
    out = enc(ids)[0]
    assert out.requires_grad and p.hip_calls == 0 and p.hip_finetune_calls == 0 and p.hip_finetune_full_calls == 0
