"""The new kernels of fine-tuning the whole LM question encoder, each alone on the MI355X: the embedding tables' scatter
(exact on integer-valued rows), the embedding forward that saves and its backward, the attention backward with MPNet's
relative bias and the bias-table reduce - against the numpy float64 statements of tests/bert_full_oracle.py.

Bound: ``bert_oracle.bound(e_ref) = max(4 e_ref, 1e-6)`` per tensor, errors relative to the tensor's largest float64 entry,
``e_ref`` the fp32 torch autograd statement of the same step.  Sums of integer-valued fp32 numbers are exact in any order: the
scatter and the reduce must then equal numpy's float64 sums bit for bit."""
import numpy as np
import pytest
import torch

import bert_dropout_oracle as do
import bert_full_oracle as fo
import bert_grad_oracle as go
import bert_oracle as bo
import guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _check(got, want64, ref32, what, worst=None):
    go.compare(got, {what: np.asarray(want64)}, {what: np.asarray(ref32)}, what, worst)


# -- k_bert_embed_scatter ------------------------------------------------------------------------------------------------

H_S, VOCAB, MAX_POS = 32, 50, 40


def _scatter_case(kind, M, rs):
    ids = {"equal": np.full(M, 7), "distinct": np.arange(M) % VOCAB}.get(kind)
    if ids is None:
        ids = rs.randint(0, VOCAB, M)
    pos = (np.arange(M) * 7) % MAX_POS if kind != "equal" else np.full(M, 3)
    if kind == "pads":
        ids[::3], pos[::3] = 1, 1
    if kind == "outside":
        ids[0] = -1
        ids[M // 2] = VOCAB
        pos[M - 1] = -1
        if M > 3:
            pos[1] = MAX_POS
    return ids.astype(np.int64), pos.astype(np.int32)


@pytest.mark.parametrize("M", [1, 5, 64, 65, 300])
@pytest.mark.parametrize("kind,word_pad,pos_pad", [("equal", None, None), ("distinct", None, None), ("random", None, None),
                                                   ("pads", 1, 1), ("pads", None, None), ("pads", 1, None),
                                                   ("outside", None, None), ("outside", 1, 1)])
def test_scatter_is_exact_on_integer_rows(dev, monkeypatch, M, kind, word_pad, pos_pad):
    from gnnrag_amd import ops
    rs = np.random.RandomState(M + len(kind))
    ids, pos = _scatter_case(kind, M, rs)
    dz = rs.randint(-8, 9, (M, H_S)).astype(np.float32)
    g = guarded.install(monkeypatch, guarded.Guard(dev, fill=guarded.FILL_ONES))
    d_word, d_pos = ops.bert_embed_scatter(g.wrap(_t(dz, dev), "dz"), g.wrap(_t(ids, dev, np.int64), "ids"),
                                           g.wrap(_t(pos, dev, np.int32), "pos"), VOCAB, MAX_POS, word_pad, pos_pad)
    g.check("scatter %s M=%d" % (kind, M))                             # nothing outside the tables, no input touched
    # a token names its rows only when BOTH its id and its position lie inside their tables
    ok = (ids >= 0) & (ids < VOCAB) & (pos >= 0) & (pos < MAX_POS)
    for got, keys, rows, pad in ((d_word, ids, VOCAB, word_pad), (d_pos, pos, MAX_POS, pos_pad)):
        got = got.cpu().numpy()
        keys = np.where(ok, keys, -1)
        want = fo.scatter64(dz, keys, rows, pad)
        assert np.array_equal(_bits(got), _bits(want)), (kind, M)
        named = np.zeros(rows, dtype=bool)
        named[keys[(keys >= 0) & (keys != (-1 if pad is None else pad))]] = True
        assert not np.signbit(got[~named]).any() and np.all(got[~named] == 0)      # untouched rows: exactly +0
    g.release()


def test_scatter_second_call_and_other_width(dev):
    """H = 768: three column rounds of 64 float4s per table row; a second call gives the same bits."""
    from gnnrag_amd import ops
    rs = np.random.RandomState(9)
    M, H = 130, 768
    ids, pos = rs.randint(0, 11, M).astype(np.int64), rs.randint(0, 5, M).astype(np.int32)
    dz = rs.standard_normal((M, H)).astype(np.float32)
    a = ops.bert_embed_scatter(_t(dz, dev), _t(ids, dev, np.int64), _t(pos, dev, np.int32), 11, 5)
    b = ops.bert_embed_scatter(_t(dz, dev), _t(ids, dev, np.int64), _t(pos, dev, np.int32), 11, 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # ascending row order in fp32: the sequential fp32 sum, bit for bit
    want = np.zeros((11, H), dtype=np.float32)
    for q in range(M):
        want[ids[q]] += dz[q]
    assert np.array_equal(_bits(a[0].cpu().numpy()), _bits(want))


# -- the embedding stage -------------------------------------------------------------------------------------------------

def _embed32(g_x0, ids, pos, word, posw, typ, g, b, eps, keep, scale, word_pad, pos_pad):
    """fp32 torch autograd of the same statement: the yardstick e_ref."""
    F = torch.nn.functional
    tw, tp = (torch.from_numpy(a.astype(np.float32)).requires_grad_(True) for a in (word, posw))
    tt = None if typ is None else torch.from_numpy(typ.astype(np.float32)).requires_grad_(True)
    tg, tb = (torch.from_numpy(a.astype(np.float32)).requires_grad_(True) for a in (g, b))
    s = F.embedding(torch.from_numpy(ids), tw, padding_idx=word_pad) + F.embedding(torch.from_numpy(pos), tp,
                                                                                   padding_idx=pos_pad)
    if tt is not None:
        s = s + tt[0]
    y = F.layer_norm(s, (word.shape[1],), tg, tb, eps)
    if keep is not None:
        y = y * torch.from_numpy(keep).float().view(y.shape) * float(scale)
    y.backward(torch.from_numpy(g_x0.astype(np.float32)))
    return {"d_word": tw.grad.numpy(), "d_pos": tp.grad.numpy(), "d_type": None if tt is None else tt.grad.numpy(),
            "d_ln_g": tg.grad.numpy(), "d_ln_b": tb.grad.numpy()}


@pytest.mark.parametrize("B,T,H", [(3, 9, 64), (8, 9, 768)])
@pytest.mark.parametrize("form", ["bert", "roberta", "mpnet"])
@pytest.mark.parametrize("p", [None, 0.3])
def test_embed_forward_save_and_backward(dev, B, T, H, form, p):
    """BERT form: row positions and the type term; RoBERTa / MPNet form: positions from the ids, with and without type."""
    from gnnrag_amd import ops
    rs = np.random.RandomState(B * 100 + H)
    vocab, max_pos, eps = 50, 32, 1e-5
    pad_id = None if form == "bert" else 1
    word_pad, pos_pad = (0, None) if form == "bert" else (1, 1)
    ids = rs.randint(0, vocab, (B, T)).astype(np.int64)
    ids[0, 3:5], ids[B - 1, 1::2], ids[1, :] = 1, 1, ids[1, 0]          # pads and repeated tokens
    word, posw = rs.standard_normal((vocab, H)).astype(np.float32), rs.standard_normal((max_pos, H)).astype(np.float32)
    typ = None if form == "mpnet" else rs.standard_normal((2, H)).astype(np.float32)
    g, b = (1.0 + 0.1 * rs.standard_normal(H)).astype(np.float32), (0.1 * rs.standard_normal(H)).astype(np.float32)
    keep = None if p is None else (rs.random_sample((B * T, H)) >= p).astype(np.uint8)
    scale = 1.0 if p is None else do.scale(p)
    g_x0 = rs.standard_normal((B, T, H)).astype(np.float32)
    d = lambda a, dt=np.float32: None if a is None else _t(a, dev, dt)  # noqa: E731
    args = (d(ids, np.int64), d(word), d(posw), d(typ), d(g), d(b), eps)
    x0, reserve = ops.bert_embed_forward_save(*args, pad_id=pad_id, keep=d(keep, np.uint8), scale=scale)
    # the bits of the embedding stage of bert_encode_train
    want_x0 = ops.bert_encode_train(*args, [], H // 64, pad_id=pad_id, scale_hidden=scale,
                                    keep_hidden=None if keep is None else d(keep[None], np.uint8))
    assert torch.equal(x0, want_x0)
    pos = fo.positions(ids, pad_id, vocab, max_pos)
    assert reserve.numel() == B * T * (H + 1) * 4
    assert np.array_equal(reserve[B * T * H * 4:].view(torch.int32).cpu().numpy(), pos.reshape(-1))
    sum0 = reserve[: B * T * H * 4].view(torch.float32).view(B * T, H).cpu().numpy()
    want_sum = (word[ids.reshape(-1)] + (0 if typ is None else typ[0])) + posw[pos.reshape(-1)]
    assert np.array_equal(_bits(sum0), _bits(want_sum))

    got = ops.bert_embed_backward(d(g_x0), args[0], reserve, args[4], eps, vocab, max_pos, 0 if typ is None else 2,
                                  word_pad=word_pad, pos_pad=pos_pad, keep=d(keep, np.uint8), scale=scale)
    want = fo.embed_bwd64(g_x0, ids, word, posw, typ, g, eps, pad_id, keep, scale, word_pad, pos_pad)
    ref = _embed32(g_x0, ids, pos, word, posw, typ, g, b, eps, keep, scale, word_pad, pos_pad)
    worst = [0.0]
    for name in ops.BERT_EMBED_GRADS:
        if want[name] is None:
            assert got[name] is None
            continue
        _check(got[name].cpu().numpy(), want[name], ref[name], "%s %s (%d,%d,%d) p=%s" % (name, form, B, T, H, p), worst)
    print("embedding backward %s (%d,%d,%d) p=%s: largest err / e_ref %.2f" % (form, B, T, H, p, worst[0]))
    dw, dp = got["d_word"].cpu().numpy(), got["d_pos"].cpu().numpy()
    assert np.all(dw[word_pad] == 0) and not np.signbit(dw[word_pad]).any()
    unnamed = np.setdiff1d(np.arange(vocab), ids.reshape(-1))
    assert np.all(dw[unnamed] == 0) and not np.signbit(dw[unnamed]).any()
    if pos_pad is not None:
        assert np.all(dp[pos_pad] == 0) and not np.signbit(dp[pos_pad]).any()
    if typ is not None:
        assert np.all(got["d_type"][1].cpu().numpy() == 0) and not np.signbit(got["d_type"][1].cpu().numpy()).any()
    # a second call gives the same bits; an unwanted gradient is None and leaves the others alone
    again = ops.bert_embed_backward(d(g_x0), args[0], reserve, args[4], eps, vocab, max_pos, 0 if typ is None else 2,
                                    word_pad=word_pad, pos_pad=pos_pad, keep=d(keep, np.uint8), scale=scale,
                                    need={"d_word": True, "d_ln_b": True})
    assert torch.equal(again["d_word"], got["d_word"]) and torch.equal(again["d_ln_b"], got["d_ln_b"])
    assert again["d_pos"] is None and again["d_type"] is None and again["d_ln_g"] is None


def test_embed_rows_outside_their_tables(dev):
    """An id -1, an id = vocab and a position past the table: the forward's rows are NaN, pos is -1 and the backward adds
    them to no table (the other tokens' table rows are those of the batch without them)."""
    from gnnrag_amd import ops
    rs = np.random.RandomState(4)
    B, T, H, vocab, max_pos, eps = 2, 6, 32, 20, 8, 1e-5
    ids = rs.randint(2, vocab, (B, T)).astype(np.int64)
    ids[0, 1], ids[1, 4] = -1, vocab
    word, posw = rs.standard_normal((vocab, H)).astype(np.float32), rs.standard_normal((max_pos, H)).astype(np.float32)
    g, b = np.ones(H, dtype=np.float32), np.zeros(H, dtype=np.float32)
    x0, reserve = ops.bert_embed_forward_save(_t(ids, dev, np.int64), _t(word, dev), _t(posw, dev), None, _t(g, dev),
                                              _t(b, dev), eps)
    pos = reserve[B * T * H * 4:].view(torch.int32).cpu().numpy().reshape(B, T)
    bad = (ids < 0) | (ids >= vocab)
    assert np.array_equal(pos, np.where(bad, -1, np.tile(np.arange(T), (B, 1))))
    assert torch.isnan(x0.cpu()[torch.from_numpy(bad)]).all() and torch.isfinite(x0.cpu()[torch.from_numpy(~bad)]).all()
    g_x0 = rs.standard_normal((B, T, H)).astype(np.float32)
    got = ops.bert_embed_backward(_t(g_x0, dev), _t(ids, dev, np.int64), reserve, _t(g, dev), eps, vocab, max_pos)
    dw, dp = got["d_word"].cpu().numpy(), got["d_pos"].cpu().numpy()
    good = ~bad.reshape(-1)
    sum0 = word[np.where(bad, 0, ids).reshape(-1)] + posw[np.tile(np.arange(T), B)]
    dz, _, _, _ = go.ln_bwd64(g_x0.reshape(-1, H)[good], sum0[good], g, eps)
    ids_good, pos_good = ids.reshape(-1)[good], np.tile(np.arange(T), B)[good]
    ref = _embed32(g_x0.reshape(-1, H)[good], ids_good, pos_good, word, posw, None, g, b, eps, None, 1.0, None, None)
    assert np.isfinite(dw).all() and np.isfinite(dp).all()
    _check(dw, fo.scatter64(dz, ids_good, vocab), ref["d_word"], "d_word beside rows outside the tables")
    _check(dp, fo.scatter64(dz, pos_good, max_pos), ref["d_pos"], "d_pos beside rows outside the tables")


# -- k_bert_attention_bwd_bias, k_bert_rel_bias_reduce -------------------------------------------------------------------

def _attention_bias32(qkv, d_ctx, B, T, heads, dh, bias, keep, scale):
    x = torch.from_numpy(np.asarray(qkv, dtype=np.float32)).requires_grad_(True)
    tb = torch.from_numpy(np.asarray(bias, dtype=np.float32)).requires_grad_(True)
    v = x.view(B, T, 3, heads, dh)
    q, k, val = (v[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / float(np.sqrt(dh)) + tb[:, j - i + T - 1][None], dim=-1)
    if keep is not None:
        p = p * torch.from_numpy(keep).float() * float(scale)
    torch.matmul(p, val).permute(0, 2, 1, 3).reshape(B * T, heads * dh).backward(
        torch.from_numpy(np.asarray(d_ctx, dtype=np.float32)))
    return x.grad.numpy(), tb.grad.numpy()


def _att_inputs(B, T, heads, dh, p, seed):
    rs = np.random.RandomState(seed)
    H = heads * dh
    qkv = rs.standard_normal((B * T, 3 * H)).astype(np.float32)
    d_ctx = rs.standard_normal((B * T, H)).astype(np.float32)
    bias = rs.standard_normal((heads, 2 * T - 1)).astype(np.float32)
    keep, scale = None, 1.0
    if p is not None:
        keep, scale = (rs.random_sample((B, heads, T, T)) >= p).astype(np.uint8), do.scale(p)
    return qkv, d_ctx, bias, keep, scale


@pytest.mark.parametrize("T", [2, 5, 65, 128])
@pytest.mark.parametrize("B,heads,dh", [(1, 1, 32), (3, 3, 32), (1, 3, 64), (3, 1, 64)])
@pytest.mark.parametrize("p", [None, 0.3])
def test_attention_backward_bias(dev, T, B, heads, dh, p):
    from gnnrag_amd import ops
    H = heads * dh
    qkv, d_ctx, bias, keep, scale = _att_inputs(B, T, heads, dh, p, 200 + T)
    kd = None if keep is None else _t(keep, dev, np.uint8)
    d_qkv, d_bias = ops.bert_attention_backward(_t(qkv, dev), _t(d_ctx, dev), B, T, heads, dh, kd, scale,
                                                rel_bias=_t(bias, dev), want_bias_grad=True)
    want, want_b, _ = fo.attention_bias_bwd64(qkv, d_ctx, B, T, heads, dh, bias, keep, scale)
    ref, ref_b = _attention_bias32(qkv, d_ctx, B, T, heads, dh, bias, keep, scale)
    got = d_qkv.cpu().numpy()
    tag = "(%d,%d,%d,%d) p=%s" % (B, T, heads, dh, p)
    worst = [0.0]
    for name, lo_, hi in (("dQ", 0, H), ("dK", H, 2 * H), ("dV", 2 * H, 3 * H)):
        _check(got[:, lo_:hi], want[:, lo_:hi], ref[:, lo_:hi], name + " " + tag, worst)
    _check(d_bias.cpu().numpy(), want_b, ref_b, "d_bias " + tag, worst)
    print("attention backward with bias %s: largest err / e_ref %.2f" % (tag, worst[0]))
    # a zero table: the bits of the kernel without a bias
    zero = torch.zeros((heads, 2 * T - 1), device=dev)
    plain = ops.bert_attention_backward(_t(qkv, dev), _t(d_ctx, dev), B, T, heads, dh, kd, scale)
    assert torch.equal(ops.bert_attention_backward(_t(qkv, dev), _t(d_ctx, dev), B, T, heads, dh, kd, scale, rel_bias=zero),
                       plain)
    # a second call gives the same bits
    d_qkv2, d_bias2 = ops.bert_attention_backward(_t(qkv, dev), _t(d_ctx, dev), B, T, heads, dh, kd, scale,
                                                  rel_bias=_t(bias, dev), want_bias_grad=True)
    assert torch.equal(d_qkv, d_qkv2) and torch.equal(d_bias, d_bias2)
    # batch independence: the last question alone gives its own d_qkv rows
    if B > 1:
        k1 = None if keep is None else _t(keep[B - 1:], dev, np.uint8)
        one = ops.bert_attention_backward(_t(qkv[(B - 1) * T:], dev), _t(d_ctx[(B - 1) * T:], dev), 1, T, heads, dh, k1,
                                          scale, rel_bias=_t(bias, dev))
        assert torch.equal(one, d_qkv[(B - 1) * T:])


@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("p", [None, 0.3])
def test_attention_backward_bias_one_token(dev, dh, p):
    """T = 1: the softmax of one key is 1 whatever the bias, dS is exactly 0 and so is the table's gradient."""
    from gnnrag_amd import ops
    B, T, heads = 3, 1, 2
    qkv, d_ctx, bias, keep, scale = _att_inputs(B, T, heads, dh, p, 7)
    if keep is not None:
        keep[:] = 1                                                     # a dropped single key is covered by the parent's tests
    d_qkv, d_bias = ops.bert_attention_backward(_t(qkv, dev), _t(d_ctx, dev), B, T, heads, dh,
                                                None if keep is None else _t(keep, dev, np.uint8), scale,
                                                rel_bias=_t(bias, dev), want_bias_grad=True)
    assert tuple(d_bias.shape) == (heads, 1) and np.all(d_bias.cpu().numpy() == 0)
    got = d_qkv.cpu().numpy().reshape(B, 3, heads * dh)
    assert np.all(got[:, :2] == 0)
    assert bo.rel_err(got[:, 2], d_ctx * scale) <= 1e-6


@pytest.mark.parametrize("T", [1, 2, 5, 65, 128])
@pytest.mark.parametrize("B", [1, 3])
def test_rel_bias_reduce_is_exact_on_integer_squares(dev, T, B):
    from gnnrag_amd import ops
    heads = 3
    rs = np.random.RandomState(T * 10 + B)
    sq = rs.randint(-8, 9, (B * heads, 2, T, T)).astype(np.float32)      # the second square of a pair is not read
    got = ops.bert_rel_bias_reduce(_t(sq, dev), B, T, heads)
    want = fo.rel_bias_reduce64(sq[:, 0], B, T, heads)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    assert torch.equal(ops.bert_rel_bias_reduce(_t(sq, dev), B, T, heads), got)
