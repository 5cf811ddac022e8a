"""The frozen RoBERTa / MPNet question encoders on the MI355X against transformers' own RobertaModel / MPNetModel in float64
(tests/lm_variants_oracle.py; the oracle runs on the CPU): positions counted from the ids, no token-type term, MPNet's
relative attention bias.

Bound of every LM-state comparison: ``bert_oracle.bound(e_ref)`` - the error relative to the oracle's largest entry is at most
max(4 x e_ref, 1e-6), where e_ref is the fp32 transformers module's own error against its float64 copy on the same input,
computed here on the CPU (or recorded by the reference's run in the fixture).  Every figure is printed before it is
asserted."""
import os

import numpy as np
import pytest
import torch

import bert_oracle as bo
import lm_variants_oracle as lo

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "lm_variants_ref.npz")
MATH_FP32, MATH_BF16X3 = 0, 1
TOL_INS = 2e-5                                  # tests/test_gpu_bert_encoder.py: the same arrays
PAD = lo.PAD


@pytest.fixture(scope="module")
def dev():
    pytest.importorskip("transformers")
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


_cases = {}


def _case(arch, dh, L, B, T, seed=31):
    """(fp32 model, float64 model, ids, float64 states, e_ref) - computed once per case on the CPU and shared.
    ``max_pos = T + pad + 1``: a full row reads the last row of the position table and nothing lies beyond it."""
    key = (arch, dh, L, B, T, seed)
    if key not in _cases:
        max_pos = T + (PAD + 1 if arch != "bert" else 0)
        m32, m64 = lo.make_model(arch, lo.config(arch, L=L, max_pos=max_pos, **lo.SMALL[dh]), seed)
        ids = lo.ids_with_pads(B, T, seed=seed)
        want = lo.states(m64, ids)
        _cases[key] = (m32, m64, ids, want, bo.rel_err(lo.states(m32, ids), want))
    return _cases[key]


# -- the embedding LayerNorm with positions from the ids ----------------------------------------------------------------

@pytest.mark.parametrize("arch", lo.ARCHS)                  # roberta: with the token-type row; mpnet: type_emb = None
@pytest.mark.parametrize("B,T,dh", [(1, 1, 32), (3, 9, 32), (6, 9, 64), (2, 65, 32), (1, 128, 64), (6, 128, 32)])
def test_embedding_against_float64(dev, arch, B, T, dh):
    """L = 0.  Rows of the random position table differ by O(0.1) per entry, so a position that is off by one lands
    orders of magnitude above the bound; row 0 is full, so the last row of ``pos_emb`` (max_pos - 1 = T + pad) is read."""
    m32, m64, ids, _, _ = _case(arch, dh, 1, B, T)
    with torch.no_grad():
        want = m64.embeddings(input_ids=torch.from_numpy(ids)).numpy()
        e_ref = bo.rel_err(m32.embeddings(input_ids=torch.from_numpy(ids)).numpy(), want)
        far = bo.rel_err(m64.embeddings(input_ids=torch.from_numpy(ids),
                                        position_ids=torch.from_numpy(lo.positions(ids, PAD) - 1)).numpy(), want)
    assert lo.positions(ids, PAD).max() == T + PAD == m32.config.max_position_embeddings - 1
    got = lo.encode(dev, m32, ids, L=0)
    err = bo.rel_err(got.cpu().numpy(), want)
    print("%s L=0 B=%d T=%d H=%d: err %.3g, e_ref %.3g, bound %.3g; positions off by one would give %.3g"
          % (arch, B, T, lo.SMALL[dh]["H"], err, e_ref, bo.bound(e_ref), far))
    assert got.shape == want.shape and far > 1e3 * bo.bound(e_ref)
    assert err <= bo.bound(e_ref)


def test_embedding_absolute_positions_without_token_types(dev):
    """``type_emb=None`` with ``pad_id=None``: positions 0 .. T-1 and no token-type term (the fourth form of the kernel)."""
    from gnnrag_amd import ops
    m32, m64, ids, _, _ = _case("bert", 32, 1, 3, 9)
    e32, e64 = m32.embeddings, m64.embeddings
    t = torch.from_numpy(ids)

    def ln_of(e):
        with torch.no_grad():
            return e.LayerNorm(e.word_embeddings(t) + e.position_embeddings(torch.arange(9))[None]).numpy()

    want = ln_of(e64)
    e_ref = bo.rel_err(ln_of(e32), want)
    to = lambda p: p.detach().to(dev)             # noqa: E731
    got = ops.bert_encode(t.to(dev), to(e32.word_embeddings.weight), to(e32.position_embeddings.weight), None,
                          to(e32.LayerNorm.weight), to(e32.LayerNorm.bias), float(m32.config.layer_norm_eps), [], 2)
    err = bo.rel_err(got.cpu().numpy(), want)
    print("no token types, absolute positions: err %.3g, e_ref %.3g" % (err, e_ref))
    assert err <= bo.bound(e_ref)


def test_an_out_of_range_id_counts_as_a_token(dev):
    """An id outside the vocabulary: its row is NaN, and the rows behind it sit one position further, as in transformers'
    arithmetic (``ne(pad)``); the other question keeps its bits."""
    m32, m64, ids, _, _ = _case("roberta", 32, 1, 3, 9)
    bad = ids.copy()
    bad[0, 2], bad[1, 0] = lo.VOCAB, -1
    fixed = bad.copy()
    fixed[0, 2], fixed[1, 0] = 5, 7              # any token that is not a pad: the same positions
    with torch.no_grad():
        want = m64.embeddings(input_ids=torch.from_numpy(fixed)).numpy()
    got = lo.encode(dev, m32, bad, L=0).cpu()
    plain = lo.encode(dev, m32, fixed, L=0).cpu()
    nan_rows = torch.isnan(got).all(-1)
    assert nan_rows[0, 2] and nan_rows[1, 0] and int(nan_rows.sum()) == 2 and int(torch.isnan(got).sum()) == 2 * 64
    keep = ~nan_rows
    assert torch.equal(got[keep], plain[keep])
    assert bo.rel_err(plain.numpy(), want) <= 1e-5


# -- attention with a relative bias ---------------------------------------------------------------------------------------

# a single key; several waves; a full wave of keys; the first key in a lane's second slot; the largest T
ATT = [(1, 1, 1, 32), (2, 9, 2, 32), (1, 64, 2, 64), (1, 65, 3, 32), (2, 128, 1, 64)]


def _att_case(B, T, heads, dh):
    rs = np.random.RandomState(200 + T)
    qkv = rs.standard_normal((B * T, 3 * heads * dh)).astype(np.float32)
    bias = rs.standard_normal((heads, 2 * T - 1)).astype(np.float32)       # O(1), nothing symmetric about it
    return qkv, bias


@pytest.mark.parametrize("B,T,heads,dh", ATT)
def test_biased_attention_against_float64(dev, B, T, heads, dh):
    """fp32 against float64 with the fp32 torch statement of the same step as e_ref.  The table is random in (head, j - i):
    reading it at i - j, off by one or from another head's row moves scores by O(1)."""
    from gnnrag_amd import ops
    qkv, bias = _att_case(B, T, heads, dh)
    want = lo.attention64(qkv, B, T, heads, dh, bias)
    x = torch.from_numpy(qkv).view(B, T, 3, heads, dh)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    s = torch.matmul(q, k.transpose(-1, -2)) / np.sqrt(dh) + torch.from_numpy(bias)[:, j - i + T - 1][None]
    ref32 = torch.matmul(torch.softmax(s, -1), v).permute(0, 2, 1, 3).reshape(B * T, heads * dh)
    e_ref = bo.rel_err(ref32.numpy(), want)
    got = ops.bert_attention(torch.from_numpy(qkv).to(dev), B, T, heads, dh, rel_bias=torch.from_numpy(bias).to(dev))
    err = bo.rel_err(got.cpu().numpy(), want)
    wrong = [bo.rel_err(lo.attention64(qkv, B, T, heads, dh, b), want)
             for b in (bias[:, ::-1], np.roll(bias, 1, axis=1), np.zeros_like(bias))] if T > 1 else []
    print("biased attention B=%d T=%d heads=%d dh=%d: err %.3g, e_ref %.3g, bound %.3g; mirrored / shifted / no table: %s"
          % (B, T, heads, dh, err, e_ref, bo.bound(e_ref), ["%.2g" % w for w in wrong]))
    assert got.shape == (B * T, heads * dh)
    assert all(w > 1e3 * bo.bound(e_ref) for w in wrong)
    assert err <= bo.bound(e_ref)
    again = ops.bert_attention(torch.from_numpy(qkv).to(dev), B, T, heads, dh, rel_bias=torch.from_numpy(bias).to(dev))
    assert torch.equal(got, again)


@pytest.mark.parametrize("B,T,heads,dh", ATT)
def test_zero_table_and_no_table_keep_the_bits(dev, B, T, heads, dh):
    from gnnrag_amd import _lib, ops
    qkv = torch.from_numpy(_att_case(B, T, heads, dh)[0]).to(dev)
    plain = ops.bert_attention(qkv, B, T, heads, dh)
    zero = ops.bert_attention(qkv, B, T, heads, dh, rel_bias=torch.zeros(heads, 2 * T - 1, device=dev))
    assert torch.equal(zero, plain)                 # x + 0 is x: the biased kernel adds nothing else
    assert torch.equal(ops.bert_attention(qkv, B, T, heads, dh, rel_bias=None), plain)
    # the new entry point without a table against the old one
    ctx = torch.full_like(plain, float("nan"))
    rc = _lib.load().gnnrag_bert_attention_bias(qkv.data_ptr(), B, T, heads, dh, None, ctx.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(ctx, plain)


# -- the whole encode -------------------------------------------------------------------------------------------------

ENCODE = [(32, 1, 1, 1), (64, 1, 3, 9), (32, 2, 5, 20), (64, 1, 2, 128)]


@pytest.mark.parametrize("math", [MATH_FP32, MATH_BF16X3], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("dh,L,B,T", ENCODE, ids=["L1-1x1", "L1-3x9", "L2-5x20", "L1-2x128"])
@pytest.mark.parametrize("arch", lo.ARCHS)
def test_encode_against_float64(dev, arch, dh, L, B, T, math):
    m32, _, ids, want, e_ref = _case(arch, dh, L, B, T)
    assert B == 1 or (ids == PAD).any()
    got = lo.encode(dev, m32, ids, math=math)
    err = bo.rel_err(got.cpu().numpy(), want)
    print("%s encode H=%d L=%d B=%d T=%d math=%d: err %.3g, e_ref %.3g, ratio %.2f, bound %.3g"
          % (arch, lo.SMALL[dh]["H"], L, B, T, math, err, e_ref, err / max(e_ref, 1e-30), bo.bound(e_ref)))
    assert got.shape == want.shape
    assert err <= bo.bound(e_ref)
    assert torch.equal(got, lo.encode(dev, m32, ids, math=math))                 # the same call twice: equal bits


@pytest.mark.parametrize("arch", lo.ARCHS)
def test_a_question_does_not_depend_on_the_batch(dev, arch):
    """Alone against inside a batch of 5 whose other rows have other pad counts (the position count of a row reads its
    own question only)."""
    m32, _, ids, _, _ = _case(arch, 32, 2, 5, 20)
    assert len({int((r == PAD).sum()) for r in ids}) >= 4 and len({tuple(r == PAD) for r in ids}) == 5
    batch = lo.encode(dev, m32, ids)
    for b in range(5):
        assert torch.equal(lo.encode(dev, m32, ids[b:b + 1]), batch[b:b + 1]), b


def test_bert_defaults_are_the_explicit_call(dev):
    """``ops.bert_encode`` with the default arguments (the old entry point) and with ``pad_id=None, rel_bias=None`` spelled
    out, and the new entry point with a negative pad id and no table: one set of bits."""
    from gnnrag_amd import _lib, ops
    m32, _, ids, want, e_ref = _case("bert", 32, 2, 5, 20)
    P = bo.layer_params(m32)
    to = lambda p: p.detach().to(dev)             # noqa: E731
    layers = [{k: to(v) for k, v in d.items()} for d in P["layers"]]
    top = [to(P[k]) for k in ("word_emb", "pos_emb", "type_emb", "ln_g", "ln_b")]
    t = torch.from_numpy(ids).to(dev)
    a = ops.bert_encode(t, *top, P["eps"], layers, P["heads"], I=P["I"])
    b = ops.bert_encode(t, *top, P["eps"], layers, P["heads"], I=P["I"], pad_id=None, rel_bias=None)
    assert torch.equal(a, b) and bo.rel_err(a.cpu().numpy(), want) <= bo.bound(e_ref)
    lib = _lib.load()
    arr = (_lib.BertLayer * 2)()
    for l, d in enumerate(layers):
        for k, v in d.items():
            setattr(arr[l], k, v.data_ptr())
    out = torch.full_like(a, float("nan"))
    ws = torch.empty(lib.gnnrag_bert_workspace_bytes(5, 20, 64, 128), dtype=torch.uint8, device=dev)
    rc = lib.gnnrag_bert_encode_ex(t.data_ptr(), top[0].data_ptr(), lo.VOCAB, top[1].data_ptr(), top[1].shape[0],
                                   top[2].data_ptr(), -1, None, top[3].data_ptr(), top[4].data_ptr(), P["eps"], 2, arr, 5,
                                   20, 64, 2, 128, out.data_ptr(), ws.data_ptr(), ws.numel(), MATH_FP32,
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(out, ops.bert_encode(t, *top, P["eps"], layers, P["heads"], I=P["I"], math=MATH_FP32))


# -- the module ---------------------------------------------------------------------------------------------------------

FIXTURE = [("roberta", "roberta"), ("sbert2", "mpnet")]


def _fixture_module(dev, tag, arch):
    g = np.load(GOLDEN)
    c = lambda k: int(g["%s.cfg.%s" % (tag, k)])    # noqa: E731
    cfg = lo.config(arch, H=c("H"), heads=c("heads"), I=c("I"), L=c("L"), vocab=c("vocab"), max_pos=c("max_pos"),
                    pad=c("pad_val"))
    m32, m64 = lo.make_model(arch, cfg, c("seed"))
    for p in m32.parameters():
        p.requires_grad_(False)                 # lm_frozen = 1 (bert_encoder.py:80-83)
    mod = bo.make_instruction_standin(m32, c("entity_dim"), c("num_step"), c("pad_val"))
    pre = tag + ".param."
    own = {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}
    missing, unexpected = mod.load_state_dict(own, strict=False)
    assert own and not unexpected and all(k.startswith("node_encoder.") for k in missing)
    return mod.to(dev).eval(), m64, {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + ".")}


class _Model:
    def __init__(self, instruction):
        self.instruction = instruction


def _count_original(mod):
    p = mod.node_encoder._gnnrag_lm_patch
    calls, orig = [], p.orig_forward

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    p.orig_forward = counted
    return p, calls


@pytest.mark.parametrize("hip_instruction", ["0", "1"])
@pytest.mark.parametrize("tag,arch", FIXTURE)
def test_patched_module_reproduces_the_reference_fixture(dev, monkeypatch, tag, arch, hip_instruction):
    from gnnrag_amd import install
    mod, m64, g = _fixture_module(dev, tag, arch)
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    monkeypatch.setenv("GNNRAG_HIP_INSTRUCTION", hip_instruction)
    install.patch_lm_encoder(_Model(mod))
    install.patch_instruction(_Model(mod))
    p, calls = _count_original(mod)
    q = torch.from_numpy(g["q_input"]).long().to(dev)
    with torch.no_grad():
        instructions, attn = mod(q)
    assert p.hip_calls == 1 and not calls
    want = lo.states(m64, g["q_input"])
    e_ref = float(g["lm.e_ref"])
    err = bo.rel_err(mod.lm_states.cpu().numpy(), want)
    print("%s fixture LM states: err %.3g, e_ref %.3g (recorded by the reference's fp32 run), bound %.3g"
          % (tag, err, e_ref, bo.bound(e_ref)))
    assert err <= bo.bound(e_ref)
    figs = {"query_hidden_emb": np.abs(mod.query_hidden_emb.cpu().numpy() - g["query_hidden_emb"]).max(),
            "instructions": np.abs(torch.stack(instructions).cpu().numpy() - g["instructions"]).max(),
            "attn": np.abs(torch.stack(attn).cpu().numpy() - g["attn"]).max()}
    print("%s fixture, GNNRAG_HIP_INSTRUCTION=%s: %s" % (tag, hip_instruction, figs))
    assert all(v <= TOL_INS for v in figs.values()), figs


@pytest.mark.parametrize("tag,arch", FIXTURE)
def test_switch_and_training_mode_on_the_device(dev, monkeypatch, tag, arch):
    """Trainer_KBQA runs the frozen LM in training mode (dropout 0.1): transformers' own forward, counted; unset and
    ``GNNRAG_HIP_LM=0`` go by the module's per-class default."""
    from gnnrag_amd import install
    from gnnrag_amd.modules.question_encoding import lm_encoder
    mod, _, g = _fixture_module(dev, tag, arch)
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    install.patch_lm_encoder(_Model(mod))
    p, calls = _count_original(mod)
    q = torch.from_numpy(g["q_input"]).long().to(dev)
    mod.train()
    assert mod.node_encoder.config.hidden_dropout_prob == 0.1
    with torch.no_grad():
        out = mod.node_encoder(q)
    assert len(calls) == 1 and p.hip_calls == 0 and hasattr(out, "pooler_output")
    mod.eval()
    with torch.no_grad():
        out = mod.node_encoder(q)
        assert len(calls) == 1 and p.hip_calls == 1 and not hasattr(out, "pooler_output")
        mod.node_encoder(q, attention_mask=torch.ones_like(q))
        assert len(calls) == 2 and p.hip_calls == 1
        monkeypatch.setenv("GNNRAG_HIP_LM", "0")
        mod.node_encoder(q)
        assert len(calls) == 3 and p.hip_calls == 1
        monkeypatch.delenv("GNNRAG_HIP_LM")
        mod.node_encoder(q)
        on = type(mod.node_encoder).__name__ in lm_encoder.DEFAULT_ON
        assert (len(calls), p.hip_calls) == ((3, 2) if on else (4, 1))
