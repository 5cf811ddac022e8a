"""Host side of fine-tuning the LM question encoder (CPU, no GPU): the numpy float64 statements of the three backward
kernels (tests/bert_grad_oracle.py) against torch float64 autograd, the key-bias fact the library relies on, the reserve and
workspace sizes against a Python restatement of their layout, and the switch ``GNNRAG_HIP_LM_FINETUNE`` on CPU stand-ins."""
import copy

import numpy as np
import pytest
import torch

import bert_dropout_oracle as do
import bert_grad_oracle as go
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

@pytest.mark.parametrize("drop", [False, True])
def test_attention_statement_against_autograd(drop):
    B, T, heads, dh = 2, 7, 2, 32
    rs = np.random.RandomState(1)
    qkv = rs.standard_normal((B * T, 3 * heads * dh))
    d_ctx = rs.standard_normal((B * T, heads * dh))
    keep = (rs.random_sample((B, heads, T, T)) >= 0.3).astype(np.uint8) if drop else None
    scale = do.scale(0.3) if drop else 1.0
    x = torch.from_numpy(qkv).requires_grad_(True)
    v = x.view(B, T, 3, heads, dh)
    q, k, val = (v[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / float(np.sqrt(dh)), dim=-1)
    if drop:
        p = p * torch.from_numpy(keep).double() * scale
    ctx = torch.matmul(p, val).permute(0, 2, 1, 3).reshape(B * T, heads * dh)
    ctx.backward(torch.from_numpy(d_ctx))
    assert _rel(go.attention_bwd64(qkv, d_ctx, B, T, heads, dh, keep, scale), x.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("drop", [False, True])
def test_layernorm_statement_against_autograd(drop):
    M, H, eps = 5, 32, 1e-12
    rs = np.random.RandomState(2)
    dy, d, res = (rs.standard_normal((M, H)) for _ in range(3))
    g, b = 1.0 + 0.1 * rs.standard_normal(H), 0.1 * rs.standard_normal(H)
    keep = (rs.random_sample((M, H)) >= 0.5).astype(np.uint8) if drop else None
    scale = do.scale(0.5) if drop else 1.0
    td, tr = torch.from_numpy(d).requires_grad_(True), torch.from_numpy(res).requires_grad_(True)
    tg, tb = torch.from_numpy(g).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    z = td * torch.from_numpy(keep).double() * scale + tr if drop else td
    torch.nn.functional.layer_norm(z, (H,), tg, tb, eps).backward(torch.from_numpy(dy))
    dz, dY, dgamma, dbeta = go.ln_bwd64(dy, d, g, eps, keep, scale, res if drop else None)
    assert _rel(dY, td.grad.numpy()) <= 1e-12 and _rel(dgamma, tg.grad.numpy()) <= 1e-12
    assert _rel(dbeta, tb.grad.numpy()) <= 1e-12
    if drop:
        assert _rel(dz, tr.grad.numpy()) <= 1e-12


def test_gelu_statement_against_autograd():
    rs = np.random.RandomState(3)
    pre = np.concatenate([rs.standard_normal(50) * 3, [10.0, -10.0, 0.0]])
    d_act = rs.standard_normal(pre.shape)
    x = torch.from_numpy(pre).requires_grad_(True)
    y = torch.nn.functional.gelu(x)
    y.backward(torch.from_numpy(d_act))
    d_pre, act = go.gelu_bwd64(pre, d_act)
    assert _rel(d_pre, x.grad.numpy()) <= 1e-12 and _rel(act, y.detach().numpy()) <= 1e-12


# -- the key bias --------------------------------------------------------------------------------------------------------

def test_key_bias_gradient_is_zero_in_float64():
    """Every row of dS sums to zero: the float64 module's key.bias gradient is below 1e-12 of the same layer's query.bias
    gradient, with dropout at both sites - the library writes exactly 0 there."""
    pytest.importorskip("transformers")
    L, B, T = 2, 3, 9
    _, m64 = do.make_bert(SMALL, L, seed=31, max_pos=16)
    rs = np.random.RandomState(32)
    ids = rs.randint(0, 64, (B, T))
    masks = do.draw(33, L, B, T, 64, 2, 0.1, 0.1)
    G = go.grads(m64, [(ids, masks, do.scale(0.1), do.scale(0.1))], [rs.standard_normal((B, T, 64))])
    for l in range(L):
        names = go.layer_names(m64, l)["db_qkv"]
        gq, gk = G[names[0]], G[names[1]]
        assert np.abs(gq).max() > 0 and np.abs(gk).max() <= 1e-12 * np.abs(gq).max()
    assert G["pooler.dense.weight"] is None and G["pooler.dense.bias"] is None


# -- sizes ---------------------------------------------------------------------------------------------------------------

def _up(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("L,B,T,H,heads,I", [(1, 1, 1, 384, 12, 1536), (2, 3, 9, 64, 2, 128), (12, 64, 20, 768, 12, 3072)])
def test_reserve_and_workspace_sizes(lib, L, B, T, H, heads, I):
    M = B * T
    assert lib.gnnrag_bert_reserve_bytes(L, B, T, H, I) == L * M * (8 * H + I) * 4
    mh, mi = M * H * 4, M * I * 4
    tn = max(lib.gnnrag_gemm_tn_workspace_bytes(M, H, I), lib.gnnrag_gemm_tn_workspace_bytes(M, I, H),
             lib.gnnrag_gemm_tn_workspace_bytes(M, H, H), lib.gnnrag_gemm_tn_workspace_bytes(M, 3 * H, H))
    want = (7 * _up(mh) + 2 * _up(mi) + _up(3 * mh) + _up(H * max(3 * H, I) * 4) + _up(B * heads * 2 * T * T * 4) + _up(tn))
    assert lib.gnnrag_bert_layers_backward_workspace_bytes(B, T, H, heads, I) == want
    assert lib.gnnrag_bert_attention_backward_workspace_bytes(B, T, heads) == B * heads * 2 * T * T * 4


def test_sizes_of_refused_shapes_are_zero(lib):
    from gnnrag_amd import ops
    assert lib.gnnrag_bert_reserve_bytes(0, 2, 5, 64, 128) == 0 and lib.gnnrag_bert_reserve_bytes(1, 2, 5, 62, 128) == 0
    assert lib.gnnrag_bert_reserve_bytes(1, 2, 5, 64, 126) == 0
    assert lib.gnnrag_bert_layers_backward_workspace_bytes(2, 129, 64, 2, 128) == 0     # T > 128
    assert lib.gnnrag_bert_layers_backward_workspace_bytes(2, 5, 96, 2, 128) == 0       # head width 48
    assert lib.gnnrag_bert_layers_backward_workspace_bytes(2, 5, 64, 2, 126) == 0       # I % 4
    assert ops.bert_layers_backward_supported(20, 384, 12, 1536) and not ops.bert_layers_backward_supported(129, 384, 12, 1536)
    assert not ops.bert_layers_backward_supported(20, 96, 2, 128) and not ops.bert_layers_backward_supported(20, 64, 2, 126)


def test_argument_rules_before_any_launch(lib):
    """Sizes, then shapes whatever the pointers are, then NULL pointers, then alignment, then the buffer sizes."""
    from gnnrag_amd import _lib
    OK, ODD = 0x10000, 0x10004
    arr = (_lib.BertLayer * 1)()
    for n, _ in _lib.BertLayer._fields_:
        setattr(arr[0], n, OK)
    save = lambda x0=OK, L=1, T=5, H=64, I=128, out=OK, rb=1 << 30, wb=1 << 30, sh=2.0, kh=None: \
        lib.gnnrag_bert_layers_forward_save(x0, L, arr, 1e-12, 2, T, H, 2, I, kh, sh, None, 1.0, out, OK, rb, OK, wb, 0, None)  # noqa: E731
    bwd = lambda g=OK, L=1, T=5, H=64, I=128, rb=1 << 30, wb=1 << 30, gx=OK: \
        lib.gnnrag_bert_layers_backward(g, L, arr, 1e-12, 2, T, H, 2, I, None, 1.0, None, 1.0, OK, rb, gx, None, OK, wb, None)  # noqa: E731
    for call in (save, bwd):
        assert call(L=0) == -1 and call(None, T=129) == -2 and call(None, H=96) == -2 and call(None, I=126) == -2
        assert call(None) == -1 and call(ODD) == -2 and call(rb=16) == -3 and call(wb=16) == -3
    assert save(kh=OK, sh=float("inf")) == -1 and save(kh=ODD + 2) == -2
    assert lib.gnnrag_bert_attention_backward(OK, OK, 2, 5, 2, 48, None, 1.0, OK, OK, 1 << 20, None) == -2
    assert lib.gnnrag_bert_attention_backward(OK, None, 2, 5, 2, 32, None, 1.0, OK, OK, 1 << 20, None) == -1
    assert lib.gnnrag_bert_attention_backward(OK, OK, 2, 5, 2, 32, None, 1.0, OK, OK, 16, None) == -3
    assert lib.gnnrag_bert_ln_backward(OK, OK, OK, 2.0, None, OK, 1e-12, 4, 64, OK, OK, OK, None, None, None) == -1
    assert lib.gnnrag_bert_ln_backward(OK, OK, None, 1.0, None, OK, 1e-12, 4, 62, OK, None, OK, None, None, None) == -2
    assert lib.gnnrag_bert_gelu_backward(OK, OK, 0, OK, None, None) == -1
    assert lib.gnnrag_bert_gelu_backward(OK, ODD, 8, OK, None, None) == -2


# -- the switch ----------------------------------------------------------------------------------------------------------

class _Holder:
    def __init__(self, enc):
        self.node_encoder = enc


def test_finetune_switch_refusals(monkeypatch):
    pytest.importorskip("transformers")
    from gnnrag_amd.modules.question_encoding import lm_encoder as le
    enc = copy.deepcopy(bo.make_model(bo.config(L=1, vocab=50, max_pos=16, **SMALL), seed=5)[0])
    le.patch_lm_encoder(_Holder(enc))
    p = enc._gnnrag_lm_patch
    ids = torch.from_numpy(np.random.RandomState(0).randint(0, 50, (2, 5))).long()
    enc.train()
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    monkeypatch.delenv("GNNRAG_HIP_LM_TRAIN", raising=False)
    monkeypatch.delenv("GNNRAG_HIP_LM_FINETUNE", raising=False)
    assert p.hip_finetune_calls == 0 and p.needs_grad()
    assert not le.finetune_enabled() and p.refusal((ids,), {}) == "a gradient is needed"            # unset: off
    for off in ("0", ""):
        monkeypatch.setenv("GNNRAG_HIP_LM_FINETUNE", off)
        assert p.refusal((ids,), {}) == "a gradient is needed"
    monkeypatch.setenv("GNNRAG_HIP_LM_FINETUNE", "1")                                               # read at every call
    assert le.finetune_enabled() and p.refusal((ids,), {}) == "input_ids is not a CUDA tensor"      # every rule before it holds
    with monkeypatch.context() as m:
        m.setattr(enc.config, "hidden_dropout_prob", 1.0)
        assert p.refusal((ids,), {}) == "a dropout probability of 1"
    with monkeypatch.context() as m:
        m.setattr(enc.config, "intermediate_size", 126)
        assert p.refusal((ids,), {}) == "a shape the backward kernels do not take"
    assert p.refusal((ids,), {"attention_mask": torch.ones_like(ids)}) == "arguments other than input_ids"
    monkeypatch.setenv("GNNRAG_HIP_LM", "0")
    assert p.refusal((ids,), {}) == "GNNRAG_HIP_LM is off"
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    # nothing requires grad: the frozen rules, unchanged by the switch
    for q in enc.parameters():
        q.requires_grad_(False)
    assert not p.needs_grad() and p.refusal((ids,), {}) == "dropout is active"
    monkeypatch.setenv("GNNRAG_HIP_LM_TRAIN", "1")
    assert p.refusal((ids,), {}) == "input_ids is not a CUDA tensor"
    enc.eval()
    monkeypatch.delenv("GNNRAG_HIP_LM_TRAIN")
    assert p.refusal((ids,), {}) == "input_ids is not a CUDA tensor"
    with torch.no_grad():                       # grad mode off: no gradient is needed whatever the parameters say
        next(enc.parameters()).requires_grad_(True)
        assert not p.needs_grad() and p.refusal((ids,), {}) == "input_ids is not a CUDA tensor"
    # a refused call is transformers' own forward and the counters stand still
    monkeypatch.delenv("GNNRAG_HIP_LM_FINETUNE")
    out = enc(ids)[0]
    assert out.requires_grad and p.hip_calls == 0 and p.hip_finetune_calls == 0


def test_mpnet_keeps_transformers_forward(monkeypatch):
    pytest.importorskip("transformers")
    from gnnrag_amd.modules.question_encoding import lm_encoder as le
    enc = copy.deepcopy(lo.make_model("mpnet", lo.config("mpnet", L=1, **lo.SMALL[32]), seed=6)[0])
    le.patch_lm_encoder(_Holder(enc))
    p = enc._gnnrag_lm_patch
    ids = torch.from_numpy(lo.ids_with_pads(2, 5)).long()
    monkeypatch.setenv("GNNRAG_HIP_LM", "1")
    monkeypatch.delenv("GNNRAG_HIP_LM_FINETUNE", raising=False)
    assert p.refusal((ids,), {}) == "a gradient is needed"
    monkeypatch.setenv("GNNRAG_HIP_LM_FINETUNE", "1")
    assert p.refusal((ids,), {}) == "a gradient is needed and the relative attention bias has no backward on the library"
    rob = copy.deepcopy(lo.make_model("roberta", lo.config("roberta", L=1, **lo.SMALL[32]), seed=7)[0])
    le.patch_lm_encoder(_Holder(rob))
    assert rob._gnnrag_lm_patch.refusal((ids,), {}) == "input_ids is not a CUDA tensor"
