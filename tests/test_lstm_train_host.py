"""The training form of the LSTM, host side: the four entry points are declared in gnnrag.h and in the binding with the
same argument counts (additive to ABI 16), the size queries are what the header says, the tensor wrappers have no CPU
path, and HipLSTM on CPU tensors under autograd is still torch's own LSTM."""
import os
import re

import pytest
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {"gnnrag_lstm_reserve_bytes": 3, "gnnrag_lstm_forward_train": 19, "gnnrag_lstm_backward_workspace_bytes": 4,
       "gnnrag_lstm_backward": 24}


def test_header_and_binding_declare_the_entry_points():
    from gnnrag_amd import _lib
    src = open(os.path.join(REPO, "include", "gnnrag.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_args in NEW.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "gnnrag.h does not declare " + name
        assert len(m.group(1).split(",")) == n_args
        assert name in _lib.SIGNATURES, "the binding lacks " + name
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert re.search(r"#define\s+GNNRAG_ABI_VERSION\s+16\b", src) and _lib.ABI_VERSION == 16
    # the training forward is the inference forward plus (reserve, reserve_bytes)
    assert len(_lib.SIGNATURES["gnnrag_lstm_forward"][1]) + 2 == NEW["gnnrag_lstm_forward_train"]


def test_library_exports_the_entry_points_and_the_reserve_size():
    from gnnrag_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
    assert lib.gnnrag_abi_version() == 16
    # act [B,T,4H] + cs [B,T,H] floats
    assert lib.gnnrag_lstm_reserve_bytes(16, 9, 200) == 16 * 9 * 5 * 200 * 4
    assert lib.gnnrag_lstm_reserve_bytes(1, 1, 50) == 5 * 50 * 4
    assert lib.gnnrag_lstm_reserve_bytes(0, 9, 200) == 0 and lib.gnnrag_lstm_reserve_bytes(16, 9, -1) == 0


@pytest.mark.parametrize("which", ["forward_train", "backward"])
def test_the_wrappers_refuse_cpu_tensors(which):
    from gnnrag_amd import _lib, ops
    B, T, E, H = 2, 3, 8, 4
    x, wi, wh = torch.randn(B, T, E), torch.randn(4 * H, E), torch.randn(4 * H, H)
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        if which == "forward_train":
            ops.lstm_forward_train(x, wi, wh)
        else:
            ops.lstm_backward(x, wi, wh, None, None, torch.randn(B, T, H), torch.zeros(B * T * 5 * H * 4, dtype=torch.uint8),
                              torch.randn(B, T, H))


@pytest.mark.parametrize("switch", [None, "0", "1"])
def test_hiplstm_on_cpu_tensors_under_autograd_is_torchs_own_lstm(monkeypatch, switch):
    from gnnrag_amd.modules.question_encoding.lstm import HipLSTM
    if switch is None:
        monkeypatch.delenv("GNNRAG_HIP_LSTM_TRAIN", raising=False)
    else:
        monkeypatch.setenv("GNNRAG_HIP_LSTM_TRAIN", switch)
    torch.manual_seed(0)
    ref = nn.LSTM(12, 6, batch_first=True)
    hip = HipLSTM.sharing(ref).train()
    x = torch.randn(3, 5, 12)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    want, (wh, wc) = ref(xa)
    (want.sum() + wh.sum() + 2 * wc.sum()).backward()
    grads = [p.grad.clone() for p in ref.parameters()]
    for p in ref.parameters():
        p.grad = None
    got, (gh, gc) = hip(xb)
    (got.sum() + gh.sum() + 2 * gc.sum()).backward()
    assert torch.equal(got, want) and torch.equal(gh, wh) and torch.equal(gc, wc)
    assert torch.equal(xa.grad, xb.grad)
    for p, g in zip(hip.parameters(), grads):
        assert torch.equal(p.grad, g)


def test_argument_checks_come_before_any_launch():
    """Refusals are decided on the host before anything is enqueued, so they can be exercised without a GPU: the
    pointers below are never dereferenced."""
    from gnnrag_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    P = 0x10000                                    # any non-null, 16-byte aligned address
    B, T, E, H = 3, 5, 8, 6
    res = lib.gnnrag_lstm_reserve_bytes(B, T, H)
    ws_f = lib.gnnrag_lstm_workspace_bytes(E, H)
    ws_b = lib.gnnrag_lstm_backward_workspace_bytes(B, T, E, H)
    assert ws_b > B * T * 4 * H * 4                # at least dG
    assert lib.gnnrag_lstm_backward_workspace_bytes(B, T, E, 257) == 0

    def fwd(x=P, reserve=P, reserve_bytes=res, ws_bytes=ws_f, h=H):
        return lib.gnnrag_lstm_forward_train(x, P, P, None, None, None, None, P, P, P, B, T, E, h, reserve, reserve_bytes,
                                             P, ws_bytes, None)

    def bwd(x=P, dw_ih=P, reserve_bytes=res, ws_bytes=ws_b, e=E, h=H):
        return lib.gnnrag_lstm_backward(x, P, P, None, None, P, P, reserve_bytes, None, None, None, None, dw_ih, P, None,
                                        None, None, B, T, e, h, P, ws_bytes, None)

    assert fwd(x=None) == -1 and fwd(h=257) == -2
    assert fwd(reserve_bytes=res - 1) == -3 and fwd(reserve=None) == -3 and fwd(ws_bytes=ws_f - 1) == -3
    assert bwd(x=None) == -1 and bwd(dw_ih=None) == -1
    assert bwd(h=257) == -2 and bwd(e=6) == -2 and bwd(x=P + 4) == -2
    assert bwd(reserve_bytes=res - 1) == -3 and bwd(ws_bytes=ws_b - 1) == -3
