"""Relation-text features, host side: the float64 oracle of the GPU tests reproduces the live reference's fixture; the
entry points are declared in gnnrag.h and in the binding (additive to ABI 16) and refuse bad arguments, small workspaces
and shapes outside the limits before they touch a device; ``patch_rel_feature`` on CPU tensors, with the switch off, for
``lm='lstm'`` and for ``rel_texts is None`` is the model's own method, bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

import rel_text_oracle as ro

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "rel_text_ref.npz")
SYMBOLS = {"gnnrag_rel_text_workspace_bytes": 5, "gnnrag_rel_text_pool": 17,
           "gnnrag_rel_text_backward_workspace_bytes": 5, "gnnrag_rel_text_pool_backward": 18}
E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3


@pytest.mark.parametrize("tag", sorted(ro.FIXTURE_CASES))
def test_oracle_reproduces_the_live_reference_fixture(tag):
    """Within the reference's own fp32 error (recorded next to the results), and never beyond 2e-6 of the largest entry."""
    c, want, ref_err = ro.fixture_case(np.load(GOLDEN), tag)
    assert tuple(c["Xs"][0].shape) + (c["W"].shape[0],) == ro.FIXTURE_CASES[tag]
    lens = c["mask"].sum(1)
    assert (lens == 0).any() and (lens == 1).any() and (lens == c["mask"].shape[1]).any()
    for name, n_dir in (("two", 2), ("one", 1)):
        got = ro.oracle(c["Xs"][:n_dir], c["mask"], c["W"], c["b"], c["a"], c["gs"][:n_dir])
        err = ro.errors(want[name], got)
        for q in ro.QUANTITIES:
            assert err[q] <= 2e-6, (name, q, err[q])
            assert abs(err[q] - ref_err[str(n_dir)][q]) <= 1e-9, (name, q)


def test_fixture_has_a_case_beyond_the_uniform_range_and_away_from_the_boundaries():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 1000000
    big = [tag for tag in ro.FIXTURE_CASES if float(z[tag + ".pad_score_max"]) > 4.0]
    assert big
    for tag in ro.FIXTURE_CASES:
        c, _, _ = ro.fixture_case(z, tag)
        for X in c["Xs"]:
            s, pad = ro.scores(X, c["mask"], c["W"], c["b"], c["a"])
            v = np.abs(s[pad]).ravel()
            assert np.abs(v % 8.0 - 4.0).min() >= 0.05


def test_oracle_rows_of_padding_only_are_uniform_below_four_and_quantised_beyond():
    c = ro.random_case(6, 5, 8, 3, seed=2)
    X, mask = torch.from_numpy(c["Xs"][0]).double(), torch.from_numpy(c["mask"]).double()
    W, b, a = (torch.from_numpy(c[k]).double() for k in ("W", "b", "a"))
    _, alpha, s = ro.pool64(X, mask, W, b, a.reshape(-1))
    assert float(s[-1].abs().max()) < 3.5 and not c["mask"][-1].any()
    assert torch.equal(alpha[-1], torch.full((5,), 0.2, dtype=torch.float64))
    assert float(alpha[1, 1:].abs().max()) == 0.0 and float(alpha[1, 0]) == 1.0        # one token: padding gets exactly 0
    s = torch.tensor([[5.0, -3.0, 13.0]], dtype=torch.float64)
    got = torch.softmax(ro.masked_scores(s, torch.zeros(1, 3, dtype=torch.float64)), 1)
    want = torch.softmax(torch.tensor([[8.0, 0.0, 16.0]], dtype=torch.float64), 1)     # fp32(s - 1e8) + 1e8
    assert torch.allclose(got, want, rtol=0, atol=1e-15)


def test_header_and_binding_declare_the_entry_points():
    from gnnrag_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gnnrag.h")).read(), flags=re.S)
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "gnnrag.h does not declare " + name
        assert len(m.group(1).split(",")) == n_args
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    for k, v in (("T", ops.REL_TEXT_MAX_T), ("K", ops.REL_TEXT_MAX_K), ("D", ops.REL_TEXT_MAX_D)):
        assert re.search(r"#define\s+GNNRAG_REL_TEXT_MAX_%s\s+%d\b" % (k, v), src)
    assert ops.REL_TEXT_MAX_T >= 64 and ops.REL_TEXT_MAX_D >= 256 and ops.REL_TEXT_MAX_K >= 768
    assert re.search(r"#define\s+GNNRAG_ABI_VERSION\s+16\b", src) and _lib.ABI_VERSION == 16
    assert "rel_text.hip" in __import__("gnnrag_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.fixture(scope="module")
def lib():
    from gnnrag_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.gnnrag_abi_version() == 16
    return lib


def test_library_exports_the_symbols(lib):
    for name in SYMBOLS:
        assert getattr(lib, name) is not None


P = 4096       # a dummy non-NULL, 16-byte aligned address: an argument error must come back before anything is dereferenced
FWD = ("X_fwd", "X_inv", "mask", "W", "b", "a", "out_fwd", "out_inv", "xbar", "alpha", "ws")
BWD = ("X_fwd", "X_inv", "W", "a", "xbar", "alpha", "g_fwd", "g_inv", "dW", "db", "da", "ws")


def _fwd(lib, R=3, T=2, K=8, D=5, ws_bytes=None, **over):
    p = dict.fromkeys(FWD, P)
    p.update(over)
    n_dir = 2 if p["X_inv"] else 1
    if ws_bytes is None:
        ws_bytes = lib.gnnrag_rel_text_workspace_bytes(R, T, K, D, n_dir) or 1 << 20
    return lib.gnnrag_rel_text_pool(p["X_fwd"], p["X_inv"], p["mask"], p["W"], p["b"], p["a"], R, T, K, D, p["out_fwd"],
                                    p["out_inv"], p["xbar"], p["alpha"], p["ws"], ws_bytes, None)


def _bwd(lib, R=3, T=2, K=8, D=5, ws_bytes=None, **over):
    p = dict.fromkeys(BWD, P)
    p.update(over)
    n_dir = 2 if p["X_inv"] else 1
    if ws_bytes is None:
        ws_bytes = lib.gnnrag_rel_text_backward_workspace_bytes(R, T, K, D, n_dir) or 1 << 20
    return lib.gnnrag_rel_text_pool_backward(p["X_fwd"], p["X_inv"], p["W"], p["a"], p["xbar"], p["alpha"], p["g_fwd"],
                                             p["g_inv"], R, T, K, D, p["dW"], p["db"], p["da"], p["ws"], ws_bytes, None)


@pytest.mark.parametrize("null", ["X_fwd", "mask", "W", "b", "a", "out_fwd"])
def test_forward_null_pointers_are_bad_arguments(lib, null):
    assert _fwd(lib, **{null: None}) == E_BADARG


def test_forward_directions_must_be_consistent(lib):
    assert _fwd(lib, X_inv=None) == E_BADARG                       # out_inv without X_inv
    assert _fwd(lib, out_inv=None) == E_BADARG                     # X_inv without out_inv


@pytest.mark.parametrize("null", ["X_fwd", "W", "a", "xbar", "alpha"])
def test_backward_null_pointers_are_bad_arguments(lib, null):
    assert _bwd(lib, **{null: None}) == E_BADARG


def test_backward_gradient_of_a_direction_that_is_not_there(lib):
    assert _bwd(lib, X_inv=None) == E_BADARG                       # g_inv without X_inv


def test_sizes_are_checked_first(lib):
    for call in (_fwd, _bwd):
        for kw in (dict(R=0), dict(R=-1), dict(T=0), dict(T=-2), dict(K=0), dict(K=-4), dict(D=0), dict(D=-1)):
            assert call(lib, **kw) == E_BADARG, (call.__name__, kw)


def test_shapes_outside_the_limits_are_unsupported_before_anything_is_launched(lib):
    from gnnrag_amd import ops
    for call in (_fwd, _bwd):
        for kw in (dict(T=ops.REL_TEXT_MAX_T + 1), dict(K=6), dict(K=ops.REL_TEXT_MAX_K + 4), dict(D=ops.REL_TEXT_MAX_D + 1),
                   dict(R=(1 << 24) + 1), dict(X_fwd=P + 4), dict(X_inv=P + 8), dict(xbar=P + 4), dict(ws=P + 4)):
            assert call(lib, **kw) == E_UNSUPPORTED, (call.__name__, kw)
    assert _bwd(lib, dW=P + 4) == E_UNSUPPORTED


def test_a_workspace_below_the_stated_size_is_refused(lib):
    for call, size in ((_fwd, lib.gnnrag_rel_text_workspace_bytes), (_bwd, lib.gnnrag_rel_text_backward_workspace_bytes)):
        for R, T, K, D in ((3, 2, 8, 5), (130, 12, 384, 50)):
            need = size(R, T, K, D, 2)
            assert need > 0
            assert call(lib, R, T, K, D, ws_bytes=need - 1) == E_WORKSPACE
            assert call(lib, R, T, K, D, ws_bytes=0) == E_WORKSPACE
            assert call(lib, R, T, K, D, ws=None) == E_WORKSPACE


def test_workspace_size_functions(lib):
    from gnnrag_amd import ops
    f, g = lib.gnnrag_rel_text_workspace_bytes, lib.gnnrag_rel_text_backward_workspace_bytes
    for size in (f, g):
        assert size(0, 2, 8, 5, 1) == 0 and size(3, 0, 8, 5, 1) == 0 and size(3, 2, 6, 5, 1) == 0
        assert size(3, 2, 8, 5, 0) == 0 and size(3, 2, 8, 5, 3) == 0
        assert size(3, ops.REL_TEXT_MAX_T + 1, 8, 5, 1) == 0 and size(3, ops.REL_TEXT_MAX_T, 8, 5, 1) > 0
        assert size(6106, 20, 384, 50, 2) > size(6106, 20, 384, 50, 1) > 0
        assert size(6106, 20, 384, 50, 2) % 256 == 0
    # forward: u and c, then xbar of every direction
    assert f(100, 7, 384, 50, 2) >= (384 + 1 + 2 * 100 * 384) * 4
    assert f(100, 7, 384, 50, 2) == f(100, 64, 384, 200, 2)              # T and D do not enter
    # backward: W^T, dxbar, the stacked padded gradients, the du partial sums, du, the padded dW, the gemm_tn scratch
    R, K, D, Dp = 100, 384, 50, 52
    assert g(R, 7, K, D, 2) >= (K * D + 2 * R * K + 2 * R * Dp + 2 * 512 * K + K + Dp * K) * 4 + \
        lib.gnnrag_gemm_tn_workspace_bytes(2 * R, Dp, K)


def test_binding_states_the_same_limits():
    from gnnrag_amd import ops
    ok = ops.rel_text_supported
    assert ok(6106, 20, 384, 50) and ok(6106, 20, 768, 200) and ok(1, 1, 4, 1) and ok(1 << 24, 256, 4096, 4096)
    assert not ok(0, 1, 4, 1) and not ok(3, 257, 4, 1) and not ok(3, 2, 6, 1) and not ok(3, 2, 4100, 1)
    assert not ok(3, 2, 4, 4097) and not ok((1 << 24) + 1, 2, 4, 1) and not ok(3, 0, 4, 1)


def test_the_wrappers_refuse_cpu_tensors():
    from gnnrag_amd import _lib, ops
    c = ro.random_case(3, 2, 8, 5, seed=0)
    t = torch.from_numpy
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.rel_text_pool(t(c["Xs"][0]), t(c["Xs"][1]), t(c["mask"]), t(c["W"]), t(c["b"]), t(c["a"]))
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.rel_text_pool_backward(t(c["Xs"][0]), None, t(c["W"]), t(c["a"]), torch.zeros(1, 3, 8), torch.zeros(1, 3, 2),
                                   t(c["gs"][0]))


def _no_library(monkeypatch):
    from gnnrag_amd import ops

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(ops, "rel_text_pool", boom)
    monkeypatch.setattr(ops, "rel_text_pool_backward", boom)


def _same(want, got):
    want, got = (want if isinstance(want, tuple) else (want,)), (got if isinstance(got, tuple) else (got,))
    return len(want) == len(got) and all(torch.equal(w, g) for w, g in zip(want, got))


@pytest.mark.parametrize("switch", [None, "0", "1"])
@pytest.mark.parametrize("directions", [1, 2])
def test_patched_model_on_cpu_tensors_is_the_original_bit_for_bit(monkeypatch, switch, directions):
    from gnnrag_amd.modules.rel_text import patch_rel_feature
    if switch is None:
        monkeypatch.delenv("GNNRAG_HIP_REL_TEXT", raising=False)
    else:
        monkeypatch.setenv("GNNRAG_HIP_REL_TEXT", switch)
    _no_library(monkeypatch)
    plain = ro.make_standin(9, 4, 8, 5, directions=directions, seed=3)
    patched = ro.make_standin(9, 4, 8, 5, directions=directions, seed=3)
    patched.load_state_dict(plain.state_dict())
    assert patch_rel_feature(patched, directions) is patched and "get_rel_feature" in patched.__dict__
    with torch.no_grad():
        assert _same(plain.get_rel_feature(), patched.get_rel_feature())
    out = patched.get_rel_feature()                                # under autograd: the reference's ops, its gradients
    (out[0] if directions == 2 else out).sum().backward()
    assert patched.instruction.question_emb.weight.grad is not None
    assert float(patched.self_att_r.attn_linear.weight.grad.abs().sum()) > 0
    assert patched.calls == 2


@pytest.mark.parametrize("why", ["lstm", "no_texts"])
def test_lstm_branch_and_embedding_branch_fall_through(monkeypatch, why):
    """With the switch ON: ``lm='lstm'`` (the reference's second pooling fails there - and must fail the same way) and
    ``rel_texts is None`` (the relation-embedding branch) are the original method's business."""
    from gnnrag_amd.modules.rel_text import patch_rel_feature
    monkeypatch.setenv("GNNRAG_HIP_REL_TEXT", "1")
    _no_library(monkeypatch)
    kw = dict(lm="lstm") if why == "lstm" else {}
    plain, patched = (ro.make_standin(9, 4, 8, 5, seed=4, **kw) for _ in range(2))
    patched.load_state_dict(plain.state_dict())
    patch_rel_feature(patched, 2)
    if why == "no_texts":
        plain.rel_texts = patched.rel_texts = None
        with torch.no_grad():
            assert _same(plain.get_rel_feature(), patched.get_rel_feature())
    else:
        errs = []
        for m in (plain, patched):
            with pytest.raises(Exception) as e, torch.no_grad():
                m.get_rel_feature()
            errs.append((type(e.value), str(e.value)))
        assert errs[0] == errs[1]
    assert patched.calls == 1


def test_switch_off_goes_straight_to_the_original_method(monkeypatch):
    """GNNRAG_HIP_REL_TEXT=0 is read at every call: the wrapper hands over before it looks at anything."""
    from gnnrag_amd.modules import rel_text as mr

    class Probe:
        rel_texts = property(lambda self: (_ for _ in ()).throw(AssertionError("state inspected")))

        def get_rel_feature(self):
            return "orig"

    m = mr.patch_rel_feature(Probe(), 2)
    monkeypatch.setenv("GNNRAG_HIP_REL_TEXT", "0")
    assert not mr.enabled() and m.get_rel_feature() == "orig"
    monkeypatch.delenv("GNNRAG_HIP_REL_TEXT")
    assert mr.DEFAULT == "0" and not mr.enabled() and m.get_rel_feature() == "orig"
    monkeypatch.setenv("GNNRAG_HIP_REL_TEXT", "1")
    assert mr.enabled()
    with pytest.raises(AssertionError, match="state inspected"):
        m.get_rel_feature()


def test_patch_is_idempotent_defaults_directions_and_sits_under_the_cache():
    from gnnrag_amd import install
    from gnnrag_amd.modules.rel_text import patch_rel_feature
    m = ro.make_standin(9, 4, 8, 5, seed=5)
    keys = list(m.state_dict())
    assert install.patch_rel_feature(m) is m
    wrapped = m.get_rel_feature
    assert wrapped.__self__.directions == 2 and patch_rel_feature(m) is m and m.get_rel_feature == wrapped
    assert list(m.state_dict()) == keys
    install.cache_rel_features(m)
    cached = m.get_rel_feature
    assert cached._gnnrag_cached and patch_rel_feature(m) is m and m.get_rel_feature is cached
    m.eval()
    with torch.no_grad():
        a, b = m.get_rel_feature(), m.get_rel_feature()
    assert m.calls == 1 and a[0] is b[0]

    class NSM(torch.nn.Module):
        def get_rel_feature(self):
            return None
    assert patch_rel_feature(NSM()).get_rel_feature.__self__.directions == 1
    other = torch.nn.Linear(3, 3)
    assert patch_rel_feature(other) is other and "get_rel_feature" not in other.__dict__
    with pytest.raises(ValueError):
        patch_rel_feature(ro.make_standin(9, 4, 8, 5), 3)
