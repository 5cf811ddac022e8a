"""gnnrag_rel_text_pool / gnnrag_rel_text_pool_backward, ops.rel_text_pool*, autograd.RelTextPoolFn and
patch_rel_feature on the MI355X against the float64 oracle (tests/rel_text_oracle.py, pinned to the live reference's
fixture by tests/test_rel_text_host.py).

Tolerance, for every quantity (out, dW, db, da): the error relative to the largest entry of the oracle's result is at most
max(4 x the reference's own fp32 error for that quantity, 1e-6) - the reference's error from the fixture, or computed here
with torch fp32 ops on the same inputs.  4 because only the summation order differs (MFMA tiles, wave reductions): the
same error class.  Every figure is printed before it is asserted (run with -s to see them)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import rel_text_oracle as ro

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "rel_text_ref.npz")
SWEEP = [(1, 1, 4, 1), (37, 5, 20, 12), (130, 12, 384, 50), (65, 64, 768, 200), (1000, 7, 384, 52)]
# the row is kept in LDS while T K + K + 2 ceil4(T) floats fit 80 KB: K = 768 holds T = 25 and not T = 26; beyond 48 KB
# the kernel's LDS cap is raised first
PATHS = [(3, 20, 768, 4), (3, 25, 768, 4), (3, 26, 768, 4)]


@pytest.fixture(scope="module")
def dev():
    import gnnrag_amd  # noqa: F401
    from gnnrag_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def tol(ref_err):
    return {q: max(4.0 * ref_err[q], 1e-6) for q in ro.QUANTITIES}


def to_dev(c, dev, n_dir):
    t = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    return dict(Xs=[t(x) for x in c["Xs"][:n_dir]], mask=t(c["mask"]), W=t(c["W"]), b=t(c["b"]), a=t(c["a"]),
                gs=[t(g) for g in c["gs"][:n_dir]])


def run_gpu(d, keep=False):
    """Forward and backward through the binding; numpy results as the oracle lays them out."""
    from gnnrag_amd import ops
    Xf, Xi = d["Xs"][0], (d["Xs"][1] if len(d["Xs"]) == 2 else None)
    of, oi, xbar, alpha = ops.rel_text_pool(Xf, Xi, d["mask"], d["W"], d["b"], d["a"], save=True)
    dW, db, da = ops.rel_text_pool_backward(Xf, Xi, d["W"], d["a"], xbar, alpha, d["gs"][0],
                                            d["gs"][1] if Xi is not None else None)
    n = lambda t: t.cpu().numpy()      # noqa: E731
    got = dict(out=[n(of)] + ([n(oi)] if oi is not None else []), dW=n(dW), db=n(db), da=n(da))
    if keep:
        got.update(xbar=n(xbar), alpha=n(alpha))
    return got


def check(what, got, want, ref_err):
    err, bound = ro.errors(got, want), tol(ref_err)
    for q in ro.QUANTITIES:
        print("%s %-3s err %.3e  reference %.3e  bound %.3e  ratio to the reference %.2f" %
              (what, q, err[q], ref_err[q], bound[q], err[q] / max(ref_err[q], 1e-30)))
    for q in ro.QUANTITIES:
        assert err[q] <= bound[q], (what, q, err[q], bound[q])


@functools.lru_cache(maxsize=None)
def sweep_case(shape, n_dir):
    """(inputs, float64 oracle, the reference's fp32 error), computed once per shape."""
    c = ro.random_case(*shape, seed=11)
    c = dict(c, Xs=c["Xs"][:n_dir], gs=c["gs"][:n_dir])
    want = ro.oracle(**c)
    ref_err = ro.errors(ro.reference32(**c), want)
    return c, want, ref_err


@pytest.mark.parametrize("n_dir", [1, 2])
@pytest.mark.parametrize("tag", sorted(ro.FIXTURE_CASES))
def test_fixture_parity(dev, tag, n_dir):
    c, _, ref_err = ro.fixture_case(np.load(GOLDEN), tag)
    c = dict(c, Xs=c["Xs"][:n_dir], gs=c["gs"][:n_dir])
    want = ro.oracle(**c)
    check("fixture %s x%d" % (tag, n_dir), run_gpu(to_dev(c, dev, n_dir)), want, ref_err[str(n_dir)])


@pytest.mark.parametrize("shape", SWEEP + PATHS, ids=lambda s: "x".join(map(str, s)))
def test_oracle_sweep(dev, shape):
    c, want, ref_err = sweep_case(shape, 2)
    for X in c["Xs"]:
        s, pad = ro.scores(X, c["mask"], c["W"], c["b"], c["a"])
        assert not pad.any() or np.abs(s[pad]).max() < 3.5
    check("sweep %s" % (shape,), run_gpu(to_dev(c, dev, 2)), want, ref_err)


def test_rows_of_padding_only_and_padded_tokens(dev):
    c, _, _ = sweep_case((37, 5, 20, 12), 2)
    got = run_gpu(to_dev(c, dev, 2), keep=True)
    pad = c["mask"].sum(1) == 0
    assert pad.any() and np.array_equal(got["alpha"][:, pad], np.full_like(got["alpha"][:, pad], np.float32(1.0) / np.float32(5)))
    some = ~pad
    assert (got["alpha"][:, some][:, c["mask"][some] == 0] == 0).all()        # exactly 0, not merely small


def test_one_direction_and_missing_upstream_gradients(dev):
    """X_inv = None is the NSM form; a None gradient of one output is that direction left out of the backward."""
    from gnnrag_amd import ops
    c, want2, ref2 = sweep_case((130, 12, 384, 50), 2)
    c1, want1, ref1 = sweep_case((130, 12, 384, 50), 1)
    check("one direction", run_gpu(to_dev(c1, dev, 1)), want1, ref1)
    d = to_dev(c, dev, 2)
    _, _, xbar, alpha = ops.rel_text_pool(d["Xs"][0], d["Xs"][1], d["mask"], d["W"], d["b"], d["a"], save=True)
    n = lambda t: t.cpu().numpy()      # noqa: E731
    for keep in (0, 1):
        gs = [d["gs"][0] if keep == 0 else None, d["gs"][1] if keep == 1 else None]
        dW, db, da = ops.rel_text_pool_backward(d["Xs"][0], d["Xs"][1], d["W"], d["a"], xbar, alpha, gs[0], gs[1])
        want = ro.oracle(c["Xs"], c["mask"], c["W"], c["b"], c["a"], [c["gs"][0] if keep == 0 else None,
                                                                     c["gs"][1] if keep == 1 else None])
        err = {q: ro.rel_err(v, want[q]) for q, v in (("dW", n(dW)), ("db", n(db)), ("da", n(da)))}
        print("only g[%d]" % keep, err)
        assert all(err[q] <= tol(ref2)[q] for q in err), err
    # outputs nobody wants are not computed
    dW, db, da = ops.rel_text_pool_backward(d["Xs"][0], d["Xs"][1], d["W"], d["a"], xbar, alpha, d["gs"][0], d["gs"][1],
                                            need_dW=False, need_da=False)
    assert dW is None and da is None and ro.rel_err(n(db), want2["db"]) <= tol(ref2)["db"]
    dW, db, da = ops.rel_text_pool_backward(d["Xs"][0], d["Xs"][1], d["W"], d["a"], xbar, alpha, d["gs"][0], d["gs"][1],
                                            need_dW=False, need_db=False)
    assert dW is None and db is None and ro.rel_err(n(da), want2["da"]) <= tol(ref2)["da"]


def test_limits(dev):
    from gnnrag_amd import _lib, ops
    lib = _lib.load()
    T = ops.REL_TEXT_MAX_T
    c = ro.random_case(3, T, 4, 2, seed=12)
    want = ro.oracle(**c)
    check("T at the limit", run_gpu(to_dev(c, dev, 2)), want, ro.errors(ro.reference32(**c), want))
    c = ro.random_case(3, T + 1, 4, 2, seed=12)
    d = to_dev(c, dev, 2)
    with pytest.raises(_lib.GnnragError) as e:
        ops.rel_text_pool(d["Xs"][0], d["Xs"][1], d["mask"], d["W"], d["b"], d["a"])
    assert e.value.code == -2
    # straight through the C ABI: the outputs keep what they held
    full = lambda *s: torch.full(s, 7.0, device=dev)      # noqa: E731
    outs = [full(3, 2), full(3, 2), full(2, 3, 4), full(2, 3, T + 1)]
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    rc = lib.gnnrag_rel_text_pool(d["Xs"][0].data_ptr(), d["Xs"][1].data_ptr(), d["mask"].data_ptr(), d["W"].data_ptr(),
                                  d["b"].data_ptr(), d["a"].data_ptr(), 3, T + 1, 4, 2, *[o.data_ptr() for o in outs],
                                  ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    grads = [full(2, 4), full(2), full(2)]
    rc2 = lib.gnnrag_rel_text_pool_backward(d["Xs"][0].data_ptr(), d["Xs"][1].data_ptr(), d["W"].data_ptr(),
                                            d["a"].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                                            d["gs"][0].data_ptr(), d["gs"][1].data_ptr(), 3, T + 1, 4, 2,
                                            *[g.data_ptr() for g in grads], ws.data_ptr(), ws.numel(),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -2 and rc2 == -2
    assert all(bool((t == 7.0).all()) for t in outs + grads) and not bool(ws.any())


def test_determinism(dev):
    from gnnrag_amd import ops
    c, _, _ = sweep_case((1000, 7, 384, 52), 2)
    d = to_dev(c, dev, 2)
    a, b = run_gpu(d, keep=True), run_gpu(d, keep=True)
    for k in ("dW", "db", "da", "xbar", "alpha"):
        assert np.array_equal(a[k], b[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(a["out"], b["out"]))
    # a row's xbar and alpha do not depend on the other rows: the call on rows [0, R/2)
    h = 500
    _, _, xbar, alpha = ops.rel_text_pool(d["Xs"][0][:h].contiguous(), d["Xs"][1][:h].contiguous(), d["mask"][:h].contiguous(),
                                          d["W"], d["b"], d["a"], save=True)
    assert np.array_equal(xbar.cpu().numpy(), a["xbar"][:, :h]) and np.array_equal(alpha.cpu().numpy(), a["alpha"][:, :h])


# ---- the module sequence -------------------------------------------------------------------------------------------------

def _standin(dev, directions, seed=21, R1=70, T=6, K=32, D=10):
    from gnnrag_amd.modules.rel_text import patch_rel_feature
    plain = ro.make_standin(R1, T, K, D, directions=directions, seed=seed, device=dev)
    patched = ro.make_standin(R1, T, K, D, directions=directions, seed=seed, device=dev)
    patched.load_state_dict(plain.state_dict())
    assert patch_rel_feature(patched, directions) is patched
    return plain, patched


def _tup(v):
    return v if isinstance(v, tuple) else (v,)


@pytest.mark.parametrize("directions", [1, 2])
def test_module_switch_off_is_the_unwrapped_method(dev, monkeypatch, directions):
    plain, patched = _standin(dev, directions)
    for switch in (None, "0"):
        if switch is None:
            monkeypatch.delenv("GNNRAG_HIP_REL_TEXT", raising=False)
        else:
            monkeypatch.setenv("GNNRAG_HIP_REL_TEXT", switch)
        with torch.no_grad():
            for w, g in zip(_tup(plain.get_rel_feature()), _tup(patched.get_rel_feature())):
                assert torch.equal(w, g)
    w = sum(o.sum() for o in _tup(plain.get_rel_feature()))
    g = sum(o.sum() for o in _tup(patched.get_rel_feature()))
    w.backward()
    g.backward()
    for pw, pg in zip(plain.parameters(), patched.parameters()):
        assert (pw.grad is None) == (pg.grad is None) and (pw.grad is None or torch.equal(pw.grad, pg.grad))


@pytest.mark.parametrize("directions", [1, 2])
def test_module_switch_on(dev, monkeypatch, directions):
    from gnnrag_amd import ops
    plain, patched = _standin(dev, directions)
    monkeypatch.setenv("GNNRAG_HIP_REL_TEXT", "1")
    calls = {"fwd": 0, "bwd": 0}
    fwd0, bwd0 = ops.rel_text_pool, ops.rel_text_pool_backward
    monkeypatch.setattr(ops, "rel_text_pool", lambda *a, **k: (calls.__setitem__("fwd", calls["fwd"] + 1), fwd0(*a, **k))[1])
    monkeypatch.setattr(ops, "rel_text_pool_backward",
                        lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + 1), bwd0(*a, **k))[1])
    c = ro.standin_case(plain, directions)
    gen = torch.Generator().manual_seed(3)
    gs = [torch.randn(70, 10, generator=gen) for _ in range(directions)]
    c["gs"] = [g.numpy() for g in gs]
    want = ro.oracle(**c)
    ref_err = ro.errors(ro.reference32(**c), want)
    with torch.no_grad():
        out = _tup(patched.get_rel_feature())
    assert calls == {"fwd": 1, "bwd": 0} and patched.calls == 0 and all(not o.requires_grad for o in out)
    err = max(ro.rel_err(o.cpu().numpy(), w) for o, w in zip(out, want["out"]))
    print("module no_grad out err %.3e bound %.3e" % (err, tol(ref_err)["out"]))
    assert err <= tol(ref_err)["out"]
    out = _tup(patched.get_rel_feature())
    assert all(o.requires_grad for o in out)
    sum((o * g.to(dev)).sum() for o, g in zip(out, gs)).backward()
    assert calls == {"fwd": 2, "bwd": 1} and patched.calls == 0
    emb, att = patched.instruction.question_emb, patched.self_att_r.attn_linear
    assert tuple(att.weight.grad.shape) == (1, 10)
    got = dict(out=[o.detach().cpu().numpy() for o in out], dW=emb.weight.grad.cpu().numpy(), db=emb.bias.grad.cpu().numpy(),
               da=att.weight.grad.cpu().numpy().reshape(-1))
    check("module autograd x%d" % directions, got, want, ref_err)
    assert patched.rel_features.grad is None and not patched.rel_features.requires_grad
    assert patched.rel_features_inv.grad is None
    # only one output used: the other direction's gradient arrives as None
    if directions == 2:
        for p in (emb.weight, emb.bias, att.weight):
            p.grad = None
        (patched.get_rel_feature()[1] * gs[1].to(dev)).sum().backward()
        want1 = ro.oracle(c["Xs"], c["mask"], c["W"], c["b"], c["a"], [None, c["gs"][1]])
        assert ro.rel_err(emb.weight.grad.cpu().numpy(), want1["dW"]) <= tol(ref_err)["dW"]
        assert ro.rel_err(att.weight.grad.cpu().numpy().reshape(-1), want1["da"]) <= tol(ref_err)["da"]


def test_module_mask_is_cached_by_identity_and_version(dev, monkeypatch):
    _, patched = _standin(dev, 2)
    monkeypatch.setenv("GNNRAG_HIP_REL_TEXT", "1")
    patch = patched.get_rel_feature.__self__
    with torch.no_grad():
        a = patched.get_rel_feature()
        m0 = patch.mask
        patched.get_rel_feature()
        assert patch.mask is m0
        patched.rel_texts[0, 0] = ro.PAD                                  # in place: the version moves
        b = patched.get_rel_feature()
        assert patch.mask is not m0 and not torch.equal(a[0][0], b[0][0])
        patched.rel_texts = patched.rel_texts.clone()
        m1 = patch.mask
        patched.get_rel_feature()
        assert patch.mask is not m1 and torch.equal(patch.mask, m1)


def test_module_under_the_cache_runs_once_per_parameter_version(dev, monkeypatch):
    from gnnrag_amd import install, ops
    _, patched = _standin(dev, 2)
    install.cache_rel_features(patched)
    monkeypatch.setenv("GNNRAG_HIP_REL_TEXT", "1")
    calls = []
    fwd0 = ops.rel_text_pool
    monkeypatch.setattr(ops, "rel_text_pool", lambda *a, **k: (calls.append(1), fwd0(*a, **k))[1])
    patched.eval()
    with torch.no_grad():
        a = patched.get_rel_feature()
        b = patched.get_rel_feature()
        assert len(calls) == 1 and a[0] is b[0]
        patched.instruction.question_emb.bias.add_(0.5)
        c = patched.get_rel_feature()
        assert len(calls) == 2 and not torch.equal(c[0], a[0])
        patched.get_rel_feature()
    assert len(calls) == 2 and patched.calls == 0
