"""The training loss and the batch metrics, host side: the float64 loss oracle and the plain-Python restatement of the metrics
(tests/train_tail_oracle.py) reproduce what the live reference recorded (tests/golden/train_tail_ref.npz) - metrics, argmax
and counts exactly, loss and d_pred within 2e-6; the entry points are declared in gnnrag.h and in the binding (additive to
ABI 16) and refuse bad arguments before they touch a device; ``GNNRAG_HIP_LOSS_METRICS`` is read at every call, defaults to
off, and - unset or set - leaves a model on CPU tensors the wrapped methods' results bit for bit."""
import copy
import inspect
import os
import re

import numpy as np
import pytest
import torch

import train_tail_oracle as to

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_FIXTURE = 2e-6


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "train_tail_ref.npz"))


def _rec(golden, tag):
    return {k.split(".", 1)[1]: golden[k] for k in golden.files if k.startswith(tag + ".")}


@pytest.mark.parametrize("tag", list(to.FIXTURE_CASES))
def test_oracle_reproduces_the_recorded_reference(golden, tag):
    r = _rec(golden, tag)
    B, N, seed, eps = to.FIXTURE_CASES[tag]
    c = to.case(B, N, seed, eps)
    for k in ("pred", "answer", "teacher", "label_valid", "seed", "local_entity"):
        assert np.array_equal(c[k], r[k]) and c[k].dtype == r[k].dtype, k        # the generator still makes the recorded inputs
    assert float(r["eps"]) == eps and int(r["pad_id"]) == c["pad_id"] and r["g"] == c["g"]
    loss, d, _, _ = to.loss_and_grad(r["pred"], r["teacher"], r["label_valid"], r["g"])
    e_loss = abs(float(r["loss"]) - loss) / abs(loss)
    e_d = float(np.abs(r["d_pred"] - d).max() / np.abs(d).max())
    print("%s: loss %.3e  d_pred %.3e (recorded %.3e / %.3e)" % (tag, e_loss, e_d, r["err_loss"], r["err_d_pred"]))
    assert e_loss <= TOL_FIXTURE and e_d <= TOL_FIXTURE
    assert r["err_loss"] <= TOL_FIXTURE and r["err_d_pred"] <= TOL_FIXTURE
    assert not d[(r["teacher"] == 0) | (r["label_valid"] == 0).repeat(N, 1)].any()
    m = to.metrics(r["pred"], r["answer"], r["seed"], r["local_entity"], int(r["pad_id"]), float(r["eps"]))
    assert np.array_equal(m["pred"], r["argmax"])
    assert m["h1"].tobytes() == r["h1"].astype(np.float32).tobytes()
    assert m["f1"].tobytes() == r["f1"].astype(np.float32).tobytes()
    # the four counts against what f1_and_hits was given and returned with every question let through the gate
    assert np.array_equal(m["cnt"][:, 0], r["kept"]) and np.array_equal(m["cnt"][:, 3], r["n_ans"])
    assert np.array_equal(m["precision"], r["precision"]) and np.array_equal(m["recall"], r["recall"])
    assert np.array_equal(m["f1_raw"], r["f1_raw"])
    full = (m["cnt"][:, 3] > 0) & (m["cnt"][:, 1] > 0)
    assert np.array_equal(m["cnt"][full, 2] / m["cnt"][full, 1], r["precision"][full])


def test_the_fixture_holds_every_corner(golden):
    seen = set()
    for tag in to.FIXTURE_CASES:
        r = _rec(golden, tag)
        m = to.metrics(r["pred"], r["answer"], r["seed"], r["local_entity"], int(r["pad_id"]), float(r["eps"]))
        kept, n_ret, correct, n_ans = m["cnt"].T
        B, N = r["pred"].shape
        for b in range(B):
            top, hit = int(m["pred"][b]), m["h1"][b] == 1
            if r["label_valid"][b, 0] == 0 and not r["answer"][b].any():
                seen.add("no answers")
            if (r["local_entity"][b] == r["pad_id"]).all():
                seen.add("pads only")
            if hit and r["seed"][b, top] > 0 and n_ans[b] == 0:
                seen.add("seed answer, retrieved empty" if n_ret[b] == 0 else "seed answer, retrieved non-empty")
                assert m["f1"][b] == (1.0 if n_ret[b] == 0 else 0.0)
            if hit and n_ans[b] > 0 and kept[b] == 0:
                seen.add("nothing survives")
                assert m["f1"][b] == 0.0 and m["precision"][b] == 1.0 and m["recall"][b] == 0.0
            p = r["pred"][b]
            if (p == p[top]).sum() > 1:
                seen.add("tie at the argmax")
                assert top == int(np.flatnonzero(p == p[top])[0])
            order = sorted((j for j in range(N) if r["seed"][b, j] <= 0 and r["local_entity"][b, j] != r["pad_id"] and
                            not float(p[j]) < (1 - float(r["eps"])) / N), key=lambda j: -p[j])
            if any(p[order[i]] == p[order[i + 1]] for i in range(n_ret[b] - 1)):
                seen.add("tie in the prefix")
            if hit and kept[b] > 1 and n_ret[b] == kept[b]:
                total = 0.0
                for j in order:
                    total += float(p[j])
                seen.add("cut on the last kept slot" if total > float(r["eps"]) else "sum never exceeds eps")
            if (p == 0).any():
                seen.add("zeros in pred")
        seen.add("eps %.2f" % float(r["eps"]))
    want = {"no answers", "pads only", "seed answer, retrieved empty", "seed answer, retrieved non-empty", "nothing survives",
            "tie at the argmax", "tie in the prefix", "cut on the last kept slot", "sum never exceeds eps", "zeros in pred",
            "eps 0.95", "eps 0.30"}
    assert want <= seen, want - seen


# -- the entry points ------------------------------------------------------------------------------------------------------

SYMBOLS = {"gnnrag_kl_loss_workspace_bytes": 1, "gnnrag_kl_loss_train": 10, "gnnrag_kl_loss_backward": 9,
           "gnnrag_train_metrics": 13}


def test_header_binding_and_python_layers_declare_the_entry_points():
    from gnnrag_amd import _lib, autograd, install, ops
    from gnnrag_amd.modules import train_tail
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gnnrag.h")).read(), flags=re.S)
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "gnnrag.h does not declare " + name
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    assert re.search(r"#define\s+GNNRAG_ABI_VERSION\s+16\b", src) and _lib.ABI_VERSION == 16
    assert re.search(r"#define\s+GNNRAG_TRAIN_METRICS_MAX_N\s+16384\b", src) and ops.TRAIN_METRICS_MAX_N == 16384
    for fn in (ops.kl_loss_train, ops.kl_loss_backward, ops.train_metrics, ops.train_metrics_supported,
               autograd.KLLossFn.apply, train_tail.patch_loss_metrics, install.patch_loss_metrics):
        assert callable(fn)
    assert "train_tail.hip" in __import__("gnnrag_amd.build", fromlist=["SOURCES"]).SOURCES
    ok = ops.train_metrics_supported
    assert ok(1, 1) and ok(64, 2000) and ok(1, 16384) and not ok(1, 16385) and not ok(0, 5) and not ok(2, 0)
    assert inspect.getsource(install.swap).count("patch_loss_metrics(model)") == 2          # the ReaRev and the NSM branch


@pytest.fixture(scope="module")
def lib():
    from gnnrag_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.gnnrag_abi_version() == 16
    return lib


def _loss(lib, B=2, N=5, ws=4096, ws_bytes=1 << 20, **null):
    v = dict(pred=4096, teacher=4096, label_valid=4096, loss=4096, reserve=4096)
    v.update(null)
    return lib.gnnrag_kl_loss_train(v["pred"], v["teacher"], v["label_valid"], B, N, v["loss"], v["reserve"], ws, ws_bytes,
                                    None)


def _loss_bwd(lib, B=2, N=5, **null):
    v = dict(g_loss=4096, pred=4096, teacher=4096, label_valid=4096, reserve=4096, d_pred=4096)
    v.update(null)
    return lib.gnnrag_kl_loss_backward(v["g_loss"], v["pred"], v["teacher"], v["label_valid"], v["reserve"], B, N,
                                       v["d_pred"], None)


def _metrics(lib, B=2, N=5, **null):
    v = dict(pred=4096, answer=4096, seed=4096, local_entity=4096, out_pred=4096, h1=4096, f1=4096, cnt=4096)
    v.update(null)
    return lib.gnnrag_train_metrics(v["pred"], v["answer"], v["seed"], v["local_entity"], 77, 0.95, B, N, v["out_pred"],
                                    v["h1"], v["f1"], v["cnt"], None)


def test_bad_arguments_are_refused_before_anything_is_launched(lib):
    """Every pointer is a dummy non-NULL address and there is no device here: each answer comes from the argument checks (a
    call that passed them would fault on the dummy addresses, so every call below is one that must not pass)."""
    for k in ("pred", "teacher", "label_valid", "loss", "reserve"):
        assert _loss(lib, **{k: None}) == -1, k
    assert _loss(lib, B=0) == -1 and _loss(lib, B=-2) == -1 and _loss(lib, N=0) == -1 and _loss(lib, N=-1) == -1
    need = lib.gnnrag_kl_loss_workspace_bytes(2)
    assert need >= 2 * 4 and lib.gnnrag_kl_loss_workspace_bytes(0) == 0 and lib.gnnrag_kl_loss_workspace_bytes(-1) == 0
    assert lib.gnnrag_kl_loss_workspace_bytes(1000) >= 4000
    assert _loss(lib, ws=None) == -3 and _loss(lib, ws_bytes=need - 1) == -3 and _loss(lib, ws_bytes=0) == -3
    for k in ("g_loss", "pred", "teacher", "label_valid", "reserve", "d_pred"):
        assert _loss_bwd(lib, **{k: None}) == -1, k
    assert _loss_bwd(lib, B=0) == -1 and _loss_bwd(lib, N=0) == -1 and _loss_bwd(lib, B=-1, N=-1) == -1
    for k in ("pred", "answer", "seed", "local_entity", "out_pred", "h1", "f1", "cnt"):
        assert _metrics(lib, **{k: None}) == -1, k
    assert _metrics(lib, B=0) == -1 and _metrics(lib, N=0) == -1 and _metrics(lib, B=-5) == -1
    assert _metrics(lib, N=16385) == -2 and _metrics(lib, N=1 << 30) == -2
    assert _metrics(lib, N=16385, pred=None) == -1                           # a bad argument is named first


def _cpu_tensors(c):
    return {k: torch.from_numpy(v) for k, v in c.items() if isinstance(v, np.ndarray) and v.ndim}


def test_the_wrappers_refuse_cpu_tensors():
    from gnnrag_amd import _lib, ops
    c = to.case(2, 5)
    t = _cpu_tensors(c)
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.kl_loss_train(t["pred"], t["teacher"], t["label_valid"])
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.kl_loss_backward(torch.ones(1), t["pred"], t["teacher"], t["label_valid"], torch.ones(2))
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.train_metrics(t["pred"], t["answer"], t["seed"], t["local_entity"], c["pad_id"], c["eps"])


# -- the module layer ------------------------------------------------------------------------------------------------------

def test_the_switch_is_read_at_every_call_and_defaults_to_off(monkeypatch):
    from gnnrag_amd.modules import train_tail
    monkeypatch.delenv("GNNRAG_HIP_LOSS_METRICS", raising=False)
    assert train_tail.DEFAULT == "0" and not train_tail.enabled()
    monkeypatch.setenv("GNNRAG_HIP_LOSS_METRICS", "1")
    assert train_tail.enabled()
    monkeypatch.setenv("GNNRAG_HIP_LOSS_METRICS", "0")
    assert not train_tail.enabled()


def _run(model, t):
    pred = t["pred"].clone().requires_grad_(True)
    loss = model.calc_loss_label(curr_dist=pred, teacher_dist=t["teacher"], label_valid=t["label_valid"])
    loss.backward()
    h1, f1 = model.get_eval_metric(pred, t["answer"])
    return [x.detach().numpy().tobytes() for x in (loss, pred.grad, h1, f1)], loss


@pytest.mark.parametrize("loss_type", ["kl", "bce"])
def test_a_model_on_cpu_tensors_keeps_the_wrapped_methods_bit_for_bit(golden, monkeypatch, loss_type):
    from gnnrag_amd import ops
    from gnnrag_amd.modules.train_tail import patch_loss_metrics

    def no_library(*a, **k):
        raise AssertionError("the library was called for CPU tensors")

    for name in ("kl_loss_train", "kl_loss_backward", "train_metrics"):
        monkeypatch.setattr(ops, name, no_library)
    c = to.case(*to.FIXTURE_CASES["n64"])
    t = _cpu_tensors(c)
    monkeypatch.delenv("GNNRAG_HIP_LOSS_METRICS", raising=False)
    plain, loss = _run(to.StandIn(c, loss_type=loss_type), t)
    assert loss.dim() == 0
    if loss_type == "kl":                                  # the stand-in is the recorded reference
        r = _rec(golden, "n64")
        assert abs(float(loss.detach()) - float(r["loss"])) <= TOL_FIXTURE * abs(float(r["loss"]))
        assert plain[2] == r["h1"].tobytes() and plain[3] == r["f1"].tobytes()
    model = to.StandIn(c, loss_type=loss_type)
    assert patch_loss_metrics(model) is model and patch_loss_metrics(model) is model          # idempotent
    assert model.calc_loss_label.__self__ is model.get_eval_metric.__self__ is not model
    for value in (None, "0", "1"):
        if value is None:
            monkeypatch.delenv("GNNRAG_HIP_LOSS_METRICS", raising=False)
        else:
            monkeypatch.setenv("GNNRAG_HIP_LOSS_METRICS", value)
        before = dict(model.calls)
        got, _ = _run(model, t)
        assert got == plain, value
        assert model.calls == {"loss": before["loss"] + 1, "metric": before["metric"] + 1}
    twin = copy.deepcopy(model)                              # a deep copy patches for itself
    assert twin.calc_loss_label.__self__.model is twin and twin.calc_loss_label.__self__.orig_loss.__self__ is twin
    got, _ = _run(twin, t)
    assert got == plain and twin.calls["loss"] == model.calls["loss"] + 1
