"""The optimiser step, host side: the float64 oracle (tests/optim_oracle.py) equals ``torch.optim.Adam(foreach=False)`` +
``clip_grad_norm_`` on float64 CPU tensors; the entry points are declared in gnnrag.h, in the binding (additive to ABI 16), in
``build.SOURCES`` and in the Python layers, and refuse bad arguments and a short workspace before they touch a device;
``GNNRAG_HIP_OPTIM`` is read at every call and defaults to off; a patched optimiser on a CPU model is torch's own, bit for
bit, whatever the switch says; patching is idempotent, keeps ``LRScheduler`` and the step hooks working and leaves
``state_dict()`` as torch writes it."""
import copy
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import optim_oracle as oo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1,), (3,), (7, 5), (64,), (2, 3, 4), (33,)]


# -- the oracle ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm", [1.0, 100.0])
def test_oracle_equals_torch_in_float64(max_norm):
    """Three steps: total norm 3.0, 0.4, 0.7 (above max_norm = 1 in step 1, below it after; always below 100); two groups
    with different lr, weight_decay 0 and 0.01; an ExponentialLR step after step 1; parameter 2 has no gradient in step 2
    only (its step count then lags the others'); parameter 5 never has one and gets no state."""
    case = oo.make_case(SHAPES, none_at=((1, 2), (0, 5), (1, 5), (2, 5)))
    assert case["groups"][0]["lr"] != case["groups"][1]["lr"]
    assert {g["weight_decay"] for g in case["groups"]} == {0.0, 0.01}
    want = oo.run_oracle(case, max_norm, gamma_after={0: 0.5})
    got, params, opt = oo.run_torch(case, max_norm, dtype=torch.float64, gamma_after={0: 0.5})
    assert opt.param_groups[0]["lr"] == pytest.approx(0.5e-3)
    for k in range(3):
        assert abs(got[k][3] - want[k][3]) <= 1e-12 * want[k][3]
        assert (want[k][3] > max_norm) == (k == 0 and max_norm == 1.0)
        for name, a, b in zip("pmv", got[k][:3], want[k][:3]):
            for i, (x, y) in enumerate(zip(a, b)):
                assert (x is None) == (y is None), (k, name, i)
                if y is not None:
                    assert oo.rel_dev(x, y) <= 1e-12, (k, name, i)
    assert want[2][1][5] is None and params[5] not in opt.state
    assert opt.state[params[2]]["step"].item() == 2 and opt.state[params[0]]["step"].item() == 3


def test_oracle_clip_corners():
    g = [np.array([3.0, 4.0]), None, np.array([[12.0]])]
    total, coef, out = oo.AdamOracle.clip(g, 1.0)
    assert total == 13.0 and coef == 1.0 / (13.0 + 1e-6) and out[1] is None
    assert oo.AdamOracle.clip(g, 1e9)[1] == 1.0
    total, coef, _ = oo.AdamOracle.clip([np.array([np.nan, 1.0])], 1.0)
    assert total != total and coef != coef
    assert oo.AdamOracle.clip([np.array([np.inf, 1.0])], 1.0)[1] == 0.0


# -- the entry points ------------------------------------------------------------------------------------------------------

SYMBOLS = {"gnnrag_optim_workspace_bytes": 1, "gnnrag_grad_norm": 8, "gnnrag_adam_step": 5}


def test_header_binding_sources_and_python_layers_declare_the_entry_points():
    from gnnrag_amd import _lib, build, install, ops, optim
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gnnrag.h")).read(), flags=re.S)
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "gnnrag.h does not declare " + name
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    assert re.search(r"#define\s+GNNRAG_ABI_VERSION\s+16\b", src) and _lib.ABI_VERSION == 16
    assert re.search(r"#define\s+GNNRAG_OPTIM_CHUNK\s+4096\b", src) and ops.OPTIM_CHUNK == _lib.OPTIM_CHUNK == 4096
    assert "optim.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "optim.hip"))
    # the struct of the header, field for field, in the ctypes mirror and in the numpy mirror
    body = re.search(r"typedef struct gnnrag_optim_seg \{(.*?)\} gnnrag_optim_seg;", src, flags=re.S).group(1)
    fields = [f for decl in body.split(";") for f in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert fields == [n for n, _ in _lib.OptimSeg._fields_] == list(ops.OPTIM_SEG_DTYPE.names)
    assert ctypes.sizeof(_lib.OptimSeg) == ops.OPTIM_SEG_DTYPE.itemsize == ops.OPTIM_SEG_BYTES == 80
    for n, _ in _lib.OptimSeg._fields_:
        assert getattr(_lib.OptimSeg, n).offset == ops.OPTIM_SEG_DTYPE.fields[n][1], n
    for fn in (ops.grad_norm, ops.adam_step, ops.optim_chunks, optim.patch_adam, optim.patch_trainer, install.patch_trainer):
        assert callable(fn)
    assert ops.optim_chunks([1, 4096, 4097, 0, 8193]) == ([0, 1, 2, 4, 4], 7)
    run_ref = open(os.path.join(REPO, "tools", "run_reference.py")).read()
    assert "install.patch_trainer(self)" in run_ref and "optim_def" in run_ref


@pytest.fixture(scope="module")
def lib():
    from gnnrag_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.gnnrag_abi_version() == 16
    return lib


def _norm(lib, T=2, n_chunks=3, max_norm=1.0, ws=4096, ws_bytes=1 << 20, **null):
    v = dict(segs=4096, out2=4096)
    v.update(null)
    return lib.gnnrag_grad_norm(v["segs"], T, n_chunks, max_norm, v["out2"], ws, ws_bytes, None)


def _adam(lib, T=2, n_chunks=3, segs=4096, coef=4096):
    return lib.gnnrag_adam_step(segs, T, n_chunks, coef, None)


def test_bad_arguments_and_a_short_workspace_are_refused_before_anything_is_launched(lib):
    """Every pointer is a dummy non-NULL address and there is no device here: each answer comes from the argument checks (a
    call that passed them would fault on the dummy addresses, so every call below is one that must not pass)."""
    for k in ("segs", "out2"):
        assert _norm(lib, **{k: None}) == -1, k
    assert _norm(lib, T=0) == -1 and _norm(lib, T=-3) == -1 and _norm(lib, n_chunks=0) == -1 and _norm(lib, n_chunks=-1) == -1
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        assert _norm(lib, max_norm=bad) == -1, bad
    need = lib.gnnrag_optim_workspace_bytes(3)
    assert need >= 3 * 4 and lib.gnnrag_optim_workspace_bytes(0) == 0 and lib.gnnrag_optim_workspace_bytes(-5) == 0
    assert lib.gnnrag_optim_workspace_bytes(100000) >= 400000
    assert _norm(lib, ws=None) == -3 and _norm(lib, ws_bytes=need - 1) == -3 and _norm(lib, ws_bytes=0) == -3
    assert _norm(lib, ws=None, segs=None) == -1                              # a bad argument is named first
    assert _adam(lib, segs=None) == -1 and _adam(lib, T=0) == -1 and _adam(lib, T=-1) == -1
    assert _adam(lib, n_chunks=0) == -1 and _adam(lib, n_chunks=-7) == -1
    assert _adam(lib, segs=None, coef=None) == -1


def test_the_wrappers_refuse_cpu_tensors():
    from gnnrag_amd import _lib, ops
    table = torch.zeros(2 * ops.OPTIM_SEG_BYTES, dtype=torch.uint8)
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.grad_norm(table, 2, 2, 1.0)
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.adam_step(table, 2, 2)


# -- the Python layer ------------------------------------------------------------------------------------------------------

def test_the_switch_is_read_at_every_call_and_defaults_to_off(monkeypatch):
    from gnnrag_amd import optim
    monkeypatch.delenv("GNNRAG_HIP_OPTIM", raising=False)
    assert optim.DEFAULT == "0" and not optim.enabled()
    monkeypatch.setenv("GNNRAG_HIP_OPTIM", "1")
    assert optim.enabled()
    monkeypatch.setenv("GNNRAG_HIP_OPTIM", "0")
    assert not optim.enabled()


def _no_library(monkeypatch):
    from gnnrag_amd import ops

    def no_library(*a, **k):
        raise AssertionError("the library was called for CPU tensors")

    for name in ("grad_norm", "adam_step"):
        monkeypatch.setattr(ops, name, no_library)


def _bytes(snaps):
    return [[None if x is None else x.tobytes() for x in part] for s in snaps for part in s[:3]] + [s[3] for s in snaps]


@pytest.mark.parametrize("value", [None, "0", "1"])
def test_a_patched_optimiser_on_a_cpu_model_is_torchs_own_bit_for_bit(monkeypatch, value):
    from gnnrag_amd.optim import patch_adam
    _no_library(monkeypatch)
    case = oo.make_case(SHAPES, none_at=((1, 2),))
    monkeypatch.delenv("GNNRAG_HIP_OPTIM", raising=False)
    plain, _, plain_opt = oo.run_torch(case, 1.0)
    if value is not None:
        monkeypatch.setenv("GNNRAG_HIP_OPTIM", value)
    fused, _, opt = oo.run_torch(case, 1.0, fused=True, patch=patch_adam)
    assert _bytes(fused) == _bytes(plain)
    assert isinstance(opt, torch.optim.Adam) and type(opt) is type(plain_opt) and opt._gnnrag_optim.calls == 0
    stepped, _, _ = oo.run_torch(case, 1.0, patch=patch_adam)              # clip_grad_norm_ + the patched step()
    assert _bytes(stepped) == _bytes(plain)


def test_patching_is_idempotent_and_keeps_the_object():
    from gnnrag_amd.optim import patch_adam
    _, opt = oo.build_torch(oo.make_case(SHAPES))
    assert patch_adam(opt) is opt
    step, fused, state = opt.step, opt.clip_and_step, opt._gnnrag_optim
    assert patch_adam(opt) is opt and opt.step == step and opt.clip_and_step == fused and opt._gnnrag_optim is state
    assert step.__self__ is opt and fused.__self__ is opt
    with pytest.raises(TypeError):
        patch_adam(torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.1))


@pytest.mark.parametrize("scheduler_first", [True, False])
def test_no_scheduler_warning_and_hooks_run_once_each(monkeypatch, scheduler_first):
    from gnnrag_amd.optim import patch_adam
    monkeypatch.setenv("GNNRAG_HIP_OPTIM", "1")
    _no_library(monkeypatch)
    case = oo.make_case(SHAPES)
    params, opt = oo.build_torch(case)
    if scheduler_first:                                       # the reference's order: optim_def, then the patch
        sched = torch.optim.lr_scheduler.ExponentialLR(opt, 0.5)
        patch_adam(opt)
    else:
        patch_adam(opt)
        sched = torch.optim.lr_scheduler.ExponentialLR(opt, 0.5)
    assert sched.optimizer is opt
    seen = {"pre": 0, "post": 0}
    opt.register_step_pre_hook(lambda o, a, k: seen.__setitem__("pre", seen["pre"] + 1))
    opt.register_step_post_hook(lambda o, a, k: seen.__setitem__("post", seen["post"] + 1))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for k in range(2):
            oo.set_grads(params, case["grads"][k])
            if k == 0:
                opt.clip_and_step(params, 1.0)
            else:
                opt.step()
            sched.step()
            assert seen == {"pre": k + 1, "post": k + 1}
    assert opt.param_groups[0]["lr"] == pytest.approx(0.25e-3)


def test_state_dict_is_torchs(monkeypatch):
    from gnnrag_amd.optim import patch_adam
    monkeypatch.setenv("GNNRAG_HIP_OPTIM", "1")
    case = oo.make_case(SHAPES, none_at=((0, 1), (1, 1), (2, 1)))
    _, _, plain = oo.run_torch(case, 1.0)
    _, _, opt = oo.run_torch(case, 1.0, fused=True, patch=patch_adam)
    a, b = plain.state_dict(), opt.state_dict()
    assert a["param_groups"] == b["param_groups"] and a["state"].keys() == b["state"].keys() and 1 not in b["state"]
    for i in a["state"]:
        assert a["state"][i].keys() == b["state"][i].keys()
        for k, x in a["state"][i].items():
            y = b["state"][i][k]
            assert x.dtype == y.dtype and x.device == y.device and x.shape == y.shape and torch.equal(x, y), (i, k)
    twin = copy.deepcopy(opt.state_dict())
    _, fresh = oo.build_torch(case)
    fresh.load_state_dict(twin)                               # a patched optimiser's checkpoint loads into a plain one
    assert fresh.state_dict()["state"].keys() == a["state"].keys()
