"""The concatenated update under dropout, host side: the float64 oracle of the GPU tests (tests/update_drop_oracle.py) equals
torch's float64 autograd of the expression written out and its case generator keeps its promises; the entry points are
declared in gnnrag.h and in the binding (additive to ABI 16) and answer the argument, limit and workspace rules before they
touch a device; ``gnnrag_dense_form`` names the kernel forms the new entries take at the shapes of the GPU tests;
``GNNRAG_HIP_UPDATE_DROP_TRAIN`` is read at every call, defaults to off, and leaves a layer on CPU tensors on the torch form."""
import os
import re

import numpy as np
import pytest
import torch

import update_drop_oracle as uo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_F64 = 1e-12
# (BN, D, I) of tests/test_gpu_update_drop.py
SHAPES = [(1, 4, 1), (70, 52, 2), (130, 68, 1), (260, 200, 3), (33, 212, 1), (32769, 4, 1), (131073, 4, 1)]


# -- the oracle ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.0, 0.2, 0.5])
def test_oracle_against_float64_autograd(p):
    BN, D, I = 9, 4, 2
    c = uo.case(BN, D, I, p, seed=3)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)      # noqa: E731
    h, agg, W, b = t(c["h"]), t(c["agg"]), t(c["W"]), t(c["b"])
    x = torch.cat([h, agg], dim=1)
    if c["keep"] is not None:
        x = x * torch.tensor(c["keep"].astype(np.float64) * float(np.float32(c["scale"])))
    pre = x @ W.T + b
    (pre * torch.tensor(c["g_pre"].astype(np.float64))).sum().backward()
    want_pre = uo.forward(c["h"], c["agg"], c["keep"], c["scale"], c["W"], c["b"])
    got = uo.backward(c["g_pre"], c["h"], c["agg"], c["keep"], c["scale"], c["W"])
    # the oracle rounds x * scale to fp32 (as the library does), autograd's float64 product does not: 2^-24 relative
    tol = TOL_F64 if p in (0.0, 0.5) else 2.0 ** -23 * 40
    assert np.abs(want_pre - pre.detach().numpy()).max() <= tol
    assert np.abs(got["g_h"] - h.grad.numpy()).max() <= TOL_F64
    assert np.abs(got["g_agg"] - agg.grad.numpy()).max() <= TOL_F64
    assert np.abs(got["dW"] - W.grad.numpy()).max() <= tol
    assert np.abs(got["db"] - b.grad.numpy()).max() <= TOL_F64


@pytest.mark.parametrize("BN,D,I", SHAPES[:5])
def test_case_generator_keeps_its_promises(BN, D, I):
    K = (2 * I + 1) * D
    c0 = uo.case(BN, D, I, 0.0)
    assert c0["keep"] is None and c0["scale"] == 1.0
    for p in (0.2, 0.5):
        c = uo.case(BN, D, I, p)
        keep = c["keep"]
        assert keep.dtype == np.uint8 and keep.shape == (BN, K) and set(np.unique(keep)) <= {0, 1}
        assert c["scale"] == float(np.float32(1) / np.float32(1 - p))
        assert not keep[0].any()                                         # a row with every element dropped
        if BN >= 2:
            assert keep[BN - 1].all()                                    # a row with none dropped
        if BN >= 3:
            assert not keep[BN // 2].any() and 0 < keep.mean() < 1
        xd = uo.xd_f32(c["h"], c["agg"], keep, c["scale"])
        assert xd.dtype == np.float32 and not xd[0].any() and not np.signbit(xd[0]).any()      # +0, not -0
    e = uo.case(BN, D, I, 0.5, exact=True)
    for k in ("h", "agg", "W", "b", "g_pre"):
        assert np.array_equal(e[k], np.round(e[k])) and np.abs(e[k]).max() <= 3
    assert e["scale"] == 2.0


# -- the entry points ------------------------------------------------------------------------------------------------------

SYMBOLS = {"gnnrag_update_drop_train": 12, "gnnrag_update_drop_backward_workspace_bytes": 3, "gnnrag_update_drop_backward": 17}


def test_header_binding_and_python_layers_declare_the_entries():
    from gnnrag_amd import _lib, autograd, ops
    from gnnrag_amd.modules.kg_reasoning.reasongnn import ReasonGNNLayer
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gnnrag.h")).read(), flags=re.S)
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "gnnrag.h does not declare " + name
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    assert re.search(r"#define\s+GNNRAG_ABI_VERSION\s+16\b", src) and _lib.ABI_VERSION == 16
    for key, macro in (("update_drop", "GNNRAG_DENSE_ENTRY_UPDATE_DROP"), ("update_drop_dx", "GNNRAG_DENSE_ENTRY_UPDATE_DROP_DX"),
                       ("update_drop_dw", "GNNRAG_DENSE_ENTRY_UPDATE_DROP_DW")):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, ops.DENSE_ENTRIES[key]), src), macro
    assert re.search(r"#define\s+GNNRAG_DENSE_GEMM_TN\s+%d\b" % ops.DENSE_GEMM_TN, src)
    # the older entries keep their ids
    assert [ops.DENSE_ENTRIES[k] for k in ("linear", "linear_pair", "update_score", "update_score_fused")] == [0, 1, 2, 3]
    for fn in (ops.update_drop_train, ops.update_drop_backward, ops.update_drop_supported, autograd.UpdateDropFn.apply,
               ReasonGNNLayer._update_drop, ReasonGNNLayer._draw_update_keep):
        assert callable(fn)
    ok = ops.update_drop_supported
    assert ok(4, 1) and ok(200, 3) and ok(212, 1) and not ok(50, 2) and not ok(0, 1) and not ok(4, 0) and not ok(1 << 29, 2)


@pytest.fixture(scope="module")
def lib():
    from gnnrag_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.gnnrag_abi_version() == 16
    return lib


A = 4096            # a dummy 16-byte aligned address


def _train(lib, BN=5, D=4, I=1, math=0, **v):
    a = dict(h=A, agg=A, keep=A, W=A, b=A, pre=A)
    a.update(v)
    return lib.gnnrag_update_drop_train(a["h"], a["agg"], a["keep"], 1.25, a["W"], a["b"], BN, D, I, a["pre"], math, None)


def _backward(lib, BN=5, D=4, I=1, math=0, ws=A, ws_bytes=0, **v):
    a = dict(g_pre=A, h=A, agg=A, keep=A, W=A, g_h=A, g_agg=A, dW=A, db=A)
    a.update(v)
    return lib.gnnrag_update_drop_backward(a["g_pre"], a["h"], a["agg"], a["keep"], 1.25, a["W"], BN, D, I, a["g_h"],
                                           a["g_agg"], a["dW"], a["db"], ws, ws_bytes, math, None)


def test_bad_arguments_and_limits_are_answered_before_anything_is_launched(lib):
    """Every pointer is a dummy non-NULL address and there is no device here: each answer comes from the argument checks (a
    call that passed them would fault on the dummy addresses, so every call below is one that must not pass)."""
    for k in ("h", "agg", "W", "b", "pre"):
        assert _train(lib, **{k: None}) == -1, k
    assert _train(lib, BN=0) == -1 and _train(lib, D=0) == -1 and _train(lib, I=0) == -1 and _train(lib, BN=-3) == -1
    assert _train(lib, math=7) == -1
    # limits: D % 4, 16-byte aligned float operands, 4-byte aligned keep, BN < 2^31
    assert _train(lib, D=6) == -2 and _train(lib, D=50, I=2) == -2
    for k in ("h", "agg", "W", "pre"):
        assert _train(lib, **{k: A + 4}) == -2, k
    assert _train(lib, keep=A + 2) == -2 and _train(lib, keep=A + 1) == -2
    assert _train(lib, BN=1 << 31) == -2
    assert _train(lib, keep=None, D=6) == -2                                   # the optional one is optional
    # BADARG is answered first
    assert _train(lib, h=None, D=6) == -1

    need = lib.gnnrag_update_drop_backward_workspace_bytes(5, 4, 1)
    assert need > 0
    for k in ("g_pre",):
        assert _backward(lib, ws_bytes=need, **{k: None}) == -1, k
    assert _backward(lib, ws_bytes=need, g_h=None, g_agg=None, dW=None, db=None) == -1            # nothing wanted
    assert _backward(lib, ws_bytes=need, W=None) == -1 and _backward(lib, ws_bytes=need, h=None) == -1
    assert _backward(lib, ws_bytes=need, agg=None) == -1
    assert _backward(lib, ws_bytes=need, BN=0) == -1 and _backward(lib, ws_bytes=need, D=-4) == -1
    assert _backward(lib, ws_bytes=need, I=0) == -1 and _backward(lib, ws_bytes=need, math=-1) == -1
    assert _backward(lib, ws_bytes=1 << 30, D=6) == -2 and _backward(lib, ws_bytes=1 << 30, BN=1 << 31) == -2
    for k in ("g_pre", "h", "agg", "W", "g_h", "g_agg", "dW"):
        assert _backward(lib, ws_bytes=need, **{k: A + 8}) == -2, k
    assert _backward(lib, ws_bytes=need, keep=A + 2) == -2 and _backward(lib, ws=A + 4, ws_bytes=need) == -2
    assert _backward(lib, ws=None, ws_bytes=need) == -3 and _backward(lib, ws_bytes=need - 1) == -3
    assert _backward(lib, ws_bytes=0, keep=None, g_h=None, g_agg=None, dW=None) == -3               # db alone, too


def test_workspace_size(lib):
    """The transposed weight [K, D], gnnrag_gemm_tn's chunk partials for (BN, D, K) and 176 partial rows of db, each rounded up
    to 256 bytes; 0 outside the limits."""
    up = lambda n: (n + 255) // 256 * 256                                      # noqa: E731
    for BN, D, I in SHAPES + [(32000, 200, 3)]:
        K = (2 * I + 1) * D
        tn = lib.gnnrag_gemm_tn_workspace_bytes(BN, D, K)
        assert tn >= D * K * 4 and tn % (D * K * 4) == 0
        assert lib.gnnrag_update_drop_backward_workspace_bytes(BN, D, I) == up(K * D * 4) + up(tn) + up(176 * D * 4), (BN, D, I)
    for BN, D, I in ((0, 4, 1), (5, 0, 1), (5, 4, 0), (5, 6, 1), (1 << 31, 4, 1), (-1, 4, 1), (5, 1 << 29, 2)):
        assert lib.gnnrag_update_drop_backward_workspace_bytes(BN, D, I) == 0, (BN, D, I)
    assert lib.gnnrag_update_drop_backward_workspace_bytes((1 << 31) - 1, 4, 1) > 0


def test_the_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    from gnnrag_amd import _lib, ops
    c = uo.case(3, 4, 1, 0.5)
    t = {k: (v if v is None or isinstance(v, float) else torch.from_numpy(v)) for k, v in c.items()}
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.update_drop_train(t["h"], t["agg"], t["keep"], c["scale"], t["W"], t["b"])
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.update_drop_backward(t["g_pre"], t["h"], t["agg"], t["keep"], c["scale"], t["W"])


# -- which kernels the new entries run -------------------------------------------------------------------------------------

# (BN, D, I) -> nt of the forward's blocks, (mt, nw)
FORMS = {(1, 4, 1): ([4], (1, 4)), (70, 52, 2): ([4], (1, 4)), (130, 68, 1): ([8], (1, 4)), (260, 200, 3): ([13], (1, 4)),
         (33, 212, 1): ([13, 4], (1, 4)), (32769, 4, 1): ([4], (1, 8)), (131073, 4, 1): ([4], (2, 4))}


def _nt(ncol):
    return 4 if ncol <= 64 else 8 if ncol <= 128 else 13


@pytest.mark.parametrize("math", [0, 1, 2])
def test_dense_form_names_the_kernels_of_the_new_entries(lib, math):
    from gnnrag_amd import ops
    seen = set()
    for (BN, D, I), (nts, (mt, nw)) in FORMS.items():
        # forward: k_gemm_f32<NT, MT, V4, EPI_LINEAR, AMODE_DROP, MATH, NW>, one launch per 208 columns of D
        for blk, nt in enumerate(nts):
            f = ops.dense_form("update_drop", BN, D, I, math=math, block=blk)
            assert f.family == f.block_family == ops.DENSE_KTILED and f.launches == len(nts) == (D + 207) // 208
            assert (f.epi, f.nt, f.mt, f.nw, f.v4, f.v4out, f.n0) == (ops.DENSE_EPI_LINEAR, nt, mt, nw, 1, 1, 208 * blk)
            assert f.math == (math != 0)
            seen.add((f.nt, f.mt, f.nw, f.math))
        # input gradient: EPI_KEEP, the blocks of g_h [BN, D] then those of g_agg [BN, 2 I D]
        nb_h, nb_agg = (D + 207) // 208, (2 * I * D + 207) // 208
        cols = [min(208, D - 208 * j) for j in range(nb_h)] + [min(208, 2 * I * D - 208 * j) for j in range(nb_agg)]
        for blk, ncol in enumerate(cols):
            f = ops.dense_form("update_drop_dx", BN, D, I, math=math, block=blk)
            assert f.family == ops.DENSE_KTILED and f.launches == nb_h + nb_agg
            assert (f.epi, f.nt, f.mt, f.nw, f.v4, f.v4out) == (ops.DENSE_EPI_KEEP, _nt(ncol), mt, nw, 1, 1), (BN, D, I, blk)
            assert f.n0 == 208 * (blk if blk < nb_h else blk - nb_h) and f.math == (math != 0)
            seen.add((f.nt, f.mt, f.nw, f.math))
        f = ops.dense_form("update_drop_dw", BN, D, I, math=math)
        assert f.family == f.block_family == ops.DENSE_GEMM_TN and f.launches == 1
        with pytest.raises(ops._lib.GnnragError):
            ops.dense_form("update_drop", BN, D, I, math=math, block=len(nts))
        with pytest.raises(ops._lib.GnnragError):
            ops.dense_form("update_drop_dx", BN, D, I, math=math, block=len(cols))
        with pytest.raises(ops._lib.GnnragError):
            ops.dense_form("update_drop_dw", BN, D, I, math=math, block=1)
    # every value of each template argument the dispatch can choose is among the test shapes: the three column-tile counts,
    # the three (MT, NW) tile shapes
    m = int(math != 0)
    assert {s[0] for s in seen} == {4, 8, 13} and {s[1:3] for s in seen} == {(1, 4), (1, 8), (2, 4)}
    assert {s[3] for s in seen} == {m}
    assert ops.dense_form("update_drop_dx", 260, 200, 3, math=math).launches == 7            # the trainer's K = 1400
    # outside the limits nothing is launched
    for entry in ("update_drop", "update_drop_dx", "update_drop_dw"):
        assert ops.dense_form(entry, 70, 50, 2, math=math).family == ops.DENSE_NONE
        assert ops.dense_form(entry, 70, 52, 2, math=math, misaligned=ops.DENSE_MISALIGNED_A).family == ops.DENSE_NONE
    # the row thresholds between the three tile shapes (gemm_form: 128-row tiles against 512 slots)
    for BN, want in ((32768, (1, 4)), (32769, (1, 8)), (65536, (1, 8)), (65537, (1, 4)), (98176, (1, 4)), (98177, (1, 8)),
                     (130944, (1, 8)), (130945, (2, 4))):
        f = ops.dense_form("update_drop", BN, 4, 1, math=math)
        assert (f.mt, f.nw) == want, BN


# -- the module layer ------------------------------------------------------------------------------------------------------

class _Plan:
    rel_total = 0


def _fake_aggregate(plan, dist, ins, T_fwd, T_inv):
    """Stands in for AggregateFn.apply (a HIP call): any differentiable [B*N, 2 I D] function of the same inputs."""
    B, I, D = ins.shape
    N = dist.shape[1]
    parts = []
    for i in range(I):
        for T in (T_fwd, T_inv):
            parts.append(dist.reshape(B, N, 1) * (ins[:, i] * T[i % T.shape[0]]).reshape(B, 1, D))
    return torch.cat(parts, dim=2).reshape(B * N, 2 * I * D)


def test_the_switch_defaults_to_off_is_read_per_call_and_leaves_cpu_tensors_on_the_torch_form(monkeypatch):
    from gnnrag_amd import ops
    from gnnrag_amd.modules.kg_reasoning import reasongnn as rg
    D, I, R, B, N, p = 8, 2, 5, 3, 6, 0.2
    torch.manual_seed(4)
    args = dict(use_cuda=False, normalized_gnn=False, num_ins=I, num_gnn=1, pos_emb=False, linear_dropout=p)
    layer = rg.ReasonGNNLayer(args, 1000, R, D, "bfs").train()
    g = torch.Generator().manual_seed(9)
    layer.batch_size, layer.max_local_entity, layer.plan = B, N, _Plan()
    layer.rel_features = torch.randn(R, D, generator=g)
    layer.rel_features_inv = torch.randn(R, D, generator=g)
    layer.local_entity_mask = (torch.rand(B, N, generator=g) < 0.7).float()
    layer.possible_cand = []
    monkeypatch.setattr(rg.AggregateFn, "apply", staticmethod(_fake_aggregate))

    def no_library(*a, **k):
        raise AssertionError("the library was called on CPU tensors")
    monkeypatch.setattr(ops, "update_drop_train", no_library)
    looks = []
    inner = rg.ReasonGNNLayer._update_drop

    def spy(self, *a, **k):
        got = inner(self, *a, **k)
        looks.append((os.environ.get("GNNRAG_HIP_UPDATE_DROP_TRAIN"), got is None))
        return got
    monkeypatch.setattr(rg.ReasonGNNLayer, "_update_drop", spy)
    h0 = torch.randn(B, N, D, generator=g)
    dist0 = torch.softmax(torch.randn(B, N, generator=g), dim=1)
    ins = torch.randn(B, I, D, generator=g)

    def run():
        layer.zero_grad(set_to_none=True)
        layer.local_entity_emb = h0.clone().requires_grad_(True)
        torch.manual_seed(21)                                   # the same dropout draws in every run
        dist, h = layer(dist0, ins, step=0)
        ((dist * dist).sum() + (h * h).sum()).backward()
        return [dist.detach(), h.detach()] + [q.grad for q in layer.parameters()]

    outs = []
    for value in (None, "0", "1", None):
        if value is None:
            monkeypatch.delenv("GNNRAG_HIP_UPDATE_DROP_TRAIN", raising=False)
        else:
            monkeypatch.setenv("GNNRAG_HIP_UPDATE_DROP_TRAIN", value)
        outs.append(run())
    for got in outs[1:]:
        for x, y in zip(got, outs[0]):
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y))
    # CPU tensors never reach the native branch (`native` is false): the switch is not even looked at
    assert looks == []
    # on the native branch it is looked at once per call, and only "1" switches it on
    # (no GPU here: the method itself)
    agg = torch.zeros(B * N, 2 * I * D)
    for value, want in ((None, True), ("0", True), ("1", True)):     # "1" on CPU tensors: not eligible either
        if value is None:
            monkeypatch.delenv("GNNRAG_HIP_UPDATE_DROP_TRAIN", raising=False)
        else:
            monkeypatch.setenv("GNNRAG_HIP_UPDATE_DROP_TRAIN", value)
        assert (layer._update_drop(agg, layer.e2e_linear0) is None) == want
    assert looks == [(None, True), ("0", True), ("1", True)]
