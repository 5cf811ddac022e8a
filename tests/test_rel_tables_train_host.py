"""Backward of the relation tables of the fused training form, host side: the float64 oracle of the GPU tests
(tests/rel_tables_grad_oracle.py) equals torch's float64 autograd of the per-fact reference expression on a hand-made row
list and keeps torch's gate at a == 0; the two entry points are declared in gnnrag.h and in the binding (additive to ABI 16),
exported by the library, and answer the argument, limit and workspace rules before they touch a device; ``gnnrag_dense_form``
names the products of the backward; ``GNNRAG_HIP_REL_TABLES_TRAIN`` is read at every call and defaults to off."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import rel_tables_grad_oracle as ro

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_F64 = 1e-12
# relation 2 is used by six of the eight questions, relation 4 by none, question 6 has no rows
ROWS = np.array([(0, 0), (0, 2), (1, 2), (1, 3), (2, 1), (2, 2), (3, 2), (3, 5), (4, 2), (5, 0), (5, 2), (5, 5), (7, 1),
                 (7, 3)], dtype=np.int64)
R1, B = 6, 8


# -- the oracle ------------------------------------------------------------------------------------------------------------

def _autograd(rows, c, I, D):
    """The per-fact expression of the reference (reasongnn.py:71-79 / :98-105: index_select of the relation rows and of the
    facts' questions, product, relu) with one "fact" per compact row, e2e_linear's column blocks applied to it."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)      # noqa: E731
    T_fwd, T_inv, ins, W = t(c["T_fwd"]), t(c["T_inv"]), t(c["ins"]), t(c["W"])
    batch_ids, batch_rels = torch.from_numpy(rows[:, 0]), torch.from_numpy(rows[:, 1])
    P = []
    for d, T in enumerate((T_fwd, T_inv)):
        acc = 0.0
        for i in range(I):
            fact_rel = torch.index_select(T, 0, batch_rels)
            fact_query = torch.index_select(ins[:, i], 0, batch_ids)
            fact_val = torch.relu(fact_rel * fact_query)
            acc = acc + fact_val @ W[:, (1 + 2 * i + d) * D:(2 + 2 * i + d) * D].T
        P.append(acc)
    P = torch.stack(P)
    (P * torch.tensor(c["g_P"].astype(np.float64))).sum().backward()
    return P.detach().numpy(), dict(g_T_fwd=T_fwd.grad.numpy(), g_T_inv=T_inv.grad.numpy(), g_ins=ins.grad.numpy(),
                                    g_W=W.grad.numpy())


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("D,I", [(4, 1), (8, 3)])
def test_oracle_against_float64_autograd_of_the_per_fact_expression(D, I, exact):
    c = ro.case(ROWS, R1, B, D, I, seed=5, exact=exact)
    want_P, want = _autograd(ROWS, c, I, D)
    got = ro.backward(ROWS, R1, B, c["T_fwd"], c["T_inv"], c["ins"], c["W"], c["g_P"])
    # the oracle rounds T * ins to fp32 (as the library does), autograd's float64 product does not: 2^-24 relative
    tol = TOL_F64 if exact else 2.0 ** -23 * 40
    assert np.abs(ro.forward(ROWS, c["T_fwd"], c["T_inv"], c["ins"], c["W"]) - want_P).max() <= tol
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.abs(got[k] - want[k]).max() <= (tol if k == "g_W" else TOL_F64), k
    # the unused relation, the question without rows, the self block
    assert not got["g_T_fwd"][4].any() and not got["g_T_inv"][4].any() and not got["g_ins"][6].any()
    assert not got["g_W"][:, :D].any() and got["g_W"][:, D:].any()
    assert got["g_T_fwd"][2].any() and got["g_ins"][7].any()
    if exact:
        c = ro.case(ROWS, R1, B, D, I, seed=5, exact=True)
        for v in c.values():
            assert v.dtype == np.float32 and np.array_equal(v, np.round(v)) and np.abs(v).max() <= 3
        a = c["T_fwd"][ROWS[:, 1]][:, None, :] * c["ins"][ROWS[:, 0]]
        assert (a == 0).mean() > 0.1               # the gate meets many exact zeros (13 / 49 of the products on average)
        assert ro.largest_sum(ROWS, R1, B, c) < 2 ** 24


def test_the_gate_is_torchs_relu_rule_at_zero():
    """a == +0, a == -0 and a < 0 pass nothing, in the oracle as in torch's relu."""
    rows = np.array([(0, 0)], dtype=np.int64)
    c = dict(T_fwd=np.array([[0.0, 1.0, -1.0, 2.0, 2.0]], np.float32), T_inv=np.array([[1.0, 1.0, 1.0, 1.0, 1.0]], np.float32),
             ins=np.array([[[5.0, 0.0, 3.0, -0.0, 1.0]]], np.float32), W=np.ones((5, 15), np.float32),
             g_P=np.ones((2, 1, 5), np.float32))
    got = ro.backward(rows, 1, 1, c["T_fwd"], c["T_inv"], c["ins"], c["W"], c["g_P"])
    _, want = _autograd(rows, c, 1, 5)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["g_T_fwd"][0], [0, 0, 0, 0, 5])                # only a = 2 * 1 > 0 passes
    assert np.array_equal(got["g_T_inv"][0], [25, 0, 15, 0, 5])              # a = ins: 5, 0, 3, -0, 1
    assert np.array_equal(got["g_ins"][0, 0], [5, 0, 5, 0, 15])
    assert not np.signbit(got["g_ins"]).any() and not np.signbit(got["g_T_fwd"]).any()


# -- the entry points ------------------------------------------------------------------------------------------------------

SYMBOLS = {"gnnrag_relation_tables_backward_workspace_bytes": 3, "gnnrag_relation_tables_backward": 16}


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
    for key, macro in (("rel_tables_dx", "GNNRAG_DENSE_ENTRY_REL_TABLES_DX"), ("rel_tables_dw", "GNNRAG_DENSE_ENTRY_REL_TABLES_DW")):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, ops.DENSE_ENTRIES[key]), src), macro
    # the older entries keep their ids
    assert [ops.DENSE_ENTRIES[k] for k in ("linear", "linear_pair", "update_score", "update_score_fused", "update_drop",
                                           "update_drop_dx", "update_drop_dw")] == list(range(7))
    for fn in (ops.relation_tables_backward, ops.relation_tables_backward_supported, autograd.RelationTablesFn.apply,
               autograd.relation_tables_dense, ReasonGNNLayer._relation_tables):
        assert callable(fn)
    ok = ops.relation_tables_backward_supported
    assert ok(4, 1) and ok(200, 2) and ok(1024, 8) and not ok(50, 2) and not ok(1028, 1) and not ok(0, 1) and not ok(4, 0)


@pytest.fixture(scope="module")
def lib():
    from gnnrag_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.gnnrag_abi_version() == 16
    return lib


def test_the_library_exports_the_entries(lib):
    for name in SYMBOLS:
        assert getattr(lib, name) is not None, name


A = 4096            # a dummy 16-byte aligned address


def _csr(rel_total=5, B=2, R1=3):
    from gnnrag_amd import _lib
    c = _lib.CsrStruct()
    c.B, c.N, c.R1, c.rel_total = B, 8, R1, rel_total
    return c


def _backward(lib, csr="default", D=4, I=1, math=0, ws=A, ws_bytes=0, **v):
    a = dict(T_fwd=A, T_inv=A, ins=A, W=A, g_P=A, g_T_fwd=A, g_T_inv=A, g_ins=A, g_W=A)
    a.update(v)
    c = _csr() if isinstance(csr, str) else csr
    return lib.gnnrag_relation_tables_backward(None if c is None else ctypes.byref(c), a["T_fwd"], a["T_inv"], a["ins"], a["W"],
                                               a["g_P"], a["g_T_fwd"], a["g_T_inv"], a["g_ins"], a["g_W"], D, I, math, ws,
                                               ws_bytes, None)


def test_bad_arguments_and_limits_are_answered_before_anything_is_launched(lib):
    """Every pointer is a dummy non-NULL address and there is no device here: each answer comes from the argument checks (a
    call that passed them would fault on the dummy addresses, so every call below is one that must not pass)."""
    need = lib.gnnrag_relation_tables_backward_workspace_bytes(ctypes.byref(_csr()), 4, 1)
    assert need > 0
    assert _backward(lib, csr=None, ws_bytes=need) == -1
    for k in ("T_fwd", "T_inv", "ins", "W", "g_P"):
        assert _backward(lib, ws_bytes=need, **{k: None}) == -1, k
    assert _backward(lib, ws_bytes=need, g_T_fwd=None, g_T_inv=None, g_ins=None, g_W=None) == -1      # nothing wanted
    assert _backward(lib, ws_bytes=need, D=0) == -1 and _backward(lib, ws_bytes=need, I=0) == -1
    assert _backward(lib, ws_bytes=need, math=7) == -1 and _backward(lib, ws_bytes=need, csr=_csr(rel_total=-1)) == -1
    # limits: D % 4, D <= 1024, 16-byte aligned operands
    assert _backward(lib, ws_bytes=1 << 30, D=6) == -2 and _backward(lib, ws_bytes=1 << 30, D=50, I=2) == -2
    assert _backward(lib, ws_bytes=1 << 40, D=1028) == -2
    for k in ("T_fwd", "T_inv", "ins", "W", "g_P", "g_T_fwd", "g_T_inv", "g_ins", "g_W"):
        assert _backward(lib, ws_bytes=need, **{k: A + 8}) == -2, k
    assert _backward(lib, ws=A + 4, ws_bytes=need) == -2
    # BADARG is answered first, the workspace last
    assert _backward(lib, ws_bytes=need, ins=None, D=6) == -1
    assert _backward(lib, ws=None, ws_bytes=need) == -3 and _backward(lib, ws_bytes=need - 1) == -3
    assert _backward(lib, ws_bytes=0, g_T_fwd=None, g_T_inv=None, g_ins=None) == -3                   # g_W alone, too


def test_workspace_size(lib):
    """The transposed weight [(2I+1)D, D], the products [2, I, M, D] and gnnrag_gemm_tn's chunk partials for (M, D, I D) of
    both directions, each rounded up to 256 bytes; 0 outside the limits and for a structure without facts; grows with
    rel_total."""
    up = lambda n: (n + 255) // 256 * 256                                      # noqa: E731
    q = lambda M, D, I: lib.gnnrag_relation_tables_backward_workspace_bytes(ctypes.byref(_csr(rel_total=M)), D, I)   # noqa: E731
    for M, D, I in ((1, 4, 1), (13, 52, 3), (200, 200, 2), (17001, 4, 1), (19200, 200, 2)):
        K = (2 * I + 1) * D
        tn = lib.gnnrag_gemm_tn_workspace_bytes(M, D, I * D)
        assert tn >= D * I * D * 4 and tn % (D * I * D * 4) == 0
        assert q(M, D, I) == up(K * D * 4) + up(2 * I * M * D * 4) + up(2 * tn), (M, D, I)
    for M, D, I in ((5, 6, 1), (5, 50, 2), (5, 0, 1), (5, 4, 0), (5, 1028, 1), (0, 4, 1), (-1, 4, 1)):
        assert q(M, D, I) == 0, (M, D, I)
    assert lib.gnnrag_relation_tables_backward_workspace_bytes(None, 4, 1) == 0
    sizes = [q(M, 200, 2) for M in (1, 100, 1000, 10000, 100000)]
    assert sizes == sorted(set(sizes))


def test_the_wrapper_refuses_cpu_tensors():
    from gnnrag_amd import _lib, ops
    c = ro.case(ROWS, R1, B, 4, 1)
    t = {k: torch.from_numpy(v) for k, v in c.items()}
    plan = types.SimpleNamespace(B=B, R1=R1, rel_total=len(ROWS), device=torch.device("cpu"))
    with pytest.raises(_lib.GnnragError, match="must live on the GPU"):
        ops.relation_tables_backward(plan, t["T_fwd"], t["T_inv"], t["ins"], t["W"], t["g_P"])


@pytest.mark.parametrize("math", [0, 1, 2])
def test_dense_form_names_the_products_of_the_backward(lib, math):
    from gnnrag_amd import ops
    # up to 16384 rows the skinny kernel (exact fp32 in every math mode, one launch), the k-tiled kernel above
    for M, D in ((1, 4), (13, 52), (200, 200), (16384, 4), (16384, 212)):
        f = ops.dense_form("rel_tables_dx", M, D, 2, math=math)
        assert f.family == f.block_family == ops.DENSE_SKINNY and f.launches == 1 and f.v4 == 1
    for M, D, nts in ((16385, 4, [4]), (17001, 4, [4]), (20000, 200, [13]), (20000, 212, [13, 4])):
        for blk, nt in enumerate(nts):
            f = ops.dense_form("rel_tables_dx", M, D, 2, math=math, block=blk)
            assert f.family == ops.DENSE_KTILED and f.launches == len(nts)
            assert (f.epi, f.nt, f.v4, f.v4out, f.n0) == (ops.DENSE_EPI_LINEAR, nt, 1, 1, 208 * blk)
            assert f.math == (math != 0)
        with pytest.raises(ops._lib.GnnragError):
            ops.dense_form("rel_tables_dx", M, D, 2, math=math, block=len(nts))
    f = ops.dense_form("rel_tables_dw", 17001, 4, 1, math=math)
    assert f.family == f.block_family == ops.DENSE_GEMM_TN and f.launches == 1
    with pytest.raises(ops._lib.GnnragError):
        ops.dense_form("rel_tables_dw", 17001, 4, 1, math=math, block=1)
    for entry in ("rel_tables_dx", "rel_tables_dw"):
        assert ops.dense_form(entry, 70, 50, 2, math=math).family == ops.DENSE_NONE
        assert ops.dense_form(entry, 70, 1028, 2, math=math).family == ops.DENSE_NONE
        assert ops.dense_form(entry, 70, 52, 2, math=math, misaligned=ops.DENSE_MISALIGNED_A).family == ops.DENSE_NONE


# -- the module layer ------------------------------------------------------------------------------------------------------

def test_the_switch_defaults_to_off_and_is_read_at_every_call(monkeypatch):
    """No GPU here: the method itself.  Unset and "0" leave the torch expression in place; "1" on CPU tensors is not
    eligible either, and the library is never called."""
    from gnnrag_amd import autograd
    from gnnrag_amd.modules.kg_reasoning import reasongnn as rg

    def no_library(*a, **k):
        raise AssertionError("the library was called on CPU tensors")
    monkeypatch.setattr(autograd.RelationTablesFn, "apply", staticmethod(no_library))
    monkeypatch.setattr(rg.RelationTablesFn, "apply", staticmethod(no_library))
    me = types.SimpleNamespace(plan=types.SimpleNamespace(rel_total=len(ROWS)))
    c = {k: torch.from_numpy(v) for k, v in ro.case(ROWS, R1, B, 4, 1).items()}
    looks, inside = [], [False]
    real_get = os.environ.get

    def get(k, *d):
        if inside[0]:
            looks.append(k)
        return real_get(k, *d)
    monkeypatch.setattr(rg.os.environ, "get", get)
    for value in (None, "0", "1", None):
        if value is None:
            monkeypatch.delenv("GNNRAG_HIP_REL_TABLES_TRAIN", raising=False)
        else:
            monkeypatch.setenv("GNNRAG_HIP_REL_TABLES_TRAIN", value)
        inside[0] = True
        got = rg.ReasonGNNLayer._relation_tables(me, c["T_fwd"], c["T_inv"], c["ins"], c["W"])
        inside[0] = False
        assert got is None
    assert looks == ["GNNRAG_HIP_REL_TABLES_TRAIN"] * 4
